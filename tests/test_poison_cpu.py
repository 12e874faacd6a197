"""CPU: poisoned-allocation runs (tests/_poison.py) of the product's HOST code on the test-only contract backend (tests/_cpu_backend.py).
Every path runs twice clean (A, B) and once with every torch.empty / empty_like / empty_strided / new_empty result, every hand-out of the persistent
scratch and every truncated cache row filled with 0xFF (P).  On the DEFINED outputs: A == B and P == A bit for bit, P finite, poison count > 0.
The positive controls show that the comparison flags the three ways a result can depend on unwritten memory.  (The kernels' side of the same
contract: tests/test_poison_gpu.py and the NaN-behind-the-bound cases of tests/test_kernels_gpu.py / test_kernels_emulated_cpu.py.)"""
import contextlib

import pytest
import torch

import _cpu_backend as CB
import _poison
from _poison import compare, poisoned_allocations
from _util import T, small_llama

torch.set_grad_enabled(False)


def abp(run, what):
    """run() three times — clean, clean, poisoned — and apply the comparison rules; returns the counts"""
    a, b = run(), run()
    with poisoned_allocations() as counts:
        p = run()
    print(f"{what}: {counts}")
    compare(a, b, p, counts, what)
    return counts


# ---- 1. the helper ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.float16, torch.bfloat16, torch.int32, torch.int8, torch.uint8])
def test_every_byte_is_ff_and_arguments_pass_through(dtype):
    with poisoned_allocations() as c:
        ts = [torch.empty(3, 5, dtype=dtype), torch.empty((3, 5), dtype=dtype, device="cpu"), torch.empty([2, 0, 4], dtype=dtype),
              torch.empty_like(torch.zeros(4, 6, dtype=dtype)), torch.empty_like(torch.zeros(4, 6), dtype=dtype),
              torch.empty_strided((3, 4), (1, 3), dtype=dtype), torch.zeros(2, dtype=torch.float32).new_empty((7,), dtype=dtype),
              torch.zeros(2, dtype=dtype).new_empty(2, 3), torch.empty(5, dtype=dtype, pin_memory=False)]
    assert [tuple(t.shape) for t in ts] == [(3, 5), (3, 5), (2, 0, 4), (4, 6), (4, 6), (3, 4), (7,), (2, 3), (5,)]
    assert ts[5].stride() == (1, 3) and all(t.dtype == dtype for t in ts)
    for t in ts:
        raw = torch.empty(0, dtype=torch.uint8).set_(t.untyped_storage(), 0, (t.untyped_storage().nbytes(),), (1,))
        assert bool((raw == 0xFF).all())
        if dtype.is_floating_point:
            assert bool(torch.isnan(t).all())
        elif t.numel():
            assert bool((t == (255 if dtype == torch.uint8 else -1)).all())
    assert c.allocations == 8 and c.refills == 0 and c.bytes == sum(t.untyped_storage().nbytes() for t in ts), "the empty tensor is not counted"


def test_names_are_restored_also_after_an_exception():
    from stllm_amd import hip
    from stllm_amd.models.llama import KVCache
    names = lambda: (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty, hip.split_workspace, KVCache.truncate)
    before = names()
    with poisoned_allocations():
        inside = names()
        assert all(i is not b for i, b in zip(inside, before))
    assert all(a is b for a, b in zip(names(), before))
    with pytest.raises(KeyError):
        with poisoned_allocations():
            raise KeyError("boom")
    assert all(a is b for a, b in zip(names(), before))
    x = torch.empty(4)
    assert x.shape == (4,)


def test_persistent_scratch_and_truncated_rows_are_refilled():
    from stllm_amd import hip
    from stllm_amd.models.llama import KVCache
    hip._split_ws.pop("cpu", None)
    try:
        first = hip.split_workspace("cpu", 64)
        first.zero_()
        with poisoned_allocations() as c:
            again = hip.split_workspace("cpu", 64)
            assert again is first and bool((again == 0xFF).all()) and (c.allocations, c.refills) == (0, 1), "a cached buffer: poisoned at the hand-out"
            again.zero_()
            assert bool((hip.split_workspace("cpu", 64) == 0xFF).all()) and c.refills == 2, "and at every later one"
            k = KVCache(2, 3, 6, 4, torch.float32, "cpu")
            n0 = c.allocations
            assert n0 == 2 and all(bool(torch.isnan(b).all()) for b in k.qkv)
            for b in k.qkv:
                b.fill_(1.0)
            k.len = 5
            k.truncate([5, 2, 4])
            for b in k.qkv:
                assert bool(torch.isfinite(b[0, :5]).all() and torch.isnan(b[1, 2:5]).all() and torch.isfinite(b[1, :2]).all() and torch.isnan(b[2, 4]).all())
                assert bool(torch.isfinite(b[:, 5]).all()), "the rows behind the old length were not the truncation's to poison"
            assert c.refills == 4
    finally:
        hip._split_ws.pop("cpu", None)


# ---- 2. positive controls: each way of depending on unwritten memory is flagged ----------------------------------------------------------------------
def _returns_an_unwritten_row():
    buf = torch.empty(4, 8)
    buf[:3] = torch.arange(24.0).view(3, 8)
    return buf          # row 3 was never written


def _multiplies_an_unwritten_row_by_zero():
    buf = torch.empty(4, 8)
    buf[:3] = torch.arange(24.0).view(3, 8)
    w = torch.tensor([0.5, 0.25, 0.25, 0.0])     # "a masked score of 0": 0 x NaN reaches the output
    return (w[:, None] * buf).sum(0)


_SCRATCH = {}


def _scratch(n):
    """a cached buffer in the style of hip.split_workspace"""
    buf = _SCRATCH.get("buf")
    if buf is None or buf.numel() < n:
        buf = _SCRATCH["buf"] = torch.empty(n)
    return buf


def _reads_cached_scratch_on_second_use(handout):
    def run():
        _SCRATCH.clear()
        out = []
        for call in range(2):
            ws = handout(8)
            if call == 0:
                ws.copy_(torch.arange(8.0))     # the first use writes the scratch ...
            out.append(ws.sum().clone())       # ... the second relies on what the first left behind
        return out
    return run


@pytest.mark.parametrize("toy", ["unwritten_row", "zero_times_unwritten", "stale_scratch"])
def test_positive_controls_fail_the_comparison(toy):
    if toy == "stale_scratch":
        # allocation-time poison alone does not see it (the first use overwrites the poison): the hand-out has to be re-filled, as hip.split_workspace is
        counts_box = []

        def handout(n):
            buf = _scratch(n)
            if counts_box:
                counts_box[0].refills += 1
                counts_box[0].bytes += _poison._fill_ff(buf, torch.empty)
            return buf
        run = _reads_cached_scratch_on_second_use(handout)
        a, b = run(), run()
        assert _poison.bits_equal(a, b)
        with poisoned_allocations() as c:
            p_alloc_only = run()
        assert _poison.bits_equal(p_alloc_only, a) and c.allocations == 1, "allocation-time poison alone: the stale read stays invisible"
        with poisoned_allocations() as c:
            counts_box.append(c)
            p = run()
        assert c.refills == 2
    else:
        run = {"unwritten_row": _returns_an_unwritten_row, "zero_times_unwritten": _multiplies_an_unwritten_row_by_zero}[toy]
        with poisoned_allocations(byte=0):   # the clean side: zeros, as in a fresh process (these toys READ unwritten memory: without this they would see
            a, b = run(), run()             # whatever block the allocator recycles — possibly one that an earlier test poisoned)
        with poisoned_allocations() as c:
            p = run()
        assert c.allocations == 1
    with pytest.raises(AssertionError, match="not finite|differs from the clean run"):
        compare(a, b, p, c, toy)
    with pytest.raises(AssertionError, match="not finite"):
        _poison.assert_finite(p)
    assert not _poison.bits_equal(p, a), "a bit difference between the clean and the poisoned call"


def test_a_path_that_poisons_nothing_fails_the_count():
    run = lambda: torch.zeros(3) + 1
    with poisoned_allocations() as c:
        p = run()
    with pytest.raises(AssertionError, match="nothing was poisoned"):
        compare(run(), run(), p, c, "zeros only")


# ---- 3. host paths on the contract backends ----------------------------------------------------------------------------------------------------------
SMALL = dict(num_hidden_layers=2, hidden_size=256, intermediate_size=768, num_attention_heads=2, vocab_size=512)   # tests/test_q4_cpu.py: both K % 128 == 0


@pytest.fixture(scope="module")
def small():
    return small_llama(SMALL, lm_head_spread=6.0)   # as tests/test_ragged_cpu.py: the rows take different paths


@pytest.fixture(scope="module")
def small_lora():
    return small_llama(SMALL, r=8, lm_head_spread=6.0)


EMB = lambda: T("poison.emb", (4, 40, 256), 0.05)
LENS = [9, 6, 9, 4]


def _live(cache):
    """the defined part of a cache: [q | k | v] columns... of which K and V of every row below its length (own buffers; local index = position - base_len)"""
    D = cache.hidden
    lens = cache.lens if cache.lens is not None else [cache.len] * cache.batch
    return [[buf[b, :n - cache.base_len, D:].clone() for b, n in enumerate(lens)] for buf in cache.qkv]


def _steps(model, cache, toks):
    out = []
    for t in range(toks.shape[1]):
        _, h16 = model.model.decode_step(toks[:, t:t + 1], cache)
        out.append(model.logits_from(h16, toks.shape[0], 1)[:, 0].float().clone())
    return out


def _mask(lens, S):
    return (torch.arange(S)[None, :] < torch.tensor(lens)[:, None]).long()


def _modes(dt, weights=None):
    from stllm_amd import runtime
    st = contextlib.ExitStack()
    st.enter_context(CB.installed())
    st.enter_context(runtime.use_dtype(dt))
    if weights:
        st.enter_context(runtime.use_decode_weights(weights))
    return st


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_prefill_right_padded_then_decode_steps(small, dt):
    """prefill with a right-padded mask into a cache (ragged), 4 decode steps; the pad rows of the prefill output and the cache rows behind a length are
    not defined outputs"""
    emb, lm = EMB(), small.model

    def run():
        c = lm.new_cache(4, 16, "cpu")
        h32, h16 = lm.prefill(emb[:, :9] * _mask(LENS, 9)[:, :, None].to(emb.device), _mask(LENS, 9), cache=c)
        assert c.lens == LENS
        hidden = [h32[b, :n].clone() for b, n in enumerate(LENS)]
        logits = _steps(small, c, emb[:, 9:13])
        return dict(hidden=hidden, logits=logits, cache=_live(c))
    with _modes(dt):
        counts = abp(run, f"prefill right-padded + 4 ragged steps, {dt}")
    assert counts.allocations >= 2 + 4 * 1, "the cache buffers and the dense scratch row of every ragged step"


def test_decode_step_uniform_ragged_with_a_restarted_row_and_shared(small):
    emb, lm = EMB(), small.model

    def run():
        out = {}
        u = lm.new_cache(2, 14, "cpu")
        lm.prefill(emb[:2, :8], None, cache=u)
        out["uniform"] = (_steps(small, u, emb[:2, 8:12]), _live(u))
        r = lm.new_cache(4, 16, "cpu")
        lm.prefill(emb[:, :9], _mask(LENS, 9), cache=r)
        r.truncate([9, 0, 9, 4])                                        # row 1: a freed slot that starts over at position 0 — the 6 rows it held are
        out["ragged"] = (_steps(small, r, emb[:, 9:13]), _live(r))      # undefined again (poisoned by the truncation)
        base = lm.new_cache(1, 13, "cpu")
        lm.prefill(emb[:1, :13], None, cache=base)
        s = base.share(rows=4, max_new=5 + 4)
        _, hs = lm.extend(emb[:, 13:18], s, lengths=[5, 1, 5, 3])
        out["shared"] = ([hs.view(4, 5, -1)[b, :n].clone() for b, n in enumerate([5, 1, 5, 3])], _steps(small, s, emb[:, 20:24]), _live(s), _live(base))
        return out
    with _modes("fp32"):
        counts = abp(run, "decode_step: uniform / ragged + restarted row / shared base")
    assert counts.refills >= 1, "the rows forgotten by truncate() are undefined again"


def test_extend_uniform_and_lengths(small, monkeypatch):
    from stllm_amd.models import llama
    emb, lm = EMB(), small.model

    def run():
        out = {}
        for entry in (True, False):                                     # the one-call stack entry | the per-op body
            monkeypatch.setattr(llama, "STACK_ENTRY", entry)
            c = lm.new_cache(2, 20, "cpu")
            lm.prefill(emb[:2, :7], None, cache=c)
            h32, _ = lm.extend(emb[:2, 7:12], c)
            out[f"uniform{entry}"] = (h32.clone(), _live(c))
        c = lm.new_cache(4, 20, "cpu")
        lm.prefill(emb[:, :7], None, cache=c)
        sfx = [5, 2, 4, 1]
        h32, _ = lm.extend(emb[:, 7:12], c, lengths=sfx)
        assert c.lens == [7 + n for n in sfx]
        out["lengths"] = ([h32[b, :n].clone() for b, n in enumerate(sfx)], _live(c), _steps(small, c, emb[:, 12:14]))
        return out
    with _modes("fp32"):
        abp(run, "extend: stack entry / per-op / lengths=")


GEN = dict(max_new_tokens=5, do_sample=False, min_length=1)


def _gen_cases(model, emb):
    """the generate() calls of the poisoned runs, on emb's device and width: emb [4, >= 32, D]"""
    D, dev = emb.shape[-1], emb.device
    S = max(LENS)
    pad = emb[:, :S] * _mask(LENS, S)[:, :, None].to(dev)            # right-padded rows of LENS tokens, zeros behind them
    mask = _mask(LENS, S)
    prefix = model.model.new_cache(1, 7, dev)
    model.model.prefill(emb[:1, 20:27], None, cache=prefix)
    qs, qmask = emb[:3, 27:32] * _mask([5, 2, 4], 5)[:, :, None].to(dev), _mask([5, 2, 4], 5)
    return {
        "greedy": dict(inputs_embeds=emb[:1, :9]),
        "5 beams": dict(inputs_embeds=emb[:1, :9], num_beams=5, repetition_penalty=1.2),
        "groups": dict(inputs_embeds=pad, attention_mask=mask),
        "ragged": dict(inputs_embeds=pad, attention_mask=mask, batching="ragged"),
        "ragged, 3 beams": dict(inputs_embeds=pad, attention_mask=mask, batching="ragged", num_beams=3),
        "prefix_cache": dict(inputs_embeds=emb[:1, 27:32], prefix_cache=prefix),
        "share_prefix, 5 beams": dict(inputs_embeds=emb[:1, :9], num_beams=5, share_prefix=True),
        "share_prefix, ragged questions": dict(inputs_embeds=qs, attention_mask=qmask, prefix_cache=prefix, batching="ragged", share_prefix=True),
    }, prefix


def _gen_run(model, emb, only=None):
    def run():
        cases, prefix = _gen_cases(model, emb)
        before = [b.clone() for b in prefix.qkv]
        out = {k: model.generate(**kw, **GEN) for k, kw in cases.items() if only is None or k in only}
        out["prefix"] = [b[:, :7, b.shape[-1] // 3:].clone() for b in prefix.qkv]
        assert all(torch.equal(x[:, :7], y[:, :7]) for x, y in zip(prefix.qkv, before))
        return out
    return run


def test_generate(small):
    with _modes("fp32"):
        abp(_gen_run(small, EMB()), "generate: greedy / beams / groups / ragged / prefix_cache / share_prefix, fp32")


@pytest.mark.parametrize("weights", ["int8", "int4g128"])
def test_quantised_decode_and_generate(small, weights):
    emb, lm = EMB(), small.model

    def run():
        c = lm.new_cache(2, 14, "cpu")
        lm.prefill(emb[:2, :8], None, cache=c)
        out = dict(steps=_steps(small, c, emb[:2, 8:12]), cache=_live(c))
        out.update(_gen_run(small, emb, only=("greedy", "5 beams", "ragged", "share_prefix, ragged questions"))())
        return out
    with _modes("bf16", weights):
        abp(run, f"decode_step + generate, {weights}")


def test_active_lora_adapter(small_lora):
    emb, lm = EMB(), small_lora.model

    def run():
        c = lm.new_cache(2, 20, "cpu")
        h32, _ = lm.prefill(emb[:2, :8], None, cache=c)
        e32, _ = lm.extend(emb[:2, 8:11], c)
        out = dict(prefill=h32.clone(), extend=e32.clone(), steps=_steps(small_lora, c, emb[:2, 11:14]), cache=_live(c))
        out.update(_gen_run(small_lora, emb, only=("greedy", "ragged", "prefix_cache"))())
        return out
    with _modes("fp32"):
        counts = abp(run, "active LoRA adapters")
    assert counts.allocations > 0


def test_train_step():
    """one training.train_step (mean pooling, 1 LLM layer: the model of tests/test_backward_cpu.py::test_mean_pooling_backward_and_one_optimizer_step):
    loss, gradient norm, every parameter and the AdamW state after the step"""
    import _cpu_backend
    from test_host_orchestration_cpu import CFGS, build, make_inputs
    from stllm_amd import runtime, training
    samples, _ = make_inputs(2, 2, False)
    model = build(CFGS["mean_pooling"], vit_depth=1, qf_layers=2, llm_layers=1)
    start = {k: v.detach().clone() for k, v in model.state_dict().items()}

    def run():
        model.load_state_dict(start)          # (in place: the step before moved the masters; loading drops every packed copy)
        opt = training.AdamW(list(training.trainable_parameters(model)), lr=1e-3, max_grad_norm=1.0)
        loss, _, norm = training.train_step(model, samples, opt)
        state = {k: v.clone() for k, v in vars(opt).items() if isinstance(v, torch.Tensor)}
        return dict(loss=loss.clone(), norm=float(norm), params={n: p.detach().clone() for n, p in training.trainable_parameters(model)}, state=state)
    with _cpu_backend.installed(), runtime.use_dtype("fp32"):
        counts = abp(run, "training.train_step")
    assert counts.allocations > 0
