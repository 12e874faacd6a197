"""CPU: the shared-prefix KV cache — KVCache.share bookkeeping, decode steps / extend on a cache with a base against forked copies,
generate(share_prefix=True) and Chat.answer_many(share_prefix=True) on the test-only contract backend (tests/_cpu_backend.py, fp32), the entry
points a shared step calls, the error paths, and the new 16-bit decode kernels + merge executed from source by the host emulator (tests/hipemu)."""
import numpy as np
import pytest
import torch

import _cpu_backend as CB
import _hipemu
import _shared_case as SC
from _util import T, small_llama
from test_ragged_cpu import CFG, SMALL, UNIFORM_LAYER, _build, _padded

torch.set_grad_enabled(False)
needs_emu = pytest.mark.skipif(not _hipemu.available() or _hipemu.ON_DEVICE, reason="ROCm clang++ not found: cannot build the emulated kernels")
OUT_TOL = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -10}   # tests/test_kernels_gpu.py OUT_TOL (importing that module would need a device)


@pytest.fixture(scope="module")
def stllm():
    m = _build(CFG)
    m.lm_head.weight.mul_(6.0)
    return m


def _logits(model, cache, toks):
    out = []
    for t in range(toks.shape[1]):
        _, h16 = model.model.decode_step(toks[:, t:t + 1], cache)
        out.append(model.logits_from(h16, toks.shape[0], 1)[:, 0].float().clone())
    return out


# ---- 1. bookkeeping --------------------------------------------------------------------------------------------------------------------------------
def test_share_bookkeeping():
    from stllm_amd import runtime
    from stllm_amd.models.llama import KVCache
    model = small_llama(SMALL)
    lm = model.model
    emb = T("shared.emb", (2, 24, 256), 0.05)
    with CB.installed(), runtime.use_dtype("fp32"):
        base = lm.new_cache(2, 7, "cpu")
        lm.prefill(emb[:, :7], None, cache=base)
        keep = [b.clone() for b in base.qkv]
        s = base.share(rows=6, max_new=12)
        assert s.base is base and s.base_len == 7 and s.len == 7 and s.lens is None and s.batch == 6 and s.max_len == 19
        assert all(x.data_ptr() == y.data_ptr() for x, y in zip(s.base.qkv, base.qkv)), "the base is the same storage"
        assert all(tuple(b.shape) == (6, 12, 3 * 256) for b in s.qkv), "own buffers hold the positions behind the base only"
        # group mapping: rows 0-2 read base row 0, rows 3-5 base row 1 — the same tokens behind different base rows give different rows, equal inside a group
        q = emb[:1, 7:10].expand(6, 3, 256).contiguous()
        _, h = lm.extend(q, s)
        h = h.view(6, 3, -1)
        assert torch.equal(h[0], h[1]) and torch.equal(h[0], h[2]) and torch.equal(h[3], h[5]) and not torch.equal(h[0], h[3])
        assert s.len == 10
        toks = emb[:1, 10:14].expand(6, 4, 256).contiguous()
        _logits(model, s, toks)
        assert s.len == 14 and all(torch.equal(x, y) for x, y in zip(base.qkv, keep)), "the base is unchanged after extend + 4 steps"
        assert base.len == 7
        # share of a cache with a base: the same base, copies of the suffix rows
        s2 = s.share(rows=12)
        assert s2.base is base and s2.batch == 12 and s2.len == 14 and s2.max_len == s.max_len
        for x, y in zip(s.qkv, s2.qkv):
            assert torch.equal(y[:, :7], x[:, :7].repeat_interleave(2, dim=0))
        # fork materialises a dense private copy
        f = s.fork(rows=12, max_len=30)
        assert f.base is None and f.len == 14 and f.batch == 12
        for x, pre, y in zip(s.qkv, base.qkv, f.qkv):
            assert torch.equal(y[:, :7], pre[:, :7].repeat_interleave(6, dim=0)) and torch.equal(y[:, 7:14], x[:, :7].repeat_interleave(2, dim=0))
        # the dense copy decodes what the shared cache decodes
        tok = emb[:1, 14:15].expand(6, 1, 256).contiguous()
        a = _logits(model, s.fork(), tok)[0]
        b = _logits(model, s, tok)[0]
        assert float((a - b).abs().max()) <= 1e-5 * float(a.abs().max())
        # truncate: not into the base
        s.truncate(9)
        assert s.len == 9
        s.truncate([9, 8, 7, 9, 9, 9])
        assert s.lens == [9, 8, 7, 9, 9, 9]
        with pytest.raises(AssertionError, match="shared base"):
            s.truncate(6)
        with pytest.raises(AssertionError, match="shared base"):
            s.truncate([9, 8, 6, 9, 9, 9])
        r = s.share(rows=12)
        assert r.lens == [9, 9, 8, 8, 7, 7, 9, 9, 9, 9, 9, 9], "the beams of a ragged batch inherit their row's length"
    # the beam re-ordering moves the positions behind the base only
    from stllm_amd import generation
    c = KVCache(1, 1, 4, 8, torch.float32, "cpu")
    c.qkv[0].copy_(torch.arange(c.qkv[0].numel()).view_as(c.qkv[0]).float())
    c.len = 4
    sh = c.share(rows=3, max_new=5)
    sh.qkv[0].copy_(torch.arange(sh.qkv[0].numel()).view_as(sh.qkv[0]).float())
    sh.len = 6                                   # 2 positions behind the base
    before, cb = sh.qkv[0].clone(), c.qkv[0].clone()

    class _LM:
        embed_tokens = staticmethod(lambda ids: torch.zeros(ids.shape[0], 1, 8))

        @staticmethod
        def decode_step(tok, cache):
            raise StopIteration
    st = generation._CacheStepper.__new__(generation._CacheStepper)
    st.m, st.lm, st.use_cache, st.cache = None, _LM, True, sh
    with pytest.raises(StopIteration):
        st.advance(torch.zeros(3, dtype=torch.long), torch.tensor([2, 0, 0]))
    assert torch.equal(sh.qkv[0][:, :2], before[[2, 0, 0], :2]) and torch.equal(sh.qkv[0][:, 2:], before[:, 2:]) and torch.equal(c.qkv[0], cb)


# ---- 2. decode steps -------------------------------------------------------------------------------------------------------------------------------
def test_shared_decode_steps_equal_forked_copies():
    """2 layers, P = 13, suffix lengths [5, 1, 5, 3], 6 steps: the logits on the shared cache equal those on a fork()ed (dense, private) copy to fp32
    round-off — the backend's attention_shared sums in fp64 over the concatenated keys, the copy path in fp32 over the same keys"""
    from stllm_amd import runtime
    model = small_llama(SMALL)
    lm = model.model
    P, sfx, steps = 13, [5, 1, 5, 3], 6
    emb = T("shared.emb2", (4, 32, 256), 0.05)
    with CB.installed(), runtime.use_dtype("fp32"):
        base = lm.new_cache(1, P, "cpu")
        lm.prefill(emb[:1, :P], None, cache=base)
        keep = [b.clone() for b in base.qkv]
        s = base.share(rows=4, max_new=5 + steps)
        _, hs = lm.extend(emb[:, P:P + 5], s, lengths=sfx)
        assert s.lens == [P + n for n in sfx] and s.len == P + 5
        f = base.fork(rows=4, max_len=P + 5 + steps)
        _, hf = lm.extend(emb[:, P:P + 5], f, lengths=sfx)
        for b, n in enumerate(sfx):
            assert torch.allclose(hs.view(4, 5, -1)[b, :n], hf.view(4, 5, -1)[b, :n], atol=1e-5)
        toks = emb[:, 20:20 + steps]
        got, want = _logits(model, s, toks), _logits(model, f, toks)
        for t in range(steps):
            err, scale = float((got[t] - want[t]).abs().max()), float(want[t].abs().max())
            assert err <= 1e-5 * scale, (t, err, scale)
        assert s.lens == [P + n + steps for n in sfx] == f.lens
        assert all(torch.equal(x, y) for x, y in zip(base.qkv, keep))
        # a multi-token extend behind a non-empty UNIFORM suffix (sfx_q_off > 0)
        u, fu = base.share(rows=2, max_new=9), base.fork(rows=2, max_len=P + 9)
        for c in (u, fu):
            lm.extend(emb[:2, P:P + 3], c)
        _, h1 = lm.extend(emb[:2, P + 3:P + 7], u)
        _, h2 = lm.extend(emb[:2, P + 3:P + 7], fu)
        assert u.len == P + 7 and torch.allclose(h1, h2, atol=1e-5)


# ---- 3. generate -----------------------------------------------------------------------------------------------------------------------------------
def test_generate_share_prefix_returns_the_same_ids(stllm):
    from stllm_amd import runtime
    model = stllm
    video = T("gen.ragged_prefix", (1, 7, 4096), 0.05)
    qs = [T(f"gen.ragged_q{i}", (n, 4096), 0.05) for i, n in enumerate([5, 2, 4])]
    emb, mask = _padded(qs, "right")
    whole = torch.cat([video[0], qs[0]])[None]
    k = dict(max_new_tokens=5, do_sample=False, min_length=1)
    with CB.installed(), runtime.use_dtype("fp32"):
        prefix = model.model.new_cache(1, 7, "cpu")
        model.model.prefill(video, None, cache=prefix)
        before = [b.clone() for b in prefix.qkv]
        cases = [("greedy", dict(inputs_embeds=whole), False),
                 ("5 beams", dict(inputs_embeds=whole, num_beams=5, repetition_penalty=1.2), True),
                 ("prefix_cache", dict(inputs_embeds=qs[0][None], prefix_cache=prefix), True),
                 ("prefix_cache, 3 beams", dict(inputs_embeds=qs[0][None], prefix_cache=prefix, num_beams=3), True),
                 ("ragged, one shared prefix row", dict(inputs_embeds=emb, attention_mask=mask, prefix_cache=prefix, batching="ragged"), True),
                 ("ragged with beams", dict(inputs_embeds=emb, attention_mask=mask, prefix_cache=prefix, batching="ragged", num_beams=3, repetition_penalty=1.2), True)]
        for what, kw, shares in cases:
            want = model.generate(**kw, **k)
            with CB.counting() as calls:
                got = model.generate(share_prefix=True, **kw, **k)
                assert ("attention_shared" in calls) == shares, (what, "greedy without a prefix has nothing to share")
            assert torch.equal(got, want), what
        assert prefix.len == 7 and prefix.lens is None and all(torch.equal(x, y) for x, y in zip(prefix.qkv, before))


# ---- 4. Chat ---------------------------------------------------------------------------------------------------------------------------------------
def test_chat_answer_many_share_prefix(stllm):
    from stllm_amd import runtime
    from stllm_amd.conversation import Chat
    model = stllm
    frames = T("input.frames2", (2, 3, 224, 224))
    questions = [[21, 22, 23], [400, 17, 9000, 5, 77], [9]]
    with CB.installed(), runtime.use_dtype("fp32"):
        chat = Chat(model, device="cpu")
        img_list = []
        chat.upload_video(frames.view(6, 224, 224), None, img_list)
        prefix = chat.prefill_video(img_list)
        before = [b.clone() for b in prefix.cache.qkv]
        for kw in (dict(num_beams=1), dict(num_beams=3)):
            k = dict(max_new_tokens=6, do_sample=False, **kw)
            want = [chat.answer(img_list, q, **k) for q in questions]
            with CB.counting() as calls:
                got = chat.answer_many(img_list, questions, prefix=prefix, share_prefix=True, **k)
                assert "attention_shared" in calls
            for (t0, i0), (t1, i1) in zip(want, got):
                assert np.array_equal(i0, i1) and t0 == t1, (kw, i0, i1)
            one = chat.answer(img_list, questions[1], prefix=prefix, share_prefix=True, **k)
            assert np.array_equal(one[1], want[1][1])
        assert all(torch.equal(x, y) for x, y in zip(prefix.cache.qkv, before))


# ---- 5. the calls of a step ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["plain", "int8", "lora"])
def test_shared_step_calls_attention_shared_once_per_layer(mode):
    import contextlib
    from stllm_amd import runtime
    model = small_llama(SMALL, r=8 if mode == "lora" else 0)
    lm = model.model
    emb = T("ragged.emb", (3, 12, 256), 0.05)
    dt = "fp32" if mode == "plain" else "bf16"
    ctx = runtime.use_decode_weights("int8") if mode == "int8" else contextlib.nullcontext()
    with CB.installed(), runtime.use_dtype(dt), ctx:
        c = lm.new_cache(1, 8, "cpu")
        lm.prefill(emb[:1, :8], None, cache=c)
        u = c.fork(rows=3, max_len=16)
        with CB.counting() as calls:
            _, h_u = lm.decode_step(emb[:, 8:9], u)
            uniform = list(calls)
        if mode == "plain":
            assert uniform == UNIFORM_LAYER * 2 + ["rmsnorm"], "base is None: the calls of the step before this feature"
        assert "attention_shared" not in uniform and uniform.count("attention") == 2
        s = c.share(rows=3, max_new=8)
        with CB.counting() as calls:
            _, h_s = lm.decode_step(emb[:, 8:9], s)
            shared = list(calls)
        assert shared.count("attention_shared") == 2 and "attention" not in shared and shared.count("kv_append_rows") == 2
        want = ["gather_rows", "gather_rows"] + [n for n in uniform if n != "attention"]
        assert [n for n in shared if n not in ("attention_shared", "kv_append_rows")] == want, shared
        assert ("gemv_w8" in shared) == (mode == "int8") and ("lora_down" in shared) == (mode == "lora")
        tol = 1e-5 if mode == "plain" else 2.0 ** -7          # 16-bit: one rounding step of the hidden row
        assert float((h_s.float() - h_u.float()).abs().max()) <= tol * float(h_u.float().abs().max())
        assert s.len == 9 and s.lens is None, "a uniform suffix stays uniform"


# ---- 6. error paths --------------------------------------------------------------------------------------------------------------------------------
def test_shared_error_paths(stllm):
    from stllm_amd import runtime
    model = small_llama(SMALL)
    lm = model.model
    emb = T("shared.emb", (2, 24, 256), 0.05)
    with CB.installed(), runtime.use_dtype("fp32"):
        base = lm.new_cache(1, 7, "cpu")
        lm.prefill(emb[:1, :7], None, cache=base)
        s = base.share(rows=2, max_new=10)
        lm.extend(emb[:, 7:10], s, lengths=[3, 1])
        with pytest.raises(NotImplementedError, match="ragged prefix"):
            lm.extend(emb[:, 10:12], s)                                        # extend behind a ragged suffix
        rag = lm.new_cache(2, 12, "cpu")
        lm.prefill(emb[:, :5], torch.tensor([[1] * 5, [1] * 3 + [0] * 2]), cache=rag)
        with pytest.raises(NotImplementedError, match="uniform"):
            rag.share(rows=2, max_new=4)                                       # a ragged base
        with pytest.raises(NotImplementedError, match="shared base"):
            lm.forward(inputs_embeds=emb[:, 12:13], past_key_values=s)
        with pytest.raises(ValueError, match="use_cache"):
            stllm.generate(inputs_embeds=T("gen.ragged_q0", (1, 5, 4096), 0.05), max_new_tokens=2, use_cache=False, share_prefix=True)
    with CB.installed(), runtime.use_dtype("fp32"):
        u = base.share(rows=2, max_new=4)
    with runtime.use_dtype("bf16x3"):
        with pytest.raises(NotImplementedError, match="bf16x3"):
            lm.decode_step(emb[:, :1], u)
        with pytest.raises(NotImplementedError, match="bf16x3"):
            lm.extend(emb[:, :2], u)


# ---- 7. the 16-bit decode kernels and the merge, from source, on the host emulator -------------------------------------------------------------------
@needs_emu
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_emulated_shared_decode_attention(dtype):
    """stllm_attention_shared, Sq = 1: H = 2, G = 2, R = 3, P = 45 (a masked last tile: keys 45 .. 63 are neither loaded nor counted), suffix lengths
    [1, 7, 33, 2, 9, 1]; everything behind the bounds is NaN.  Against fp64 over the concatenated live keys within 2 x OUT_TOL (the bound of the split-and-
    merge decode attention tests); the prefix buffers are not written; two calls give the same bits."""
    td = {"bf16": torch.bfloat16, "fp16": torch.float16}[dtype]
    G, R, H, P, sfx = 2, 3, 2, 45, [1, 7, 33, 2, 9, 1]
    pre, suf, q = SC.make(td, G, R, H, P, sfx)
    keep = pre.clone()
    want, _ = SC.reference(pre, suf, q, G, R, H, P, sfx)
    with _hipemu.emulated() as hip:
        assert hasattr(hip.lib(), "stllm_attention_shared"), "the emulated library exports the new entry point"
        got = SC.call(hip, pre, suf, q, G, R, H, P, sfx)
        again = SC.call(hip, pre, suf, q, G, R, H, P, sfx)
        with pytest.raises(RuntimeError, match="unsupported"):
            hip.attention_shared(q[:, :64], pre.view(-1, pre.shape[-1])[:, :64], pre.view(-1, pre.shape[-1])[:, :64], suf.view(-1, suf.shape[-1])[:, :64],
                                 suf.view(-1, suf.shape[-1])[:, :64], B=6, G=2, H=1, Sq=1, P=P, D=64, scale=1.0, max_sfx=33)
    assert torch.isfinite(got.float()).all(), "nothing behind P or behind a suffix length was read"
    assert torch.equal(got, again) and torch.equal(torch.nan_to_num(pre.float()), torch.nan_to_num(keep.float()))
    scale = float(want.abs().max())
    for b in range(G * R):
        err = float((got[b].double() - want[b]).abs().max())
        print(f"shared decode attention {dtype} row {b} (suffix {sfx[b]}): err {err:.3e} / abs-max {scale:.3e}")
        assert err <= 2 * OUT_TOL[dtype] * scale, (b, err, scale)


@needs_emu
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_emulated_shared_extend_attention(dtype):
    """stllm_attention_shared, Sq > 1 (extend(lengths=) behind a shared base): H = 1, G = 1, R = 3, P = 33, Sq = 8 causal query rows per batch row, ragged
    suffix lengths [8, 5, 1] — the suffix pass is attn_mfma_kernel with LIVE loads, the only tile-kernel instantiation that does not load the key rows
    behind a row's length.  Everything behind P and behind every suffix length is NaN, and the partial-state workspace is poisoned: the live query rows
    against fp64 within 2 x OUT_TOL (the bound of tests/test_shared_prefix_gpu.py::test_attention_shared_extend), finite."""
    import _poison
    td = {"bf16": torch.bfloat16, "fp16": torch.float16}[dtype]
    G, R, H, P, Sq, sfx = 1, 3, 1, 33, 8, [8, 5, 1]
    pre, suf, q = SC.make(td, G, R, H, P, sfx, Sq=Sq)
    want, live = SC.reference(pre, suf, q, G, R, H, P, sfx, Sq=Sq, causal=True, q_off=0)
    with _hipemu.emulated() as hip:
        with _poison.poisoned_allocations() as counts:
            got = SC.call(hip, pre, suf, q, G, R, H, P, sfx, Sq=Sq, causal=True, q_off=0)
    live = live.reshape(-1)
    assert counts.count > 0
    assert torch.isfinite(got[live].float()).all(), "something behind P or behind a suffix length was read"
    scale = float(want.abs().max())
    err = float((got[live].double() - want[live]).abs().max())
    print(f"shared extend attention {dtype}: err {err:.3e} / abs-max {scale:.3e}")
    assert err <= 2 * OUT_TOL[dtype] * scale, (err, scale)
