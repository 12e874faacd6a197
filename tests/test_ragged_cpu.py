"""CPU: the ragged KV cache — decode attention with per-row lengths and the KV append scatter on the host emulator of the real sources (tests/hipemu),
KVCache.lens, ragged prefill / extend / decode_step, generate(batching="ragged"), Chat.answer_many on the test-only contract backend
(tests/_cpu_backend.py, fp32), and the C ABI surface."""
import os
import re

import numpy as np
import pytest
import torch

import _cpu_backend as CB
import _hipemu
from _util import T, small_llama

torch.set_grad_enabled(False)
EMU_TOL = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}   # tests/test_kernels_emulated_cpu.py TOL: one rounding step of the 16-bit output
CFG = dict(vit_model="eva_clip_g", image_size=224, num_query_token=32, video_input="mean", use_mask=False, mvm_decode=False,
           qformer_text_input=False, max_txt_len=32, end_sym=" 2")
SMALL = dict(num_hidden_layers=2, hidden_size=256, intermediate_size=704, num_attention_heads=2, vocab_size=512)
needs_emu = pytest.mark.skipif(not _hipemu.available() or _hipemu.ON_DEVICE, reason="ROCm clang++ not found: cannot build the emulated kernels")


def rnd(*shape, seed=0, dtype=torch.float32, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def fp64_rows(q, cache, lens, H, D):
    """softmax(scale q K^T) V in fp64 of the same 16-bit inputs, row b over its own keys [0, lens[b]); zeros for an empty row"""
    B, HD = q.shape[0], H * D
    out = torch.zeros(B, HD, dtype=torch.float64)
    for b, n in enumerate(lens):
        if n <= 0:
            continue
        qb = q[b, :HD].double().view(H, 1, D)
        kb = cache[b, :n, HD:2 * HD].double().view(n, H, D).transpose(0, 1)
        vb = cache[b, :n, 2 * HD:].double().view(n, H, D).transpose(0, 1)
        out[b] = ((qb @ kb.transpose(-1, -2) * D ** -0.5).softmax(-1) @ vb).reshape(HD)
    return out


# ---- 1. the kernels, emulated from source ----------------------------------------------------------------------------------------------------------
RAGGED_CASES = [
    # (lens, attn_decode_single, what): max(lens) <= 1536 with the option on -> the single-pass kernel; option off, or max(lens) > 1536 -> the split-KV pair
    ([1, 3, 5, 0, 100, 64], 1, "single pass: 1 key, just below / above one wave quad (4 keys), a free slot, two longer rows"),
    ([1, 3, 5, 0, 100, 49], 0, "split pair: the same lengths, 1 - 3 splits per row"),
    ([100, 1600, 0, 47], 1, "a mix that straddles the single / split boundary (1536): the host takes the split pair for every row"),
]


@needs_emu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("lens,single,what", RAGGED_CASES)
def test_emulated_ragged_decode_attention(dtype, lens, single, what):
    """stllm_attention_decode_ragged (attn_decode_single_ragged / attn_decode_partial_ragged + attn_decode_merge_ragged) on a strided cache with q in a dense
    scratch row: every row against fp64 of the same 16-bit inputs (the bound of test_emulated_split_kv_decode_attention: 2 x one output rounding step), a
    zero-length row gives zeros, and every row is bit-identical to stllm_attention_decode on that row alone with Skv = lens[b] when both take one schedule"""
    import _poison
    B, H, D = len(lens), 1, 128
    HD = H * D
    ML = max(lens) + 3
    cache = rnd(B, ML, 3 * HD, seed=300 + len(lens), dtype=dtype, scale=0.6)
    q = rnd(B, 3 * HD, seed=301, dtype=dtype, scale=0.6)
    for b, n in enumerate(lens):
        cache[b, n:] = float("nan")                             # the rows at or behind a row's length are uninitialised memory: never read
        if n == 0:
            q[b] = float("nan")                                 # ... and so is the query of a free slot
    kv_len = torch.tensor(lens, dtype=torch.int32)
    flat = cache.view(B * ML, 3 * HD)
    strides = (ML * 3 * HD, 3 * HD)
    want = fp64_rows(q, cache, lens, H, D)
    g = _poison.Guarded(B, HD, dtype)                           # the output starts as 0xFF (NaN) inside a 0xFF-filled buffer: a free slot must still read zeros
    with _hipemu.emulated() as hip:
        hip.set_option("attn_decode_single", single)
        try:
            with _poison.poisoned_allocations() as counts:      # the partial-state workspace: 0xFF in every byte (a merge that read an unwritten record would see it)
                got = hip.attention_decode_ragged(q[:, :HD], flat[:, HD:2 * HD], flat[:, 2 * HD:], kv_len, B=B, H=H, max_kv=max(lens), D=D, scale=D ** -0.5,
                                                  q_stride=3 * HD, k_strides=strides, v_strides=strides, out=g.out)
                routed = hip.attention(q[:, :HD], flat[:, HD:2 * HD], flat[:, 2 * HD:], B=B, H=H, Sq=1, Skv=max(lens), D=D, scale=D ** -0.5, kv_len=kv_len,
                                       q_strides=(3 * HD, 3 * HD), k_strides=strides, v_strides=strides)
            assert counts.allocations >= 2 and g.intact(), "no byte around the output rows was written"
            assert torch.equal(got, routed), "hip.attention(Sq=1, kv_len=...) routes to the ragged decode kernels"
            split_all = single == 0 or max(lens) > 1536
            for b, n in enumerate(lens):
                if n == 0:
                    assert float(got[b].float().abs().max()) == 0.0, "a free slot writes zeros, not NaN"
                    continue
                same_schedule = split_all == (single == 0 or n > 1536)
                if not same_schedule:
                    continue
                alone = hip.attention(q[b:b + 1, :HD], cache[b][:, HD:2 * HD], cache[b][:, 2 * HD:], B=1, H=H, Sq=1, Skv=n, D=D, scale=D ** -0.5,
                                      q_strides=(3 * HD, 3 * HD), k_strides=strides, v_strides=strides)
                assert torch.equal(got[b], alone[0]), (what, b, n)
        finally:
            hip.set_option("attn_decode_single", 1)
    assert not torch.isnan(got.float()).any()
    scale = max(want.abs().max().item(), 1e-6)
    for b in range(B):
        err = (got[b].double() - want[b]).abs().max().item()
        print(f"ragged decode attention {dtype} lens[{b}]={lens[b]} single={single}: err {err:.3e} / abs-max {scale:.3e}")
        assert err <= 2 * EMU_TOL[dtype] * scale, (what, b, lens[b], err, scale)


@needs_emu
def test_emulated_ragged_decode_rejects_what_it_does_not_serve():
    """fp32 / another head_dim: STLLM_ERR_UNSUPPORTED with a message, never a fallback"""
    q, c = rnd(2, 3 * 128), rnd(2 * 8, 3 * 128)
    kv_len = torch.tensor([3, 5], dtype=torch.int32)
    with _hipemu.emulated() as hip:
        with pytest.raises(RuntimeError, match="unsupported"):
            hip.attention_decode_ragged(q[:, :128], c[:, 128:256], c[:, 256:], kv_len, B=2, H=1, max_kv=5, D=128, scale=1.0, q_stride=384,
                                        k_strides=(8 * 384, 384), v_strides=(8 * 384, 384))
        with pytest.raises(RuntimeError, match="unsupported"):
            hip.attention_decode_ragged(q[:, :128].bfloat16(), c[:, 128:256].bfloat16(), c[:, 256:].bfloat16(), kv_len, B=2, H=2, max_kv=5, D=64, scale=1.0,
                                        q_stride=384, k_strides=(8 * 384, 384), v_strides=(8 * 384, 384))


@needs_emu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("with_q", [False, True])
def test_emulated_kv_append_rows(dtype, with_q):
    """stllm_kv_append_rows: exact; q columns of the target rows and every other cache row untouched; a position outside [0, max_len) writes nothing"""
    B, ML, hidden = 5, 7, 136                                   # 3 * 136 * 2 bytes = 816 = 51 x 16: a partial last workgroup
    cache = rnd(B, ML + 1, 3 * hidden, seed=310, dtype=dtype)[:, :ML]   # batch stride > max_len * row stride
    src = rnd(B, 3 * hidden, seed=311, dtype=dtype)
    pos = torch.tensor([0, 6, 3, -1, 7], dtype=torch.int32)     # rows 3 and 4: free slots (negative / == max_len)
    want = cache.clone()
    c0 = 0 if with_q else hidden
    for b, p in enumerate(pos.tolist()):
        if 0 <= p < ML:
            want[b, p, c0:] = src[b, c0:]
    with _hipemu.emulated() as hip:
        hip.kv_append_rows(src, cache, pos, with_q=with_q)
    assert torch.equal(cache, want)
    ref = rnd(B, ML + 1, 3 * hidden, seed=310, dtype=dtype)
    assert torch.equal(cache[3], ref[3, :ML]) and torch.equal(cache[4], ref[4, :ML])
    got = ref[:, :ML].clone()
    CB.kv_append_rows(src, got, pos, with_q=with_q)              # the contract backend restates the same thing
    assert torch.equal(got, want)


# ---- models ----------------------------------------------------------------------------------------------------------------------------------------
def _build(cfg, vit_depth=1, qf_layers=2, llm_layers=2):
    from stllm_amd import synth
    from stllm_amd.models import st_llm
    from stllm_amd.models.blip2 import Blip2Base
    from stllm_amd.tokenizer import IdTokenizer
    old = (Blip2Base.vit_depth, Blip2Base.qformer_layers, Blip2Base.init_tokenizer)
    Blip2Base.vit_depth, Blip2Base.qformer_layers = vit_depth, qf_layers
    Blip2Base.init_tokenizer = classmethod(lambda cls, truncation_side="right": IdTokenizer(0, 1, 2, 32000))
    try:
        m = st_llm.STLLMForCausalLM.from_config(dict(cfg, llama_model=dict(num_hidden_layers=llm_layers)), device="cpu")
    finally:
        Blip2Base.vit_depth, Blip2Base.qformer_layers, Blip2Base.init_tokenizer = old
    synth.fill_module_(m, 0, "")
    return m


@pytest.fixture(scope="module")
def stllm():
    m = _build(CFG)
    m.lm_head.weight.mul_(6.0)   # as test_generate_padded_batch_by_length_groups: spread the logits so that the rows take different paths
    return m


LENS = [9, 6, 9, 4]


def _padded(prompts, side):
    S = max(p.shape[0] for p in prompts)
    emb = torch.zeros(len(prompts), S, prompts[0].shape[1])
    mask = torch.zeros(len(prompts), S, dtype=torch.long)
    for i, p_ in enumerate(prompts):
        n = p_.shape[0]
        sl = slice(0, n) if side == "right" else slice(S - n, S)
        emb[i, sl] = p_
        mask[i, sl] = 1
    return emb, mask


# ---- 2. generate(batching="ragged") ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["right", "left"])
def test_generate_ragged_equals_every_prompt_alone_and_the_length_groups(stllm, side):
    """the lengths and seeds of test_generate_padded_batch_by_length_groups (9 / 6 / 9 / 4), fp32, 2 layers: ONE batched call on a ragged KV cache returns,
    row for row, the ids of each prompt generated alone — and what batching="groups" returns"""
    from stllm_amd import runtime
    model = stllm
    prompts = [T(f"gen.ragged{i}", (n, 4096), 0.05) for i, n in enumerate(LENS)]
    emb, mask = _padded(prompts, side)
    with CB.installed(), runtime.use_dtype("fp32"):
        for kw in (dict(num_beams=1), dict(num_beams=3, repetition_penalty=1.2)):
            k = dict(max_new_tokens=5, do_sample=False, min_length=1, **kw)
            alone = [model.generate(inputs_embeds=p_[None], **k)[0] for p_ in prompts]
            with CB.counting() as calls:
                got = model.generate(inputs_embeds=emb, attention_mask=mask, batching="ragged", **k)
                assert calls.count("kv_append_rows") > 0, "one batched decode loop on a ragged cache"
            groups = model.generate(inputs_embeds=emb, attention_mask=mask, **k)
            assert got.shape == (len(LENS), max(a.numel() for a in alone))
            for i, a in enumerate(alone):
                assert got[i, : a.numel()].tolist() == a.tolist(), (side, kw, i)
                assert (got[i, a.numel():] == 0).all()
            assert torch.equal(got, groups), (side, kw)
        # equal lengths under batching="ragged": the plain batched call (uniform cache)
        e2 = torch.stack([prompts[0], prompts[2]])
        with CB.counting() as calls:
            a = model.generate(inputs_embeds=e2, attention_mask=torch.ones(2, 9, dtype=torch.long), max_new_tokens=3, batching="ragged")
            assert calls.count("kv_append_rows") == 0
        assert torch.equal(a, model.generate(inputs_embeds=e2, max_new_tokens=3))
        with pytest.raises(ValueError, match="batching"):
            model.generate(inputs_embeds=e2, max_new_tokens=3, batching="paged")


# ---- 3. one shared prefix row, questions of different lengths --------------------------------------------------------------------------------------
def test_generate_ragged_behind_a_shared_prefix(stllm):
    from stllm_amd import runtime
    model = stllm
    video = T("gen.ragged_prefix", (1, 7, 4096), 0.05)
    qs = [T(f"gen.ragged_q{i}", (n, 4096), 0.05) for i, n in enumerate([5, 2, 4])]
    emb, mask = _padded(qs, "right")
    with CB.installed(), runtime.use_dtype("fp32"):
        prefix = model.model.new_cache(1, 7, "cpu")
        model.model.prefill(video, None, cache=prefix)
        before = [b.clone() for b in prefix.qkv]
        for kw in (dict(num_beams=1), dict(num_beams=3, repetition_penalty=1.2)):
            k = dict(max_new_tokens=5, do_sample=False, min_length=1, **kw)
            alone = [model.generate(inputs_embeds=q[None], prefix_cache=prefix, **k)[0] for q in qs]
            whole = [model.generate(inputs_embeds=torch.cat([video[0], q])[None], **k)[0] for q in qs]
            got = model.generate(inputs_embeds=emb, attention_mask=mask, prefix_cache=prefix, batching="ragged", **k)
            for i, a in enumerate(alone):
                assert a.tolist() == whole[i].tolist()
                assert got[i, : a.numel()].tolist() == a.tolist(), (kw, i)
                assert (got[i, a.numel():] == 0).all()
            assert prefix.len == 7 and prefix.lens is None and all(torch.equal(x, y) for x, y in zip(prefix.qkv, before))
        # equal-length questions behind the shared row, and one prefix row per prompt
        same = torch.stack([qs[0][:3], qs[2][:3]])
        got = model.generate(inputs_embeds=same, prefix_cache=prefix, batching="ragged", max_new_tokens=3)
        for i in range(2):
            assert got[i].tolist() == model.generate(inputs_embeds=same[i:i + 1], prefix_cache=prefix, max_new_tokens=3)[0].tolist()
        per_row = prefix.fork(rows=3)
        got = model.generate(inputs_embeds=emb, attention_mask=mask, prefix_cache=per_row, batching="ragged", max_new_tokens=4, min_length=1)
        want = model.generate(inputs_embeds=emb, attention_mask=mask, prefix_cache=prefix, batching="ragged", max_new_tokens=4, min_length=1)
        assert torch.equal(got, want)


# ---- 4. Chat.answer_many ---------------------------------------------------------------------------------------------------------------------------
def test_chat_answer_many_equals_answer_per_question(stllm):
    from stllm_amd import runtime
    from stllm_amd.conversation import Chat, StoppingCriteriaSub
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
            for pf in (None, prefix):
                got = chat.answer_many(img_list, questions, prefix=pf, **k)
                assert len(got) == len(questions)
                for (t0, i0), (t1, i1) in zip(want, got):
                    assert np.array_equal(i0, i1) and t0 == t1, (kw, pf is not None, i0, i1)
            assert all(torch.equal(x, y) for x, y in zip(prefix.cache.qkv, before))
        # a stop sequence that ends one row several steps before the others: the reference's criterion looks at row 0 only and would stop all of them
        free = [chat.answer(img_list, q, max_new_tokens=8, stopping_criteria=[])[1].tolist() for q in questions]
        pick = None
        for r, ids in enumerate(free):
            for t in range(1, 4):
                if all(ids[t] not in o[:t + 4] for j, o in enumerate(free) if j != r) and ids[t] not in ids[:t]:
                    pick = (r, t, ids[t])
                    break
            if pick:
                break
        assert pick is not None, ("no token separates the rows early enough", free)
        r, t, tok = pick
        stops = [torch.tensor([tok])]
        k = dict(max_new_tokens=8, num_beams=1)
        want = [chat.answer(img_list, q, stopping_criteria=[StoppingCriteriaSub(stops=stops)], **k) for q in questions]
        got = chat.answer_many(img_list, questions, stop_sequences=stops, prefix=prefix, **k)
        lengths = [len(i) for _, i in got]
        assert lengths[r] == t + 1 and max(lengths) >= lengths[r] + 3, (pick, lengths)
        for (t0, i0), (t1, i1) in zip(want, got):
            assert np.array_equal(i0, i1) and t0 == t1
        # the truncation rule of answer(): prompts longer than max_length - max_new_tokens keep their last embeddings (the uncached path)
        nv = img_list[0].shape[1]
        k = dict(max_new_tokens=4, max_length=nv + 2, num_beams=1)
        want = [chat.answer(img_list, q, **k) for q in questions]
        got = chat.answer_many(img_list, questions, prefix=prefix, **k)
        for (t0, i0), (t1, i1) in zip(want, got):
            assert np.array_equal(i0, i1)


# ---- 5. KVCache.lens; the uniform step is the step it was ------------------------------------------------------------------------------------------
def test_kv_cache_fork_and_truncate_with_lens():
    from stllm_amd.models.llama import KVCache
    c = KVCache(2, 3, 10, 8, torch.float32, "cpu")
    for i, b in enumerate(c.qkv):
        b.copy_(torch.arange(b.numel()).view_as(b).float() + 1000 * i)
    assert c.lens is None
    c.set_lens([6, 2, 4])
    assert c.len == 6 and c.lens == [6, 2, 4]
    f = c.fork(rows=6, max_len=12)
    assert f.lens == [6, 6, 2, 2, 4, 4] and f.len == 6 and f.batch == 6 and c.lens == [6, 2, 4]
    for src, dst in zip(c.qkv, f.qkv):
        assert torch.equal(dst[:, :6], src[:, :6].repeat_interleave(2, dim=0))
    f.truncate(3)
    assert f.lens == [3, 3, 2, 2, 3, 3] and f.len == 3
    f.truncate([1, 3, 0, 2, 3, 3])
    assert f.lens == [1, 3, 0, 2, 3, 3] and f.len == 3
    with pytest.raises(AssertionError):
        f.truncate([2, 3, 0, 2, 3, 3])       # row 0 holds 1 position
    f.truncate(2)
    assert f.lens == [1, 2, 0, 2, 2, 2] and f.len == 2
    f.truncate(0)
    assert f.lens is None and f.len == 0, "equal lengths: a uniform cache again"
    u = KVCache(1, 2, 10, 8, torch.float32, "cpu")
    u.len = 5
    u.truncate([5, 3])
    assert u.lens == [5, 3] and u.len == 5
    assert u.fork().lens == [5, 3]


UNIFORM_LAYER = ["rmsnorm", "gemm", "attention", "gemm", "rmsnorm", "gemm", "gemm"]   # B = 3 > FUSE_NORM_ROWS (and fp32 never fuses): the parent's launches


def test_uniform_step_is_unchanged_and_ragged_step_adds_the_append():
    """lens = None: exactly the backend calls of the step before this feature.  lens set: the same plus one kv_append_rows per layer and the two RoPE-row
    gathers of the step.  A ragged cache whose rows have one length gives the uniform step's logits bit for bit; different lengths give, per row, the
    logits of that row decoded alone."""
    from stllm_amd import runtime
    model = small_llama(SMALL)
    lm = model.model
    emb = T("ragged.emb", (3, 12, 256), 0.05)
    lens = [8, 5, 3]
    with CB.installed(), runtime.use_dtype("fp32"):
        c = lm.new_cache(3, 16, "cpu")
        lm.prefill(emb[:, :8], None, cache=c)
        r = c.fork()
        r.lens = [8, 8, 8]                     # ragged code path, equal lengths
        with CB.counting() as calls:
            _, h_u = lm.decode_step(emb[:, 8:9], c)
            assert calls == UNIFORM_LAYER * 2 + ["rmsnorm"], calls
        with CB.counting() as calls:
            _, h_r = lm.decode_step(emb[:, 8:9], r)
            want = ["gather_rows", "gather_rows"] + (UNIFORM_LAYER[:2] + ["kv_append_rows"] + UNIFORM_LAYER[2:]) * 2 + ["rmsnorm"]
            assert calls == want, calls
        assert torch.equal(h_u, h_r) and r.lens == [9, 9, 9] and r.len == 9 and c.len == 9 and c.lens is None
        for x, y in zip(c.qkv, r.qkv):
            assert torch.equal(x[:, :9, 256:], y[:, :9, 256:])
        # different lengths: ragged prefill (right-padded mask), then 3 steps; every row against itself alone
        mask = (torch.arange(8)[None, :] < torch.tensor(lens)[:, None]).long()
        rg = lm.new_cache(3, 16, "cpu")
        _, h16 = lm.prefill(emb[:, :8], mask, cache=rg)
        assert rg.lens == lens and rg.len == 8
        alone = []
        for b, n in enumerate(lens):
            cb = lm.new_cache(1, 16, "cpu")
            _, hb = lm.prefill(emb[b:b + 1, :n], None, cache=cb)
            assert torch.allclose(h16.view(3, 8, -1)[b, :n], hb, atol=1e-5)
            alone.append(cb)
        for t in range(3):
            tok = emb[:, 9 + t:10 + t]
            _, h = lm.decode_step(tok, rg)
            for b in range(3):
                _, hb = lm.decode_step(tok[b:b + 1], alone[b])
                assert torch.allclose(h[b], hb[0], atol=1e-5), (t, b)
        assert rg.lens == [n + 3 for n in lens] and rg.len == 11
        with pytest.raises(NotImplementedError, match="ragged prefix"):
            lm.extend(emb[:, :2], rg)


@pytest.mark.parametrize("mode", ["int8", "lora"])
def test_ragged_step_under_int8_weights_and_lora_shares_the_attention_half(mode):
    """bf16 contract backend: a ragged cache with equal lengths == the uniform step, bit for bit, under runtime.use_decode_weights("int8") and with active
    adapters; with different lengths every row equals itself alone (one code path for the attention half: LlamaModel.decode_attn)"""
    import contextlib
    from stllm_amd import runtime
    model = small_llama(SMALL, r=8 if mode == "lora" else 0)
    lm = model.model
    emb = T("ragged.emb", (2, 12, 256), 0.05)
    ctx = runtime.use_decode_weights("int8") if mode == "int8" else contextlib.nullcontext()
    with CB.installed(), runtime.use_dtype("bf16"), ctx:
        c = lm.new_cache(2, 16, "cpu")
        lm.prefill(emb[:, :8], None, cache=c)
        r = c.fork()
        r.lens = [8, 8]
        with CB.counting() as calls:
            _, h_u = lm.decode_step(emb[:, 8:9], c)
            n_u = len(calls)
            assert ("gemv_w8" in calls) == (mode == "int8") and ("lora_down" in calls) == (mode == "lora")
        with CB.counting() as calls:
            _, h_r = lm.decode_step(emb[:, 8:9], r)
            assert len(calls) == n_u + 2 + 2 and calls.count("kv_append_rows") == 2
        assert torch.equal(h_u, h_r)
        mask = torch.tensor([[1] * 8, [1] * 5 + [0] * 3])
        rg = lm.new_cache(2, 16, "cpu")
        lm.prefill(emb[:, :8], mask, cache=rg)
        cb = lm.new_cache(1, 16, "cpu")
        lm.prefill(emb[1:2, :5], None, cache=cb)
        for t in range(2):
            _, h = lm.decode_step(emb[:, 9 + t:10 + t], rg)
            _, hb = lm.decode_step(emb[1:2, 9 + t:10 + t], cb)
            scale = float(hb.float().abs().max())
            assert float((h[1].float() - hb[0].float()).abs().max()) <= 2.0 ** -7 * scale   # one bf16 rounding step of the hidden row (B = 2 vs B = 1 contract calls)


# ---- 6. ABI ----------------------------------------------------------------------------------------------------------------------------------------
def test_abi_declares_and_exports_the_ragged_entry_points():
    from stllm_amd import hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "stllm_hip.h")).read()
    for name in ("stllm_attention_decode_ragged", "stllm_attention_decode_ragged_workspace_bytes", "stllm_kv_append_rows"):
        assert name in hip.EXPORTS
        assert re.search(r"\b" + name + r"\(", header), name
    # the header's argument lists and the ctypes bindings agree in length
    import ctypes

    class _L:
        pass
    fake = _L()
    for n in hip.EXPORTS:
        setattr(fake, n, _L())
    hip._bind(fake)
    for name in ("stllm_attention_decode_ragged", "stllm_kv_append_rows", "stllm_attention_decode_ragged_workspace_bytes"):
        decl = re.search(r"^int(?:64_t)? " + name + r"\(([^;]*?)\);", header, re.S | re.M).group(1)
        assert len(getattr(fake, name).argtypes) == len(decl.split(",")), name
    assert fake.stllm_attention_decode_ragged_workspace_bytes.restype is ctypes.c_int64
    if os.path.exists(hip.LIB_PATH):
        L = hip.lib()
        assert L.stllm_abi_version() == 7
        assert all(hasattr(L, n) for n in hip.EXPORTS)
        assert L.stllm_attention_decode_ragged_workspace_bytes(4, 32, 1100) == L.stllm_attention_decode_workspace_bytes(4, 32, 1100) > 0
        assert L.stllm_attention_decode_ragged_workspace_bytes(4, 32, 0) == -1
