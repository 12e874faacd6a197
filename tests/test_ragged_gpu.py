"""GPU: the ragged KV cache on the device — stllm_attention_decode_ragged / stllm_kv_append_rows against fp64 and against the uniform decode kernels,
ragged decode_step against the uniform step and against every row decoded alone (full width), generate(batching="ragged") in fp32, the int8-weight and
LoRA steps, and the launch count of a ragged step."""
import numpy as np
import pytest
import torch

import _poison
from _util import T
from test_kernels_gpu import OUT_TOL, check

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
D = 128


@pytest.fixture(scope="module")
def hip():
    from stllm_amd import hip as h
    h.lib()
    return h


def _model(layers=3, r=0):
    from stllm_amd import synth
    from stllm_amd.models.st_llm import STLLMForCausalLM, StllmConfig
    m = STLLMForCausalLM(StllmConfig(num_hidden_layers=layers), device="cuda")
    synth.fill_module_(m, 0, "")
    if r:
        m.add_lora(r, 32)
        for i, mod in enumerate(m._lora_modules()):
            mod.B.copy_(T(f"ragged.B{i}", tuple(mod.B.shape), 0.02).cuda())
    return m


def _lens(B):
    """B - 1 lengths drawn from a fixed seed in [1, 2048] plus one row of length 0 (a free slot); B = 1: one drawn length"""
    rs = np.random.RandomState(1234 + B)
    lens = [int(x) for x in rs.randint(1, 2049, size=max(B - 1, 1))]
    return lens + [0] if B > 1 else lens


# ---- 1. the attention kernels ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("single", [1, 0])
@pytest.mark.parametrize("B", [1, 5, 16])
def test_attention_decode_ragged(hip, dtype, B, single):
    """H = 32, per-row lengths in [1, 2048] + a zero-length row.  Every row vs fp64 with the bound of test_attention_decode_split_kv (2 x OUT_TOL); per row
    bit-identical to stllm_attention_decode on that row alone (Skv = its length) whenever both calls take the same schedule.  single = 0 forces the
    split-KV pair through the "attn_decode_single" option."""
    H = 32
    lens = _lens(B)
    if single == 1 and B == 5:
        lens = [min(n, 1536) for n in lens]                  # one case where the host takes the single-pass kernel for the whole ragged batch
    max_kv = max(lens)
    ML = max_kv + 5
    td = hip.torch_dtype(dtype)
    cache = T("ragged.kvcache", (B, ML, 3 * H * D), 1.0).to(td).cuda()
    q = T("ragged.q", (B, 3 * H * D), 1.0).to(td).cuda()
    for b, n in enumerate(lens):
        cache[b, n:] = float("nan")                          # the rows at or behind a row's length are uninitialised memory: never read
        if n == 0:
            q[b] = float("nan")                              # ... and so is the query of a free slot
    kv_len = torch.tensor(lens, dtype=torch.int32).cuda()
    full = cache.view(B * ML, 3 * H * D)
    ks = (ML * 3 * H * D, 3 * H * D)
    ragged_single = single == 1 and (max_kv <= 1536 or B * H >= 256)
    hip.set_option("attn_decode_single", single)
    try:
        g = _poison.Guarded(B, H * D, td, device="cuda")     # the output starts as 0xFF (NaN) inside a 0xFF-filled buffer: a free slot must still read zeros
        with _poison.poisoned_allocations() as counts:       # the partial-state workspace: 0xFF in every byte (a merge that read an unwritten record would see it)
            got = hip.attention(q[:, :H * D], full[:, H * D:2 * H * D], full[:, 2 * H * D:], B=B, H=H, Sq=1, Skv=max_kv, D=D, scale=D ** -0.5, kv_len=kv_len,
                                q_strides=(3 * H * D, 3 * H * D), k_strides=ks, v_strides=ks, out=g.out)
        torch.cuda.synchronize()
        assert counts.allocations > 0 and g.intact(), "a byte outside the output rows was written"
        n_same = 0
        for b, n in enumerate(lens):
            if n == 0:
                assert float(got[b].float().abs().max()) == 0.0, "a free slot writes zeros"
                continue
            c = cache[b].double().cpu().view(ML, 3, H, D)
            k, v = c[:n, 1].transpose(0, 1), c[:n, 2].transpose(0, 1)
            qb = q[b].double().cpu().view(3, H, D)[0]
            ref = (torch.softmax((qb.unsqueeze(1) @ k.transpose(-1, -2)) * D ** -0.5, dim=-1) @ v).reshape(1, H * D)
            check(got[b:b + 1], ref, 2 * OUT_TOL[dtype], f"ragged decode attention row {b} (len {n}) vs fp64")
            alone_single = single == 1 and (n <= 1536 or H >= 256)
            if alone_single == ragged_single:
                alone = hip.attention(q[b:b + 1, :H * D], cache[b][:, H * D:2 * H * D], cache[b][:, 2 * H * D:], B=1, H=H, Sq=1, Skv=n, D=D,
                                      scale=D ** -0.5, q_strides=(3 * H * D, 3 * H * D), k_strides=ks, v_strides=ks)
                assert torch.equal(got[b], alone[0]), f"row {b} (len {n}): not bit-identical to the uniform kernel on the row alone"
                n_same += 1
        assert n_same > 0
    finally:
        hip.set_option("attn_decode_single", 1)


# ---- 2. the append ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("with_q", [False, True])
def test_kv_append_rows(hip, dtype, with_q):
    td = hip.torch_dtype(dtype)
    B, ML, hidden = 5, 40, 4096
    cache = T("ragged.append_cache", (B, ML, 3 * hidden), 1.0).to(td).cuda()
    src = T("ragged.append_src", (B, 3 * hidden), 1.0).to(td).cuda()
    pos_h = [0, 39, 17, -1, 40]                              # rows 3 and 4: free slots
    want = cache.clone()
    c0 = 0 if with_q else hidden
    for b, p in enumerate(pos_h):
        if 0 <= p < ML:
            want[b, p, c0:] = src[b, c0:]
    hip.kv_append_rows(src, cache, torch.tensor(pos_h, dtype=torch.int32).cuda(), with_q=with_q)
    assert torch.equal(cache, want), "exact, and every other cache row unchanged"


# ---- 3. decode equivalence at full width -----------------------------------------------------------------------------------------------------------
def _prefill_rows(lm, emb, lens, n_new):
    """a ragged cache filled by ONE prefill of the right-padded rows"""
    B, S = len(lens), max(lens)
    mask = (torch.arange(S)[None, :] < torch.tensor(lens)[:, None]).long()
    c = lm.new_cache(B, S + n_new + 1, "cuda")
    lm.prefill(emb[:, :S], mask, cache=c)
    return c


def _steps(model, cache, toks):
    out = []
    for t in range(toks.shape[1]):
        _, h16 = model.model.decode_step(toks[:, t:t + 1], cache)
        out.append(model.logits_from(h16, toks.shape[0], 1)[:, 0].float().clone())
    return out


def test_ragged_decode_matches_uniform_and_every_row_alone(hip):
    """3 layers, D = 4096, bf16.
    (a) a ragged cache whose rows all have one length: logits bit-identical to the uniform decode_step (same GEMV launches; the ragged attention kernels
        are bit-identical per row; the appended K / V rows are the bytes the GEMV would have written in place).
    (b) lengths [97, 40, 97, 13], 6 steps: every row's logits within a bound of the same row decoded alone.  The bound is MEASURED here, not guessed:
        yardstick = the uniform path's own batched-vs-alone logit difference (4 equal-length rows of 97 in one batch against each row alone, same model,
        same 6 tokens: different GEMV kernels for 4 rows and 1 row, same math); the ragged batch adds a second source of reordering (the prefill of a
        padded batch against an unpadded one), so 2 x yardstick is allowed.  The yardstick is computed at run time from the uniform path (never from the ragged path) and printed with the ragged
        figure (pytest -s); neither figure has been recorded yet (profiles/ragged_decode.md: NOT measured yet).
    (c) fp32 mode: the ids (argmax of the logits) of every step equal the row's alone."""
    from stllm_amd import runtime
    model = _model(3)
    lm = model.model
    lens, n_new = [97, 40, 97, 13], 6
    emb = T("ragged.prompt", (4, 97, 4096), 0.05).cuda()
    toks = lm.embed_tokens(torch.tensor([[5, 9, 1234, 77, 31000, 8], [31000, 8, 4, 2, 17, 900], [12, 13, 14, 15, 16, 17], [3000, 1, 7, 29999, 5, 6]])).cuda()
    with runtime.use_dtype("bf16"):
        # (a)
        cu = lm.new_cache(4, 97 + n_new + 1, "cuda")
        lm.prefill(emb, None, cache=cu)
        cr = cu.fork()
        cr.lens = [97] * 4
        uni, rag = _steps(model, cu, toks), _steps(model, cr, toks)
        assert all(torch.equal(a, b) for a, b in zip(uni, rag)), "equal lengths: the ragged step must be the uniform step, bit for bit"
        assert cr.lens == [97 + n_new] * 4 and cu.lens is None
        # yardstick: uniform batched vs alone, equal lengths
        yard = 0.0
        for b in range(4):
            cb = lm.new_cache(1, 97 + n_new + 1, "cuda")
            lm.prefill(emb[b:b + 1], None, cache=cb)
            for t, lg in enumerate(_steps(model, cb, toks[b:b + 1])):
                yard = max(yard, float((uni[t][b] - lg[0]).abs().max()))
        # (b)
        rc = _prefill_rows(lm, emb, lens, n_new)
        assert rc.lens == lens
        got = _steps(model, rc, toks)
        worst = 0.0
        for b, n in enumerate(lens):
            cb = lm.new_cache(1, n + n_new + 1, "cuda")
            lm.prefill(emb[b:b + 1, :n], None, cache=cb)
            for t, lg in enumerate(_steps(model, cb, toks[b:b + 1])):
                worst = max(worst, float((got[t][b] - lg[0]).abs().max()))
        scale = float(torch.stack(uni).abs().max())
        print(f"ragged decode bf16: batched-vs-alone yardstick (uniform path) {yard:.4e}, ragged-vs-alone {worst:.4e}, logits abs-max {scale:.3f}")
        assert yard > 0 and worst <= 2 * yard, f"ragged vs alone {worst:.4e} > 2 x yardstick {yard:.4e}"
    with runtime.use_dtype("fp32"):
        rc = _prefill_rows(lm, emb, lens, n_new)
        got = _steps(model, rc, toks)
        for b, n in enumerate(lens):
            cb = lm.new_cache(1, n + n_new + 1, "cuda")
            lm.prefill(emb[b:b + 1, :n], None, cache=cb)
            for t, lg in enumerate(_steps(model, cb, toks[b:b + 1])):
                assert int(got[t][b].argmax()) == int(lg[0].argmax()), (b, t)
                assert float((got[t][b] - lg[0]).abs().max()) <= 2e-4 * float(lg.abs().max()), (b, t)   # the fp32 bound of test_kv_cache_decode_matches_reprefill


# ---- 4. generate(batching="ragged") on the device --------------------------------------------------------------------------------------------------
def test_generate_ragged_on_device():
    """mirrors test_generate_padded_batch_on_device (fp32, left-padded 9 / 6 / 9 / 4, greedy and 3 beams): one batched call on a ragged cache returns every
    row's ids as its unpadded prompt generates alone, and what batching="groups" returns"""
    from stllm_amd import runtime
    from test_model_gpu import build_stllm
    cfg = dict(vit_model="eva_clip_g", image_size=224, num_query_token=32, video_input="mean", use_mask=False, mvm_decode=False,
               qformer_text_input=False, max_txt_len=32, end_sym=" 2")
    model = build_stllm(cfg, vit_depth=1, qf_layers=2, llm_layers=2)
    model.lm_head.weight.mul_(6.0)
    lens = [9, 6, 9, 4]
    prompts = [T(f"gen.ragged{i}", (n, 4096), 0.05).cuda() for i, n in enumerate(lens)]
    S = max(lens)
    emb = torch.zeros(len(lens), S, 4096, device="cuda")
    mask = torch.zeros(len(lens), S, dtype=torch.long)
    for i, (p_, n) in enumerate(zip(prompts, lens)):
        emb[i, S - n:] = p_
        mask[i, S - n:] = 1
    with runtime.use_dtype("fp32"):
        for kw in (dict(num_beams=1), dict(num_beams=3, repetition_penalty=1.2)):
            k = dict(max_new_tokens=5, do_sample=False, min_length=1, **kw)
            alone = [model.generate(inputs_embeds=p_[None], **k)[0] for p_ in prompts]
            got = model.generate(inputs_embeds=emb, attention_mask=mask.cuda(), batching="ragged", **k)
            groups = model.generate(inputs_embeds=emb, attention_mask=mask.cuda(), **k)
            for i, a in enumerate(alone):
                assert got[i, : a.numel()].tolist() == a.tolist(), (kw, i)
                assert (got[i, a.numel():] == 0).all()
            assert torch.equal(got, groups), kw
        # three questions of different lengths behind ONE shared prefix row
        prefix = model.model.new_cache(1, 9, "cuda")
        model.model.prefill(prompts[0][None], None, cache=prefix)
        qs = [prompts[1][:5], prompts[2][:2], prompts[3][:4]]
        qe = torch.zeros(3, 5, 4096, device="cuda")
        qm = torch.zeros(3, 5, dtype=torch.long)
        for i, q in enumerate(qs):
            qe[i, :q.shape[0]] = q
            qm[i, :q.shape[0]] = 1
        k = dict(max_new_tokens=5, do_sample=False, min_length=1)
        got = model.generate(inputs_embeds=qe, attention_mask=qm, prefix_cache=prefix, batching="ragged", **k)
        for i, q in enumerate(qs):
            a = model.generate(inputs_embeds=q[None], prefix_cache=prefix, **k)[0]
            assert got[i, : a.numel()].tolist() == a.tolist(), i
        assert prefix.len == 9 and prefix.lens is None


# ---- 5. int8 weights / LoRA ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["int8", "lora"])
def test_ragged_step_under_int8_and_lora_is_the_uniform_step_on_equal_lengths(hip, mode):
    import contextlib
    from stllm_amd import runtime
    model = _model(2, r=16 if mode == "lora" else 0)
    lm = model.model
    emb = T("ragged.prompt", (2, 40, 4096), 0.05).cuda()
    toks = lm.embed_tokens(torch.tensor([[5, 9, 1234], [31000, 8, 4]])).cuda()
    ctx = runtime.use_decode_weights("int8") if mode == "int8" else contextlib.nullcontext()
    seen = []
    orig = hip.gemv_w8

    def spy(*a, **k):
        seen.append(1)
        return orig(*a, **k)
    hip.gemv_w8 = spy
    try:
        with runtime.use_dtype("bf16"), ctx:
            cu = lm.new_cache(2, 48, "cuda")
            lm.prefill(emb, None, cache=cu)
            cr = cu.fork()
            cr.lens = [40, 40]
            uni, rag = _steps(model, cu, toks), _steps(model, cr, toks)
            assert "lora_A" in lm.pack()[0] if mode == "lora" else len(seen) == 2 * 3 * 2 * 4
    finally:
        hip.gemv_w8 = orig
    assert all(torch.equal(a, b) for a, b in zip(uni, rag)), mode


# ---- 6. launches per layer -------------------------------------------------------------------------------------------------------------------------
ENTRY_POINTS = ["gemm", "gemv_w8", "rmsnorm", "attention", "kv_append_rows", "gather_rows", "lora_down"]


def _count(hip, fn):
    """names of the hip entry points fn() calls (a counting wrapper, as tests/test_w8_gpu.py wraps gemv_w8) and the kernels they launched"""
    calls = []
    saved = {n: getattr(hip, n) for n in ENTRY_POINTS}

    def wrap(name, f):
        def g(*a, **k):
            r = f(*a, **k)
            calls.append((name, hip.lib().stllm_last_kernel().decode()))
            return r
        return g
    try:
        for n, f in saved.items():
            setattr(hip, n, wrap(n, f))
        fn()
    finally:
        for n, f in saved.items():
            setattr(hip, n, f)
    return calls


def test_ragged_step_launch_count(hip):
    """a ragged step = the uniform step's entry-point calls + 1 per LAYER (the append) + 2 per STEP (the gathers of the cos / sin table rows).  What is
    counted are calls of the hip entry points through a wrapper, not kernel launches; in this regime each call is one launch (B = 4 rows, Skv <= 1536:
    GEMV kernels, the single-pass attention kernel).  The uniform step's calls are those it always made: 7 per layer at B = 4 (no fused
    norm above 2 rows), 5 per layer at B = 2."""
    from stllm_amd import runtime
    model = _model(2)
    lm = model.model
    emb = T("ragged.prompt", (4, 40, 4096), 0.05).cuda()
    tok = lm.embed_tokens(torch.tensor([[5], [9], [1234], [77]])).cuda()
    with runtime.use_dtype("bf16"):
        for B, per_layer in ((4, 7), (2, 5)):
            cu = lm.new_cache(B, 48, "cuda")
            lm.prefill(emb[:B], None, cache=cu)
            cr = _prefill_rows(lm, emb[:B], [40, 13, 40, 22][:B], 4)
            uni = _count(hip, lambda: lm.decode_step(tok[:B], cu))
            rag = _count(hip, lambda: lm.decode_step(tok[:B], cr))
            names_u, names_r = [n for n, _ in uni], [n for n, _ in rag]
            assert len(uni) == 2 * per_layer + 1 and "kv_append_rows" not in names_u and "gather_rows" not in names_u, names_u
            assert names_r.count("kv_append_rows") == 2 and names_r.count("gather_rows") == 2, names_r
            layer_r = [n for n in names_r if n != "gather_rows"]
            assert len(layer_r) == len(uni) + 2, (names_u, names_r)
            assert [n for n in layer_r if n != "kv_append_rows"] == names_u
            kern = [k for n, k in rag if n == "attention"]
            print(f"ragged step B={B}: {len(layer_r) - 1} calls in 2 layers (uniform {len(uni) - 1}); attention kernel {kern[0]}")
