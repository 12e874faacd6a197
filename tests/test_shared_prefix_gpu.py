"""GPU: the shared-prefix KV cache on the device — stllm_attention_shared against fp64 (decode and extend shapes, bf16 / fp16 / fp32,
NaN behind every bound), decode steps / generate on a cache with a shared base against forked copies at full width, the int8-weight and LoRA steps,
the launches of a shared step and the memory a share() allocates."""
import contextlib

import pytest
import torch

import _shared_case as SC
from _util import T
from test_kernels_gpu import OUT_TOL, check
from test_ragged_gpu import _model, _steps

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
H = 32
TD = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


@pytest.fixture(scope="module")
def hip():
    from stllm_amd import hip as h
    h.lib()
    return h


def _check_rows(got, want, live, tol, what):
    got = got.detach().double().cpu()
    assert torch.isfinite(got[live]).all(), f"{what}: non-finite output (something behind a bound was read)"
    scale = max(float(want.abs().max()), 1e-6)
    err = float((got[live] - want[live]).abs().max())
    print(f"{what}: err {err:.3e} / abs-max {scale:.3e} (bound {tol * scale:.3e})")
    assert err <= tol * scale, f"{what}: max err {err:.3e} > {tol:.1e} * {scale:.3e}"


# ---- A. decode -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("P", [7, 33, 577, 2048])
@pytest.mark.parametrize("G,R", [(1, 1), (1, 5), (1, 16), (2, 3), (1, 17), (1, 33)])
def test_attention_shared_decode(hip, dtype, G, R, P):
    """H = 32; suffix lengths from a fixed seed in [1, 300] plus one row of length 1; prefix and suffix buffers of different max_len; NaN behind P and
    behind every sfx_len[b].  Every row within 2 x OUT_TOL of the fp64 softmax over its concatenated live keys (the bound of
    test_attention_decode_split_kv / test_attention_decode_ragged), finite, bit-identical between two calls, prefix buffers unchanged."""
    sfx = SC.draw_lens(G * R, R + P)
    pre, suf, q = SC.make(TD[dtype], G, R, H, P, sfx, device="cuda")
    keep = pre.clone()
    got = SC.call(hip, pre, suf, q, G, R, H, P, sfx)
    again = SC.call(hip, pre, suf, q, G, R, H, P, sfx)
    torch.cuda.synchronize()
    want, _ = SC.reference(pre, suf, q, G, R, H, P, sfx)
    _check_rows(got, want, torch.ones(G * R, dtype=torch.bool), 2 * OUT_TOL[dtype], f"shared decode {dtype} G={G} R={R} P={P}")
    assert torch.equal(got, again), "two calls, identical bits"
    assert torch.equal(torch.nan_to_num(pre.float()), torch.nan_to_num(keep.float())), "the prefix buffers are read-only"


# ---- B. extend -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("P", [33, 577])
@pytest.mark.parametrize("G,R", [(1, 4), (2, 2)])
@pytest.mark.parametrize("Sq,q_off,ragged", [(1, 0, False), (8, 0, False), (40, 0, False), (1, 5, False), (8, 5, False), (40, 5, False), (8, 0, True), (40, 0, True)])
def test_attention_shared_extend(hip, dtype, G, R, P, Sq, q_off, ragged):
    """causal, Sq query rows at the suffix positions q_off .. q_off + Sq - 1; ragged: per-row suffix lengths <= Sq with q_off = 0 (query rows at or behind
    a row's length are don't-care).  Same fp64 check and bound as the decode shape."""
    B = G * R
    sfx = [max(1, Sq - 3 * b) for b in range(B)] if ragged else [q_off + Sq] * B
    pre, suf, q = SC.make(TD[dtype], G, R, H, P, sfx, Sq=Sq, device="cuda")
    got = SC.call(hip, pre, suf, q, G, R, H, P, sfx, Sq=Sq, causal=True, q_off=q_off, ragged=ragged)
    torch.cuda.synchronize()
    want, live = SC.reference(pre, suf, q, G, R, H, P, sfx, Sq=Sq, causal=True, q_off=q_off)
    _check_rows(got, want, live.reshape(-1), 2 * OUT_TOL[dtype], f"shared extend {dtype} G={G} R={R} P={P} Sq={Sq} q_off={q_off} ragged={ragged}")


# ---- C. fp32 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,R,P,Sq,q_off", [(1, 5, 33, 1, 0), (2, 3, 577, 1, 0), (1, 17, 7, 1, 0), (2, 2, 33, 8, 5), (1, 4, 577, 40, 0)])
def test_attention_shared_fp32(hip, G, R, P, Sq, q_off):
    B = G * R
    sfx = SC.draw_lens(B, R + P) if Sq == 1 else [max(1, Sq - 3 * b) for b in range(B)] if q_off == 0 else [q_off + Sq] * B
    pre, suf, q = SC.make(torch.float32, G, R, H, P, sfx, Sq=Sq, device="cuda")
    got = SC.call(hip, pre, suf, q, G, R, H, P, sfx, Sq=Sq, causal=Sq > 1, q_off=q_off)
    torch.cuda.synchronize()
    want, live = SC.reference(pre, suf, q, G, R, H, P, sfx, Sq=Sq, causal=Sq > 1, q_off=q_off)
    _check_rows(got, want, live.reshape(-1), OUT_TOL["fp32"], f"shared fp32 G={G} R={R} P={P} Sq={Sq} q_off={q_off}")


# ---- D / F. the model at full width ----------------------------------------------------------------------------------------------------------------
P_, QLENS, NEW = 97, [40, 13, 40, 7], 6
TOKS = [[5, 9, 1234, 77, 31000, 8], [31000, 8, 4, 2, 17, 900], [12, 13, 14, 15, 16, 17], [3000, 1, 7, 29999, 5, 6]]


def _copy_vs_shared(model, hip):
    """(yardstick, worst): yardstick = the COPY path's own batched-vs-each-row-alone logit difference (forked private copies: 4 rows in one ragged batch
    against each row alone, same model and tokens), computed from the copy path only; worst = shared path vs copy path, same batch."""
    lm = model.model
    video = T("shared.video", (1, P_, 4096), 0.05).cuda()
    qemb = T("shared.questions", (4, max(QLENS), 4096), 0.05).cuda()
    toks = lm.embed_tokens(torch.tensor(TOKS)).cuda()
    base = lm.new_cache(1, P_, "cuda")
    lm.prefill(video, None, cache=base)
    keep = [b.clone() for b in base.qkv]
    S = max(QLENS)
    f = base.fork(rows=4, max_len=P_ + S + NEW)
    lm.extend(qemb, f, lengths=QLENS)
    copy = _steps(model, f, toks)
    yard = 0.0
    for b, n in enumerate(QLENS):
        fb = base.fork(max_len=P_ + n + NEW)
        lm.extend(qemb[b:b + 1, :n], fb)
        for t, lg in enumerate(_steps(model, fb, toks[b:b + 1])):
            yard = max(yard, float((copy[t][b] - lg[0]).abs().max()))
    s = base.share(rows=4, max_new=S + NEW)
    lm.extend(qemb, s, lengths=QLENS)
    shared = _steps(model, s, toks)
    worst = max(float((a - b).abs().max()) for a, b in zip(shared, copy))
    assert all(torch.equal(x, y) for x, y in zip(base.qkv, keep)), "the base is never written"
    return yard, worst, float(torch.stack(copy).abs().max())


def test_shared_decode_matches_forked_copies(hip):
    """3 layers, D = 4096, bf16, P = 97, one base row, 4 questions [40, 13, 40, 7], 6 steps: shared-path logits within 2 x yardstick of the copy path
    (fork).  The yardstick is measured here from the copy path alone (its batched-vs-alone difference); 2 x because sharing adds one more summation
    re-ordering — the two-segment merge — on top of the batch's."""
    from stllm_amd import runtime
    model = _model(3)
    with runtime.use_dtype("bf16"):
        yard, worst, scale = _copy_vs_shared(model, hip)
    print(f"shared decode bf16: copy-path batched-vs-alone yardstick {yard:.4e}, shared-vs-copy {worst:.4e}, logits abs-max {scale:.3f}")
    assert yard > 0 and worst <= 2 * yard, f"shared vs copy {worst:.4e} > 2 x yardstick {yard:.4e}"


@pytest.mark.parametrize("mode", ["int8", "lora"])
def test_shared_step_under_int8_and_lora(hip, mode):
    """the int8-weight step and the LoRA step (r = 8) on a shared cache against the same steps on forked copies: the bound of the test above"""
    from stllm_amd import runtime
    model = _model(3, r=8 if mode == "lora" else 0)
    seen = []
    orig = hip.gemv_w8

    def spy(*a, **k):
        seen.append(1)
        return orig(*a, **k)
    hip.gemv_w8 = spy
    try:
        with runtime.use_dtype("bf16"), (runtime.use_decode_weights("int8") if mode == "int8" else contextlib.nullcontext()):
            yard, worst, scale = _copy_vs_shared(model, hip)
            assert "lora_A" in model.model.pack()[0] if mode == "lora" else len(seen) > 0
    finally:
        hip.gemv_w8 = orig
    print(f"shared decode bf16 {mode}: yardstick {yard:.4e}, shared-vs-copy {worst:.4e}, logits abs-max {scale:.3f}")
    assert yard > 0 and worst <= 2 * yard, f"{mode}: shared vs copy {worst:.4e} > 2 x yardstick {yard:.4e}"


# ---- E. generate in fp32 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beams", [1, 5])
def test_generate_share_prefix_same_ids_fp32(hip, beams):
    """the same 3-layer model in fp32: generate(share_prefix=True) returns the ids of share_prefix=False over 8 new tokens (greedy: behind a prefix cache;
    5 beams: the prompt's own cache is the base).  Guard: on the copy path the top-2 logit margin of every compared step exceeds 100 x the largest
    shared-vs-copy logit difference observed on the same steps."""
    from stllm_amd import generation, runtime
    model = _model(3)
    model.lm_head.weight.mul_(6.0)
    lm = model.model
    video = T("shared.video", (1, P_, 4096), 0.05).cuda()
    quest = T("shared.questions", (4, max(QLENS), 4096), 0.05).cuda()[:1, :13]
    logs = {False: [], True: []}
    orig = generation._CacheStepper.advance

    with runtime.use_dtype("fp32"):
        kw = dict(max_new_tokens=8, do_sample=False, min_length=8, num_beams=beams)
        if beams == 1:
            prefix = lm.new_cache(1, P_, "cuda")
            lm.prefill(video, None, cache=prefix)
            kw.update(inputs_embeds=quest, prefix_cache=prefix)
        else:
            kw.update(inputs_embeds=torch.cat([video, quest], dim=1))
        out = {}
        for share in (False, True):
            def spy(self, *a, _s=share, **k):
                r = orig(self, *a, **k)
                logs[_s].append(self.logits.clone())
                return r
            generation._CacheStepper.advance = spy
            try:
                out[share] = model.generate(share_prefix=share, **kw)
            finally:
                generation._CacheStepper.advance = orig
    assert len(logs[False]) == len(logs[True]) == 7
    diff = max(float((a - b).abs().max()) for a, b in zip(logs[True], logs[False]))
    top2 = [lg.topk(2, dim=-1).values for lg in logs[False]]
    margin = min(float((t[:, 0] - t[:, 1]).min()) for t in top2)
    print(f"generate fp32 beams={beams}: shared-vs-copy logit diff {diff:.3e}, smallest top-2 margin on the copy path {margin:.3e}")
    assert margin > 100 * diff, "the guard: choose other prompt ids"
    assert out[True].shape == out[False].shape and torch.equal(out[True], out[False])


# ---- G. launches -----------------------------------------------------------------------------------------------------------------------------------
def test_shared_step_launch_count(hip):
    """a shared step: per layer the uniform step's entry points with `attention` replaced by kv_append_rows + attention_shared, the latter being TWO
    launches — the family stllm_last_kernel reports as 'attn_shared_decode_kernel' is the partial pass + the merge, nothing else (launch_shared)"""
    from stllm_amd import runtime
    from test_ragged_gpu import ENTRY_POINTS
    model = _model(2)
    lm = model.model
    emb = T("ragged.prompt", (4, 40, 4096), 0.05).cuda()
    tok = lm.embed_tokens(torch.tensor([[5], [9], [1234], [77]])).cuda()
    names = ENTRY_POINTS + ["attention_shared"]
    calls = []
    saved = {n: getattr(hip, n) for n in names}

    def wrap(name, f):
        def g(*a, **k):
            r = f(*a, **k)
            calls.append((name, hip.lib().stllm_last_kernel().decode()))
            return r
        return g
    with runtime.use_dtype("bf16"):
        base = lm.new_cache(1, 40, "cuda")
        lm.prefill(emb[:1], None, cache=base)
        s = base.share(rows=4, max_new=8)
        try:
            for n, f in saved.items():
                setattr(hip, n, wrap(n, f))
            lm.decode_step(tok, s)
            torch.cuda.synchronize()
        finally:
            for n, f in saved.items():
                setattr(hip, n, f)
    got = [n for n, _ in calls]
    assert got.count("attention_shared") == 2 and got.count("attention") == 0 and got.count("kv_append_rows") == 2, got
    assert all(k == "attn_shared_decode_kernel" for n, k in calls if n == "attention_shared"), calls
    per_layer = [n for n in got if n != "gather_rows"]
    assert len(per_layer) == 2 * 8 + 1, per_layer          # rmsnorm, gemm, append, attention_shared, gemm, rmsnorm, gemm, gemm
    print(f"shared step: {len(per_layer) - 1} entry-point calls in 2 layers, attention family attn_shared_decode_kernel (partial pass + merge)")


# ---- H. memory -------------------------------------------------------------------------------------------------------------------------------------
def test_share_allocates_the_suffix_only(hip):
    from stllm_amd import runtime
    model = _model(2)
    lm = model.model
    with runtime.use_dtype("bf16"):
        base = lm.new_cache(1, 512, "cuda")
        base.len = 512
        torch.cuda.synchronize()
        m0 = torch.cuda.memory_allocated()
        s = base.share(rows=16, max_new=48)
        grown = torch.cuda.memory_allocated() - m0
        one_copy = 2 * 512 * 3 * 4096 * 2                      # layers x positions x [q | k | v] x bytes
        print(f"share(rows=16) behind P = 512: + {grown} bytes; one private prefix copy = {one_copy} bytes, 16 of them = {16 * one_copy}")
        assert s.base is base and 0 < grown < 2 * one_copy
