"""CPU: the fp64 references of tests/_train_refs.py, checked before any kernel is compared with them.

1. every closed-form backward agrees with torch.autograd through the fp64 forward of the same file to 1e-10 of the tensor's abs-max
   (attention: with the UNROUNDED o, so that delta = dO . o is the exact one);
2. every reference agrees with the fp32 restatement of the same contract in tests/_cpu_backend.py on one small case, at the tolerances
   tests/test_kernels_emulated_cpu.py uses for that restatement — two statements of each contract, written apart, that cannot drift apart;
3. the designed rounding of the 16-bit attention backward (P and dS rounded to 16 bit before the second product, outputs rounded once:
   _train_refs.attention_bwd_model16) stays below HALF the 16-bit bound of tests/test_train_kernels_gpu.py on every case of its table — the
   bound is reachable by a correct kernel — and the peaked cases really are peaked."""
import pytest
import torch

import _cpu_backend as C
import _train_refs as R

F64 = torch.float64


def rnd(*shape, seed=0, std=1.0, shift=0.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64) * std + shift


def close(got, want, tol, what):
    err = R.rel_err(got, want)
    assert err <= tol, f"{what}: {err:.3e} of abs-max (tol {tol:g})"


def vjp(fn, inputs, cot):
    """gradients of <fn(*inputs), cot> w.r.t. every input"""
    leaves = [t.clone().requires_grad_(True) for t in inputs]
    with torch.enable_grad():
        out = fn(*leaves)
        return torch.autograd.grad((out * cot).sum(), leaves)


# ---- 1. closed forms against autograd ------------------------------------------------------------------------------------------------------------
def test_norm_backward_closed_forms_match_autograd():
    M, D = 13, 72
    x, gamma, beta, dy = rnd(M, D, seed=1, std=2.0, shift=0.3), rnd(D, seed=2, std=0.2, shift=1.0), rnd(D, seed=3), rnd(M, D, seed=4)
    gx, gg = vjp(lambda a, g: R.rmsnorm_fwd(a, g, 1e-6), (x, gamma), dy)
    dx, dgamma = R.rmsnorm_bwd(x, gamma, 1e-6, dy)
    close(dx, gx, 1e-10, "rmsnorm dx"); close(dgamma, gg, 1e-10, "rmsnorm dgamma")
    gx, gg, gb = vjp(lambda a, g, b: R.layernorm_fwd(a, g, b, 1e-5), (x, gamma, beta), dy)
    dx, dgamma, dbeta = R.layernorm_bwd(x, gamma, 1e-5, dy)
    close(dx, gx, 1e-10, "layernorm dx"); close(dgamma, gg, 1e-10, "layernorm dgamma"); close(dbeta, gb, 1e-10, "layernorm dbeta")


def test_elementwise_backward_closed_forms_match_autograd():
    gu, dg = rnd(5, 192, seed=5, std=2.0), rnd(5, 96, seed=6)
    close(R.swiglu_bwd(gu, dg), vjp(R.swiglu_fwd, (gu,), dg)[0], 1e-10, "swiglu_bwd")
    x, dy = torch.linspace(-12, 12, 7 * 64, dtype=F64).reshape(7, 64), rnd(7, 64, seed=7)
    close(R.gelu_bwd(x, dy), vjp(R.gelu_fwd, (x,), dy)[0], 1e-10, "gelu_bwd")
    y = rnd(7, 64, seed=8)
    close(R.relu_bwd(dy, R.relu_fwd(y)), vjp(R.relu_fwd, (y,), dy)[0], 1e-10, "relu_bwd")
    sc = rnd(3, seed=9).abs()
    idx = torch.tensor([2, 0, 1, 1, 0, 2, 2], dtype=torch.int32)
    close(R.scale_rows(dy, sc, idx=idx), vjp(lambda a: R.scale_rows_fwd(a, sc, idx), (x,), dy)[0], 1e-10, "scale_rows")


def test_rope_backward_is_the_transpose_of_the_forward():
    from stllm_amd import pack
    S, B, N, rc = 9, 2, 768, 512
    cos, sin = pack.rope_tables(S, 128)
    x, dy = rnd(B * S, N, seed=10), rnd(B * S, N, seed=11)
    got = R.rope_bwd(dy, cos, sin, S, rc)
    close(got, vjp(lambda a: R.rope_fwd(a, cos, sin, S, rc), (x,), dy)[0], 1e-10, "rope_bwd")
    assert torch.equal(got[:, rc:], dy[:, rc:])


@pytest.mark.parametrize("causal,kv_len,Sq,Skv", [(True, None, 37, 37), (True, [37, 5], 37, 37), (False, [20, 41], 9, 41), (True, [0, 37], 37, 37)])
def test_attention_backward_closed_form_matches_autograd(causal, kv_len, Sq, Skv):
    B, H, D = 2, 2, 24
    q, k, v, do = rnd(B, Sq, H, D, seed=12), rnd(B, Skv, H, D, seed=13), rnd(B, Skv, H, D, seed=14), rnd(B, Sq, H, D, seed=15)
    scale = D ** -0.5
    fwd = lambda a, b, c: R.attention_fwd(a, b, c, scale, causal, kv_len)
    want = vjp(fwd, (q, k, v), do)
    got = R.attention_bwd(q, k, v, fwd(q, k, v), do, scale, causal, kv_len)
    for g, w, n in zip(got, want, ("dq", "dk", "dv")):
        assert torch.isfinite(g).all(), n
        if w.abs().max() == 0:
            assert g.abs().max() == 0, n
        else:
            close(g, w, 1e-10, n)
    if kv_len is not None:
        for b, L in enumerate(kv_len):
            assert not got[1][b, max(L, 0):].any() and not got[2][b, max(L, 0):].any(), "dk / dv rows at or behind kv_len are 0"
            if L <= 0:
                assert not got[0][b].any(), "kv_len <= 0: zero dq"


def test_loss_backward_closed_forms_match_autograd():
    n, V, Vp = 6, 50, 64
    logits = rnd(n, Vp, seed=16, std=3.0)
    labels = torch.tensor([5, -100, 49, 0, -100, 17], dtype=torch.int32)
    want = vjp(lambda a: R.cross_entropy_fwd(a, labels, 0.25, V), (logits,), torch.ones((), dtype=F64))[0]
    got = R.cross_entropy_bwd(logits, labels, 0.25, V)
    close(got, want, 1e-10, "cross_entropy_bwd")
    assert not got[:, V:].any() and not got[1].any()
    a, b = rnd(9, 40, seed=17), rnd(20, 40, seed=18)
    ia = torch.tensor([0, 8, 3, 3, 1, 2, 5], dtype=torch.int32)
    ib = torch.tensor([3, 1, 4, 1, 5, 9, 19], dtype=torch.int32)
    aa = a[ia.long()]                         # the gradient is w.r.t. the GATHERED rows
    want = vjp(lambda t: 0.3 * R.cosine_rows_fwd(t, b, None, ib).sum(), (aa,), torch.ones((), dtype=F64))[0]
    close(R.cosine_rows_bwd(a, b, ia, ib, 0.3), want, 1e-10, "cosine_rows_bwd")


def test_linear_transposes_match_autograd():
    # scatter_add_rows is the transpose of gather_rows; bcast_add_t of mean_t up to 1 / T; colsum of a row broadcast
    src = rnd(7, 12, seed=19)
    idx = torch.tensor([0, 3, -1, 3, -5, 2, -1], dtype=torch.int32)
    a0, b0 = torch.zeros(4, 12, dtype=F64), torch.zeros(6, 12, dtype=F64)
    ga, gb = vjp(lambda a, b: 0.5 * R.gather_fwd(a, b, idx), (a0, b0), src)
    wa, wb = R.scatter_add_rows(src, idx, a0, b0, 0.5)
    close(wa, ga, 1e-10, "scatter dst_a"); close(wb, gb, 1e-10, "scatter dst_b")
    x, g = rnd(2, 3, 8, seed=20), rnd(2, 8, seed=21)
    close(R.bcast_add_t(torch.zeros_like(x), g, 1 / 3), vjp(R.mean_t_fwd, (x,), g)[0], 1e-10, "bcast_add_t")
    y, dbias = rnd(11, 8, seed=22), rnd(8, seed=23)
    close(R.colsum(y), vjp(lambda bias: y * 0 + bias, (dbias,), y)[0], 1e-10, "colsum")
    t = torch.arange(15.0).reshape(3, 5)
    assert torch.equal(R.transpose(t, pad=4), torch.cat((t.t(), torch.zeros(5, 1)), dim=1))


def test_adamw_reference_matches_torch_optim():
    n = 300
    p, g = rnd(n, seed=24), rnd(n, seed=25)
    m, v = torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    w = p.clone().requires_grad_(True)
    opt = torch.optim.AdamW([w], lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1)
    for step in (1, 2, 3):
        w.grad = (g * 0.5 * step).clone()
        opt.step()
        p, m, v = R.adamw(p, g * step, m, v, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.1, step=step, grad_scale=0.5)
    close(p, w.detach(), 1e-12, "adamw vs torch.optim.AdamW")
    close(R.sumsq(g), (g * g).sum(), 1e-14, "sumsq")


# ---- 2. against the restatements of tests/_cpu_backend.py ------------------------------------------------------------------------------------------
def test_references_agree_with_the_cpu_backend():
    f = lambda t: t.float()
    M, D = 13, 72
    x, gamma, dy = f(rnd(M, D, seed=30, std=2.0, shift=0.3)), f(rnd(D, seed=31, std=0.2, shift=1.0)), f(rnd(M, D, seed=32))
    dx = torch.zeros(M, D)
    dgamma = C.rmsnorm_bwd(x, gamma, 1e-6, dy, dx, accumulate=False)
    for g, w, n in zip((dx, dgamma), R.rmsnorm_bwd(x, gamma, 1e-6, dy), ("dx", "dgamma")):
        close(g, w, 1e-5, "rmsnorm_bwd " + n)
    for g, w, n in zip(C.layernorm_bwd(x, gamma, 1e-5, dy), R.layernorm_bwd(x, gamma, 1e-5, dy), ("dx", "dgamma", "dbeta")):
        close(g, w, 1e-5, "layernorm_bwd " + n)
    gu, dg = f(rnd(5, 192, seed=33)), f(rnd(5, 96, seed=34))
    close(C.swiglu(gu), R.swiglu(gu), 1e-5, "swiglu")
    close(C.swiglu_bwd(gu, dg), R.swiglu_bwd(gu, dg), 1e-5, "swiglu_bwd")
    from stllm_amd import pack
    cos, sin = pack.rope_tables(5, 128)
    d = f(rnd(10, 384, seed=35))
    close(C.rope_bwd(d.clone(), cos, sin, rope_seq=5, rope_cols=256), R.rope_bwd(d, cos, sin, 5, 256), 1e-5, "rope_bwd")
    logits = f(rnd(6, 64, seed=36, std=3.0))
    labels = torch.tensor([5, -100, 49, 0, -100, 17], dtype=torch.int32)
    close(C.cross_entropy_bwd(logits, labels, 0.25, dtype=torch.float32, vocab=50), R.cross_entropy_bwd(logits, labels, 0.25, 50), 1e-5, "ce_bwd")
    src = f(rnd(7, 12, seed=37))
    idx = torch.tensor([0, 3, -1, 3, -5, 2, -1], dtype=torch.int32)
    a0, b0 = f(rnd(4, 12, seed=38)), f(rnd(6, 12, seed=39))
    wa, wb = R.scatter_add_rows(src, idx, a0, b0, 0.5)
    ga, gb = a0.clone(), b0.clone()
    C.scatter_add_rows(src, idx, ga, gb, scale=0.5)
    close(ga, wa, 1e-6, "scatter dst_a"); close(gb, wb, 1e-6, "scatter dst_b")
    a, b = f(rnd(9, 40, seed=40)), f(rnd(20, 40, seed=41))
    ib = torch.tensor([3, 1, 4, 1, 5, 9, 2, 6, 19], dtype=torch.int32)
    close(C.cosine_rows_bwd(a, b, None, ib, n_rows=9, scale=1 / 9), R.cosine_rows_bwd(a, b, None, ib, 1 / 9), 1e-5, "cosine_rows_bwd")
    y = f(rnd(11, 16, seed=42))
    close(C.colsum(y), R.colsum(y), 1e-5, "colsum")
    close(C.relu_bwd(y, -y + 0.1), R.relu_bwd(y, -y + 0.1), 0.0, "relu_bwd")
    xg = torch.linspace(-12, 12, 11 * 16).reshape(11, 16)
    close(C.gelu(xg), R.gelu(xg), 2e-6, "gelu")
    close(C.gelu_bwd(xg, y), R.gelu_bwd(xg, y), 2e-6, "gelu_bwd")
    sc = f(rnd(4, seed=43))
    close(C.scale_rows(y.clone(), sc, rows_per_group=3), R.scale_rows(y, sc, rows_per_group=3), 1e-6, "scale_rows")
    dst, s2 = f(rnd(2, 3, 8, seed=44)), f(rnd(2, 8, seed=45))
    want = R.bcast_add_t(dst, s2, 1 / 3)
    C.bcast_add_t(dst, s2, 1 / 3)
    close(dst, want, 1e-6, "bcast_add_t")
    assert torch.equal(C.transpose(y, pad=8), R.transpose(y, pad=8))
    n = 300
    p, g, m, v = f(rnd(n, seed=46)), f(rnd(n, seed=47)), f(rnd(n, seed=48).abs() * 0.1), f(rnd(n, seed=49).abs() * 0.01)
    kw = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.1, step=3, grad_scale=0.5)
    want = R.adamw(p, g, m, v, **kw)
    C.adamw(p, g, m, v, **kw)
    for got, w, nme in zip((p, m, v), want, "pmv"):
        close(got, w, 2e-6, "adamw " + nme)
    close(C.sumsq(g)[0], R.sumsq(g), 1e-5, "sumsq")


@pytest.mark.parametrize("causal,kv_len,Sq,Skv", [(True, [37, 5], 37, 37), (False, None, 9, 41)])
def test_attention_reference_agrees_with_the_cpu_backend(causal, kv_len, Sq, Skv):
    B, H, D = 2, 2, 24
    q, k, v, do = (rnd(B, S, H, D, seed=50 + i, std=0.7).float() for i, S in enumerate((Sq, Skv, Skv, Sq)))
    flat = lambda t: t.reshape(-1, H * D)
    kl = None if kv_len is None else torch.tensor(kv_len, dtype=torch.int32)
    o = C.attention(flat(q), flat(k), flat(v), B=B, H=H, Sq=Sq, Skv=Skv, D=D, scale=D ** -0.5, causal=causal, kv_len=kl)
    close(o, flat(R.attention_fwd(q.double(), k.double(), v.double(), D ** -0.5, causal, kv_len)), 2e-5, "attention forward")
    got = [torch.zeros(B * S, H * D) for S in (Sq, Skv, Skv)]
    C.attention_bwd(flat(q), flat(k), flat(v), o, flat(do), *got, B=B, H=H, Sq=Sq, Skv=Skv, D=D, scale=D ** -0.5, causal=causal, kv_len=kl)
    want = R.attention_bwd(q, k, v, o.view(B, Sq, H, D), do, D ** -0.5, causal, kv_len)
    for g, w, n in zip(got, want, ("dq", "dk", "dv")):
        close(g, flat(w), 2e-5, n)


# ---- 3. the 16-bit attention bounds are reachable, the peaked cases are peaked ------------------------------------------------------------------
@pytest.mark.parametrize("case", R.ATTN_CASES, ids=R.ATTN_IDS)
def test_designed_16_bit_rounding_stays_below_half_the_bound(case):
    name, B, H, Sq, Skv, D, causal, kv_len, kind = case
    for dtype in ("bf16",) if name in R.ATTN_BF16_ONLY else ("bf16", "fp16"):
        q, k, v, o, do = R.attn_inputs(case, dtype)
        want = R.attention_bwd(q, k, v, o, do, D ** -0.5, causal, kv_len)
        model = R.attention_bwd_model16(q, k, v, o, do, D ** -0.5, causal, kv_len, R.DTYPES[dtype])
        for g, w, n in zip(model, want, ("dq", "dk", "dv")):
            err = R.rel_err(g, w)
            assert err <= 0.5 * R.ATTN_TOL[dtype], f"{name} {dtype} {n}: designed rounding alone is {err / R.ATTN_TOL[dtype]:.2f} of the bound"


@pytest.mark.parametrize("case", [c for c in R.ATTN_CASES if c[8] == "peaked"], ids=lambda c: c[0])
def test_peaked_cases_have_one_dominant_weight_per_row(case):
    name, B, H, Sq, Skv, D, causal, kv_len, kind = case
    for dtype in ("bf16", "fp16", "fp32"):
        q, k, v, o, do = R.attn_inputs(case, dtype)
        top = R.attention_probs(q, k, D ** -0.5, causal, kv_len).amax(-1).mean().item()
        assert top >= 0.5, f"{name} {dtype}: mean largest softmax weight {top:.3f}"
    flat_case = next(c for c in R.ATTN_CASES if c[0] == "eva_257")
    q, k, v, o, do = R.attn_inputs(flat_case, "fp32")
    assert R.attention_probs(q, k, 88 ** -0.5, False, None).amax(-1).mean().item() < 0.05      # what N(0, 0.7^2) inputs give: a flat softmax
