"""GPU (-m gpu): the backward / optimizer kernels of csrc/attention_bwd.hip and csrc/train_ops.hip on the device, in-process, against the plain
fp64 references of tests/_train_refs.py (themselves checked against torch.autograd by tests/test_train_refs_cpu.py), at the widths the model runs
them at and on the edges of their tiles, loops and grids.  Calls go to stllm_amd.hip with device tensors.

Rules of the file
  * inputs are rounded to the compute dtype before either side sees them; data are asymmetric random;
  * strided operands carry NaN in the gap behind their columns (never read), outputs sit inside 0xFF-filled guard buffers (never written);
  * attention backward: the tolerances of test_kernels_emulated_cpu.py::test_attention_bwd — fp32 2e-5 of the tensor's abs-max, bf16 2^-6, fp16 2^-9
    (test_train_refs_cpu.py shows that the designed 16-bit rounding alone stays below half of these on every case); every case runs twice, bit-identical;
  * elementwise results: fp32 outputs 1e-5 of abs-max, 16-bit outputs OUT_TOL of test_kernels_gpu.py;
  * reductions (dgamma, dbeta, colsum, sumsq): no chosen number — |err| <= (chain + 1) * 2^-24 * sum |terms| with `chain` the longest path of fp32
    additions (and roundings of a term) in the kernel, derived next to each use.
Every test prints `TRAINERR <what> <error / bound>` before it asserts (pytest -s shows them; profiles/train_kernel_tests.md records one run)."""
import functools
import math

import pytest
import torch

import _poison
import _train_refs as R
from test_kernels_gpu import OUT_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = ["bf16", "fp16", "fp32"]
EPS24 = 2.0 ** -24
ELT_TOL = dict(OUT_TOL, fp32=1e-5)       # elementwise outputs


@pytest.fixture(scope="module")
def hip():
    from stllm_amd import hip as h
    h.lib()
    return h


def rnd(*shape, seed, std=1.0, shift=0.0, dtype="fp32"):
    """asymmetric random values already rounded to `dtype`, as an fp64 CPU tensor"""
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * std + shift
    return x.to(R.DTYPES[dtype]).double()


def dev(x, dtype="fp32"):
    """the device copy of the 2-D fp64 tensor x in `dtype`, as a row-strided view (ld = cols + 8) with NaN in the gap"""
    return _poison.nan_padded(x.to(R.DTYPES[dtype]).to(DEV))


def report(what, err, bound):
    print(f"TRAINERR {what} {err / bound if bound > 0 else float(err > 0):.3f}")


def check(got, ref, tol, what):
    """max |got - ref| <= tol * abs-max(ref), got finite"""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, f"{what}: {got.shape} vs {ref.shape}"
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    scale = max(ref.abs().max().item(), 1e-30)
    err = (got - ref).abs().max().item()
    report(what, err, tol * scale)
    assert err <= tol * scale, f"{what}: max err {err:.3e} > {tol:.2e} * {scale:.3e}"


def check_sum(got, ref, abs_terms, chain, what):
    """a reduction: |got - ref| <= (chain + 1) * 2^-24 * sum |terms| per output element"""
    got = got.detach().double().cpu().reshape(ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    bound = (chain + 1) * EPS24 * abs_terms.double().reshape(ref.shape)
    ratio = ((got - ref).abs() / bound.clamp(min=1e-300)).max().item()
    report(f"{what} (chain {chain})", ratio, 1.0)
    assert ratio <= 1.0, f"{what}: {ratio:.2f} of the derived bound (chain {chain})"


def same_bits(a, b):
    return _poison.bits_equal(a.contiguous(), b.contiguous())


# =================================================================================================================================================
# attention backward
# =================================================================================================================================================
@functools.lru_cache(maxsize=None)
def attn_case(name, dtype):
    """(inputs, reference) of a case: computed once, shared, never modified"""
    case = R.ATTN_CASES[R.ATTN_IDS.index(name)]
    inp = R.attn_inputs(case, dtype)
    ref = R.attention_bwd(*inp, case[5] ** -0.5, case[6], case[7])
    return case, inp, ref


class Fused:
    """n logical [B, S, H, D] tensors as column blocks of ONE 2-D buffer [B * S_alloc, n * H * D + pad_cols] — the fused-QKV layout of the model.
    With S_alloc > S / pad_cols > 0 the batch stride is larger than S * row stride, and the gap rows and columns hold `fill`."""

    def __init__(self, B, S, HD, n, td, S_alloc=None, pad_cols=0, fill=float("nan"), ff=False):
        self.B, self.S, self.HD, self.n = B, S, HD, n
        self.S_alloc = S_alloc or S
        self.W = n * HD + pad_cols
        if ff:      # every byte 0xFF
            self.buf = torch.full((B * self.S_alloc, self.W * torch.empty(0, dtype=td).element_size()), 0xFF, dtype=torch.uint8, device=DEV).view(td)
        else:
            self.buf = torch.full((B * self.S_alloc, self.W), fill, dtype=td, device=DEV)
        self.strides = (self.S_alloc * self.W, self.W)

    def part(self, i):
        """the 2-D view a kernel gets for block i"""
        return self.buf[:, i * self.HD:(i + 1) * self.HD]

    def logical(self, i=None):
        v = self.buf.view(self.B, self.S_alloc, self.W)[:, :self.S]
        return v[:, :, :self.n * self.HD] if i is None else v[:, :, i * self.HD:(i + 1) * self.HD]

    def put(self, i, x):
        self.logical(i).copy_(x.reshape(self.B, self.S, self.HD).to(self.buf.dtype))

    def get(self, i, H):
        return self.logical(i).reshape(self.B, self.S, H, self.HD // H)

    def outside_untouched(self):
        """every byte outside the logical [B, S, n * H * D] region still 0xFF"""
        it = {2: torch.int16, 4: torch.int32}[self.buf.element_size()]
        c = self.buf.clone().view(it)
        c.view(self.B, self.S_alloc, self.W)[:, :self.S, :self.n * self.HD] = -1
        return bool((c == -1).all())


def run_attention_bwd(hip, name, dtype, path, layout=False):
    (_, B, H, Sq, Skv, D, causal, kv_len, _), (q, k, v, o, do), ref = attn_case(name, dtype)
    td, HD = R.DTYPES[dtype], H * D
    gap = dict(S_alloc=Sq + 5, pad_cols=64) if layout else {}
    assert not layout or Sq == Skv
    if Sq == Skv:                                   # q | k | v in one fused buffer, dq | dk | dv in a second one
        src = Fused(B, Sq, HD, 3, td, **gap)
        for i, t in enumerate((q, k, v)):
            src.put(i, t)
        ins, ins_kv = (src, 0), ((src, 1), (src, 2))
        mk_out = lambda: (lambda f: ((f, 0), (f, 1), (f, 2)))(Fused(B, Sq, HD, 3, td, ff=True, **gap))
    else:                                           # cross-attention: q alone, k | v fused
        sq, skv = Fused(B, Sq, HD, 1, td), Fused(B, Skv, HD, 2, td)
        sq.put(0, q); skv.put(0, k); skv.put(1, v)
        ins, ins_kv = (sq, 0), ((skv, 0), (skv, 1))
        mk_out = lambda: (lambda a, b: ((a, 0), (b, 0), (b, 1)))(Fused(B, Sq, HD, 1, td, ff=True), Fused(B, Skv, HD, 2, td, ff=True))
    od, dod = (t.reshape(B * Sq, HD).to(td).to(DEV) for t in (o, do))
    kl = None if kv_len is None else torch.tensor(kv_len, dtype=torch.int32, device=DEV)
    runs = []
    hip.set_option("attn_bwd_valu", 1 if path == "valu" else 0)
    try:
        for _ in range(2):
            outs = mk_out()
            (fq, iq), (fk, ik), (fv, iv) = outs
            hip.attention_bwd(ins[0].part(ins[1]), ins_kv[0][0].part(ins_kv[0][1]), ins_kv[1][0].part(ins_kv[1][1]), od, dod,
                              fq.part(iq), fk.part(ik), fv.part(iv), B=B, H=H, Sq=Sq, Skv=Skv, D=D, scale=D ** -0.5, causal=causal, kv_len=kl,
                              strides=ins[0].strides, kv_strides=ins_kv[0][0].strides, d_strides=fq.strides, dkv_strides=fk.strides)
            if DEV == "cuda":
                torch.cuda.synchronize()
            runs.append(outs)
    finally:
        hip.set_option("attn_bwd_valu", 0)
    what = f"attention_bwd {name} {dtype} {path}" + (" layout" if layout else "")
    got = [f.get(i, H) for f, i in runs[0]]
    again = [f.get(i, H) for f, i in runs[1]]
    for f in {id(f): f for f, _ in runs[0]}.values():
        assert f.outside_untouched(), f"{what}: a byte outside the logical [B, S, H * D] regions was written"
    for g, g2, n in zip(got, again, ("dq", "dk", "dv")):
        assert torch.isfinite(g).all(), f"{what} {n}: an in-range element is not finite (never written, or computed from a masked row)"
        assert torch.equal(g, g2), f"{what} {n}: two runs differ (there are no atomics in these kernels)"
    if kv_len is not None:
        for b, L in enumerate(kv_len):
            L = max(L, 0)
            assert not got[1][b, L:].any() and not got[2][b, L:].any(), f"{what}: dk / dv rows at or behind kv_len[{b}] = {L} must be exactly 0"
            if L == 0:
                assert not got[0][b].any(), f"{what}: kv_len[{b}] = 0 must give zero dq"
    for g, w, n in zip(got, ref, ("dq", "dk", "dv")):
        check(g, w, R.ATTN_TOL[dtype], f"{what} {n}")


ATTN_PARAMS = [(c[0], d) for c in R.ATTN_CASES for d in (("bf16",) if c[0] in R.ATTN_BF16_ONLY else DT)]


@pytest.mark.parametrize("name,dtype", ATTN_PARAMS, ids=[f"{n}-{d}" for n, d in ATTN_PARAMS])
def test_attention_bwd(hip, name, dtype):
    """bf16 / fp16 on the MFMA kernels, fp32 on the VALU kernels"""
    run_attention_bwd(hip, name, dtype, "valu" if dtype == "fp32" else "mfma")


# one 16-bit case per head dim on the VALU twins (+ the Sq != Skv shape)
@pytest.mark.parametrize("name,dtype", [("llama_129_len", "bf16"), ("eva_257", "fp16"), ("qf_self", "bf16"), ("qf_cross", "fp16"), ("d40", "bf16"),
                                        ("d72", "bf16"), ("d104", "bf16")])
def test_attention_bwd_valu_16_bit(hip, name, dtype):
    run_attention_bwd(hip, name, dtype, "valu")


@pytest.mark.parametrize("name,dtype,path", [("llama_129_len", "bf16", "mfma"), ("qf_self", "fp16", "valu"), ("llama_300_len", "fp32", "valu")])
def test_attention_bwd_fused_layout_with_gaps(hip, name, dtype, path):
    """q | k | v inside [B * (S + 5), 3 H D + 64] with NaN in the gap rows and columns (never read), +-1e3 in the K / V rows behind kv_len (read,
    weightless), dq | dk | dv inside a 0xFF-filled buffer of the same shape: nothing outside [B, S, H D] is written, everything inside is"""
    run_attention_bwd(hip, name, dtype, path, layout=True)


# =================================================================================================================================================
# norm backward, column sums
# =================================================================================================================================================
def col_chain(M):
    """col_partial_kernel + col_final_kernel: a thread adds ceil(rows_per / 4) rows (rows_per = ceil(M / 64)), 3 additions join the 4 row lanes,
    col_final_kernel adds the 64 partials in order"""
    return -(-(-(-M // 64)) // 4) + 3 + 64


def stat_chain(D):
    """mu / r of norm_bwd_dx_kernel: a lane adds D / 64 values (D / 256 float4 steps), 6 shuffle levels, then divide, add eps, rsqrt"""
    return D // 64 + 6 + 3


def run_norm_bwd(hip, rms, M, D, dy_dtype, accumulate):
    x = rnd(M, D, seed=1, std=2.0, shift=0.3)                     # "x * 2 + 0.3"
    gamma = rnd(D, seed=2, std=0.2, shift=1.0)
    dy = rnd(M, D, seed=3, shift=0.05, dtype=dy_dtype)
    dx0 = rnd(M, D, seed=4)
    eps = 1e-6 if rms else 1e-5
    want = (R.rmsnorm_bwd if rms else R.layernorm_bwd)(x, gamma, eps, dy)
    t_xh, t_dy = R.norm_terms(x, eps, dy, rms)
    xd, dyd, gd = dev(x), dev(dy, dy_dtype), gamma.float().to(DEV)
    outs = []
    for _ in range(2):
        g = _poison.Guarded(M, D, torch.float32, device=DEV)
        g.out.copy_(dx0.float())
        if rms:
            red = (hip.rmsnorm_bwd(xd, gd, eps, dyd, g.out, accumulate=accumulate),)
        else:
            red = hip.layernorm_bwd(xd, gd, eps, dyd, g.out, accumulate=accumulate)[1:]
        assert g.intact(), "norm backward: a byte outside the M x D dx was written"
        outs.append((g.out.clone(),) + tuple(red))
    what = f"{'rmsnorm' if rms else 'layernorm'}_bwd {M}x{D} dy {dy_dtype} acc {int(accumulate)}"
    for a, b in zip(*outs):
        assert same_bits(a, b), f"{what}: two runs differ (deterministic two-stage reduction)"
    check(outs[0][0], want[0] + (dx0 if accumulate else 0), 1e-5, what + " dx")
    # dgamma: the column chain + 3 roundings of a term ((x - mu) * r * dy) + the chain behind mu and r; a term's error also scales with
    # |dy| |mu| r (the error of mu enters xh absolutely, not relative to x - mu)
    mu_r = 0.0 if rms else (x.mean(-1) * torch.rsqrt(x.var(-1, unbiased=False) + eps)).abs().max().item()
    check_sum(outs[0][1], want[1], t_xh + mu_r * t_dy, col_chain(M) + 3 + stat_chain(D), what + " dgamma")
    if not rms:
        check_sum(outs[0][2], want[2], t_dy, col_chain(M), what + " dbeta")


@pytest.mark.parametrize("dy_dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("accumulate", [True, False])
@pytest.mark.parametrize("M,D", [(577, 4096), (37, 4096)])          # 16 passes of every `c += 64` loop; rows_per 10 (a ragged last slab) and 1
def test_rmsnorm_bwd(hip, M, D, accumulate, dy_dtype):
    run_norm_bwd(hip, True, M, D, dy_dtype, accumulate)


@pytest.mark.parametrize("dy_dtype", DT)
# 352 / 192 float4 per row: 5.5 and 3 passes; rows_per 9 and 2.  At those M the last of the 64 row slabs is empty (63 * rows_per >= M), so (128, 768)
# is here too: rows_per 2 and every slab holds rows — a partial dropped or doubled by col_final_kernel shows in dgamma and dbeta as well
@pytest.mark.parametrize("M,D", [(514, 1408), (70, 768), (128, 768)])
def test_layernorm_bwd(hip, M, D, dy_dtype):
    run_norm_bwd(hip, False, M, D, dy_dtype, False)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("M,N", [(4112, 1408), (65, 136)])           # rows_per 65: 17 steps per thread, last slab 17 rows; rows_per 2: slabs >= 33 empty
def test_colsum(hip, M, N, dtype):
    x = rnd(M, N, seed=5, shift=0.1, dtype=dtype)
    xd = dev(x, dtype)
    a, b = hip.colsum(xd), hip.colsum(xd)
    assert same_bits(a, b), "colsum: two runs differ"
    check_sum(a, R.colsum(x), x.abs().sum(0), col_chain(M), f"colsum {M}x{N} {dtype}")


# =================================================================================================================================================
# elementwise kernels
# =================================================================================================================================================
def raw(hip, name, *args):
    """an entry point whose wrapper allocates its own output, called on a guarded output instead"""
    hip._check(getattr(hip._tlib(), name)(*args, hip._stream()), name)


@pytest.mark.parametrize("dtype", DT)
def test_swiglu_and_backward(hip, dtype):
    M, I = 37, 11008                                                  # 344 packed column groups
    td = R.DTYPES[dtype]
    gu, dg = rnd(M, 2 * I, seed=6, std=2.0, shift=0.1, dtype=dtype), rnd(M, I, seed=7, shift=-0.05, dtype=dtype)
    gud, dgd = dev(gu, dtype), dev(dg, dtype)
    go, gb = _poison.Guarded(M, I, td, device=DEV), _poison.Guarded(M, 2 * I, td, device=DEV)
    hip.swiglu(gud, out=go.out)
    hip.swiglu_bwd(gud, dgd, out=gb.out)
    assert go.intact() and gb.intact(), "swiglu: a byte outside the outputs was written"
    check(go.out, R.swiglu(gu), ELT_TOL[dtype], f"swiglu {dtype}")
    check(gb.out, R.swiglu_bwd(gu, dg), ELT_TOL[dtype], f"swiglu_bwd {dtype}")


@pytest.mark.parametrize("dtype", DT)
def test_gelu_and_backward(hip, dtype):
    M, N = 37, 6144
    td, code = R.DTYPES[dtype], hip.dtype_code(R.DTYPES[dtype])
    g = torch.Generator().manual_seed(8)
    x = (torch.rand(M, N, generator=g, dtype=torch.float64) * 24 - 12).to(td).double()       # covers [-12, 12]: both tails of erf and exp
    x[0, :4] = torch.tensor([-12.0, 12.0, 0.0, -0.0])
    dy = rnd(M, N, seed=9, shift=0.05, dtype=dtype)
    xd, dyd = dev(x, dtype), dev(dy, dtype)
    go, gb = _poison.Guarded(M, N, td, device=DEV), _poison.Guarded(M, N, td, device=DEV)
    raw(hip, "stllm_gelu", code, hip._p(xd), xd.stride(0), hip._p(go.out), go.out.stride(0), M, N)
    raw(hip, "stllm_gelu_bwd", code, hip._p(xd), xd.stride(0), hip._p(dyd), dyd.stride(0), hip._p(gb.out), gb.out.stride(0), M, N)
    assert go.intact() and gb.intact(), "gelu: a byte outside the outputs was written"
    check(go.out, R.gelu(x), ELT_TOL[dtype], f"gelu {dtype}")
    check(gb.out, R.gelu_bwd(x, dy), ELT_TOL[dtype], f"gelu_bwd {dtype}")
    assert same_bits(hip.gelu(xd), go.out) and same_bits(hip.gelu_bwd(xd, dyd), gb.out), "the wrappers give what the guarded calls gave"


@pytest.mark.parametrize("dtype", DT)
def test_relu_bwd_and_scale_rows(hip, dtype):
    M, N = 70, 768
    td, code = R.DTYPES[dtype], hip.dtype_code(R.DTYPES[dtype])
    dy, y = rnd(M, N, seed=10, shift=0.05, dtype=dtype), rnd(M, N, seed=11, shift=0.2, dtype=dtype)
    y[3, :8] = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 1.0, -1.0, 0.0, 0.0]).to(td).double()
    dyd, yd = dev(dy, dtype), dev(y, dtype)
    g = _poison.Guarded(M, N, td, device=DEV)
    raw(hip, "stllm_relu_bwd", code, hip._p(dyd), dyd.stride(0), hip._p(yd), yd.stride(0), hip._p(g.out), g.out.stride(0), M, N)
    assert g.intact(), "relu_bwd: a byte outside the output was written"
    want = R.relu_bwd(dy, y)
    check(g.out, want, ELT_TOL[dtype], f"relu_bwd {dtype}")
    assert torch.equal(g.out.double().cpu(), want), "relu_bwd is exact"
    assert same_bits(hip.relu_bwd(dyd, yd), g.out)
    scale = rnd(7, seed=12, shift=0.5).abs()
    scale[2] = 0.0                                                    # a dropped sample
    idx = torch.randint(0, 7, (M,), generator=torch.Generator().manual_seed(13)).to(torch.int32)
    for kw, rkw, n in ((dict(idx=idx.to(DEV)), dict(idx=idx), "idx"), (dict(rows_per_group=10), dict(rows_per_group=10), "rows_per_group")):
        g = _poison.Guarded(M, N, td, device=DEV)
        g.out.copy_(dy.to(td))
        hip.scale_rows(g.out, scale.float().to(DEV), **kw)
        assert g.intact(), "scale_rows: a byte outside the rows was written"
        check(g.out, R.scale_rows(dy, scale.float(), **rkw), ELT_TOL[dtype], f"scale_rows {n} {dtype}")


@pytest.mark.parametrize("dtype", DT)
def test_rope_bwd(hip, dtype):
    from stllm_amd import pack
    B, S, heads = 2, 70, 4                                            # positions 0 .. 69 of the table, 4 heads of 128 as q | k | v
    N, rc = 3 * heads * 128, 2 * heads * 128
    td = R.DTYPES[dtype]
    cos, sin = pack.rope_tables(S, 128)
    d = rnd(B * S, N, seed=14, shift=0.05, dtype=dtype)
    g = _poison.Guarded(B * S, N, td, device=DEV)
    g.out.copy_(d.to(td))
    hip.rope_bwd(g.out, cos.to(DEV), sin.to(DEV), rope_seq=S, rope_cols=rc)
    assert g.intact(), "rope_bwd: a byte outside the rows was written"
    check(g.out, R.rope_bwd(d, cos, sin, S, rc), ELT_TOL[dtype], f"rope_bwd {dtype}")
    assert torch.equal(g.out[:, rc:].double().cpu(), d[:, rc:]), "the v third must come back bit-identical"


@pytest.mark.parametrize("dtype", DT)
def test_cross_entropy_bwd(hip, dtype):
    n, V, Vp = 7, 32001, 32128
    logits = rnd(n, Vp, seed=15, std=2.0, shift=0.1)
    logits[4] = (logits[4] * (80.0 / logits[4, :V].abs().max())).float().double()      # one row spread to +-80
    labels = torch.tensor([0, V - 1, -100, 17, 31999, -100, 5], dtype=torch.int32)
    want = R.cross_entropy_bwd(logits, labels, 0.2, V)
    poisoned = logits.clone()
    poisoned[:, V:] = float("nan")                                    # the lm_head padding columns of the logits are never read
    got = hip.cross_entropy_bwd(dev(poisoned), labels.to(DEV), 0.2, dtype=dtype, vocab=V)
    check(got, want, ELT_TOL[dtype], f"cross_entropy_bwd {dtype}")
    assert not got[:, V:].any() and not got[2].any() and not got[5].any(), "padding columns and ignored rows are written as 0"


def test_scatter_add_rows(hip):
    n, D = 40, 4096                                                   # 16 passes of the `c += 256` loop
    src = rnd(n, D, seed=16, shift=0.05)
    idx = torch.tensor([(i * 7) % 9 if i % 3 else -((i * 5) % 6) - 1 for i in range(n)], dtype=torch.int32)
    idx[torch.tensor([1, 4, 8, 13, 17, 22, 26, 31, 37])] = 9          # one destination row hit 9 times
    assert (idx == 9).sum() == 9
    a0, b0 = rnd(11, D, seed=17), rnd(6, D, seed=18)
    wa, wb = R.scatter_add_rows(src, idx, a0, b0, 0.5)
    ga, gb = _poison.Guarded(11, D, torch.float32, device=DEV), _poison.Guarded(6, D, torch.float32, device=DEV)
    ga.out.copy_(a0.float()); gb.out.copy_(b0.float())
    hip.scatter_add_rows(dev(src), idx.to(DEV), ga.out, gb.out, scale=0.5)
    assert ga.intact() and gb.intact(), "scatter_add_rows: a byte outside the destinations was written"
    check(ga.out, wa, 1e-5, "scatter_add_rows dst_a"); check(gb.out, wb, 1e-5, "scatter_add_rows dst_b")


def test_cosine_rows_bwd(hip):
    n, D = 33, 1408                                                   # 352 float4 per row: 5.5 passes of the `c += 64` loop; 9 blocks of 4 rows
    a, b = rnd(50, D, seed=19, shift=0.1), rnd(64, D, seed=20, shift=-0.1)
    g = torch.Generator().manual_seed(21)
    ia, ib = torch.randperm(50, generator=g)[:n].to(torch.int32), torch.randperm(64, generator=g)[:n].to(torch.int32)
    got = hip.cosine_rows_bwd(dev(a), dev(b), ia.to(DEV), ib.to(DEV), scale=1.0 / n)
    check(got, R.cosine_rows_bwd(a, b, ia, ib, 1.0 / n), 1e-5, "cosine_rows_bwd")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("R_,C_,pad", [(577, 4096, 64), (5, 200, 128)])     # 10 x 64 row tiles, the last ragged; rows_padded 128 > rows + 64
def test_transpose(hip, R_, C_, pad, dtype):
    td = R.DTYPES[dtype]
    x = rnd(R_, C_, seed=22, shift=0.05, dtype=dtype)
    Rp = (R_ + pad - 1) // pad * pad
    g = _poison.Guarded(C_, Rp, td, device=DEV)
    hip.transpose(dev(x, dtype), pad=pad, out=g.out)
    assert g.intact(), "transpose: a byte outside the C x Rp output was written"
    assert torch.equal(g.out.cpu(), R.transpose(x.to(td), pad)), "transpose must be exact, zero behind the rows"


# =================================================================================================================================================
# grid-stride kernels: more elements than one sweep of the capped grid
# =================================================================================================================================================
ADAM = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.1, step=3, grad_scale=0.5)


@pytest.mark.parametrize("p16", [None, "bf16", "fp16"])
@pytest.mark.parametrize("n", [16384 * 256 + 259, 257, 1])           # one full sweep of the 16384-block grid + a ragged second one
def test_adamw(hip, n, p16):
    p, g = rnd(n, seed=23, shift=0.05), rnd(n, seed=24, shift=-0.02)
    m, v = rnd(n, seed=25, std=0.1).abs(), rnd(n, seed=26, std=0.01).abs()
    want = R.adamw(p, g, m, v, **ADAM)
    pd, gd, md, vd = (t.float().to(DEV) for t in (p, g, m, v))
    h = _poison.Guarded(1, n, R.DTYPES[p16], device=DEV, pad=0) if p16 else None
    hip.adamw(pd, gd, md, vd, p16=h.out[0] if p16 else None, **ADAM)
    for got, w, nme in zip((pd, md, vd), want, "pmv"):
        check(got, w, 1e-5, f"adamw n={n} {nme}")
    assert torch.equal(gd.double().cpu(), g), "the gradient is read only"
    if p16:
        assert h.intact(), "adamw: a byte outside p16 was written"
        assert torch.equal(h.out[0], pd.to(R.DTYPES[p16])), "p16 is the cast of the new p"
        check(h.out[0], want[0], ELT_TOL[p16], f"adamw n={n} p16 {p16}")


def test_sumsq(hip):
    n = 2048 * 256 * 2 + 259                                          # two full sweeps of the 2048-block grid + a ragged third
    x = rnd(n, seed=27)
    x[0] = x[524288] = x[n - 1] = 30.0                                # first element, first element of the second sweep, last of the tail
    total = R.sumsq(x)
    # each planted element moves the sum by 900 / ~1.05e6 ~ 8.6e-4, ~7x the derived bound: a dropped tail or a wrong stride cannot hide under it
    assert 900.0 / total.item() > 5 * (3 + 6 + 3 + 2048 + 1) * EPS24
    out = torch.full((1,), 2.5, dtype=torch.float32, device=DEV)     # out[0] += ...
    hip.sumsq(x.float().to(DEV), out)
    # chain: 3 elements in a thread, 6 shuffle levels, 3 additions over the waves, 2048 atomic additions into out[0] (+ 1: the square itself)
    check_sum(out, (total + 2.5).reshape(1), (total + 2.5).reshape(1), 3 + 6 + 3 + 2048, "sumsq")


def test_bcast_add_t(hip):
    B, T, J = 2, 16, 2097160                                          # B T J / 4 = 16 777 280: 64 float4 more than one sweep of the 65536-block grid
    g = torch.Generator(device=DEV).manual_seed(28)
    dst = torch.randn(B, T, J, generator=g, device=DEV) + 0.05
    src = torch.randn(B, J, generator=g, device=DEV) - 0.1
    want = R.bcast_add_t(dst, src, 1.0 / T)                           # fp64 on the device: a host copy would dominate the test
    hip.bcast_add_t(dst, src, 1.0 / T)
    err, scale = (dst.double() - want).abs().max().item(), want.abs().max().item()
    report("bcast_add_t", err, 1e-5 * scale)
    assert math.isfinite(err) and err <= 1e-5 * scale, f"bcast_add_t: max err {err:.3e} > 1e-5 * {scale:.3e}"
