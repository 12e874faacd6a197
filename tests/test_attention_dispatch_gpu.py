"""GPU: stllm_attention, every dispatch configuration at its tile and window edges against fp64 (tests/_attention_case.py: inputs, reference, tolerances, names).

tests/test_kernels_gpu.py::test_attention runs the workload's shapes under two option settings; this file pins the DISPATCHER: every case asserts the kernel
stllm_last_kernel() reports, then the guards around the output, finiteness and the comparison (2 x OUT_TOL x abs-max for bf16 / fp16, 2e-5 x abs-max for fp32),
on a random input set and, where the shape has a mask boundary, on the planted set that makes the boundary decide the output.
  A. head_dim 128, 16-bit: the four LDS-DMA configurations forced through attn_dma = 10 x tiles + waves, each with attn_q_lds 1 and 0
  B. head_dim 128: the automatic rule, one shape per branch, and the register-staged kernel behind attn_dma = 0
  C. head_dim 88: dma88 / resident on the 96-key window edges, the temporal kernel, the fall-through
  D. head_dim 64: one and two waves
  E. fp32: matrix-core and vector kernel by attn_f32_mfma and the Sq >= 8 rule; the vector kernel's Skv bound"""
import pytest
import torch

import _attention_case as AC
import _poison
from _attention_case import Shape

pytestmark = pytest.mark.gpu
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DT16 = [pytest.param(BF16, id="bf16"), pytest.param(F16, id="fp16")]


@pytest.fixture(scope="module")
def hip():
    from stllm_amd import hip as h
    h.lib()
    return h


def run_all(hip, cases):
    """cases: (shape, dtype, options, name) — every one runs, the failures are reported together"""
    failed = []
    for shape, dtype, opts, name in cases:
        try:
            AC.run_case(hip, shape, dtype, opts, name)
        except AssertionError as e:
            failed.append(f"{shape.id} {opts}: {e}")
    assert not failed, "\n".join(failed)


# One test item per configuration, option setting and dtype, its table of shapes inside: every item ends in a collection + cache release (tests/conftest.py)
# that costs more than the launches of a whole table, and run_all reports every failing shape of the item, not the first.


# ---- A ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT16)
@pytest.mark.parametrize("q_lds", [1, 0])
@pytest.mark.parametrize("cfg", sorted(AC.DMA_CONFIGS))
def test_dma128_forced(hip, cfg, q_lds, dtype):
    ks2, tiles = AC.DMA_CONFIGS[cfg]
    run_all(hip, [(s, dtype, {"attn_dma": cfg, "attn_q_lds": q_lds}, AC.dma_name(dtype, ks2, tiles, s.Sq, q_lds)) for s in AC.A_SHAPES])


# ---- B ---------------------------------------------------------------------------------------------------------------------------------------------------------------
AUTO = [  # (B, H, S) -> the branch of dispatch<T>() it takes, written out
    ((1, 4, 70), "attn_dma_kernel<{T},4,128,512> nw=2 q_lds=1 merge_par=1"),      # B H <= 32, <= 20 query tiles: 4 key-split waves x 2 query tiles
    ((4, 32, 33), "attn_dma_kernel<{T},1,128,512> nw=2 q_lds=1 merge_par=0"),     # 128 workgroups with 12 tiles each: 1 x 12, clipped to the 2 tiles there are
    ((2, 32, 160), "attn_dma_kernel<{T},2,128,512> nw=4 q_lds=1 merge_par=1"),    # 64 x ceil(5 / 4) = 128 workgroups: 2 x 4
    ((3, 16, 70), "attn_dma_kernel<{T},4,128,768> nw=3 q_lds=1 merge_par=1"),     # B H = 48 > 32, too few tiles for either: 4 x 3, 12 waves
    ((1, 32, 640), "attn_dma_kernel<{T},4,128,512> nw=2 q_lds=1 merge_par=1"),    # 20 query tiles: still 4 x 2
    ((1, 32, 641), "attn_dma_kernel<{T},2,128,512> nw=4 q_lds=1 merge_par=1"),    # 21: 32 x ceil(21 / 4) = 192 workgroups: 2 x 4
]


@pytest.mark.parametrize("bhs,name", AUTO, ids=["x".join(map(str, c[0])) for c in AUTO])
def test_dma128_automatic_rule(hip, bhs, name):
    B, H, S = bhs
    for dtype in (BF16, F16):
        AC.run_case(hip, Shape(B, H, S, S, 128, True), dtype, {"attn_dma": 1}, name.format(T=AC.TNAME[dtype]), planted=False)


@pytest.mark.parametrize("dtype", DT16)
@pytest.mark.parametrize("S", [33, 129, 257])
def test_resident128(hip, S, dtype):
    """attn_dma = 0: the register-staged kernel, four key-split waves per query tile"""
    name = f"attn_resident_kernel<{AC.TNAME[dtype]},128,128,4> nw={ {33: 2, 129: 3, 257: 3}[S]}"   # 96 queries per workgroup, clipped to the tiles there are
    run_all(hip, [(s, dtype, {"attn_dma": 0}, name) for s in [Shape(2, 2, S, S, 128, True), Shape(2, 2, S, S, 128, True, (S, 32))]])


# ---- C ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT16)
@pytest.mark.parametrize("dma", [1, 0])
def test_dim88_windows(hip, dma, dtype):
    name = f"attn_dma88_kernel<{AC.TNAME[dtype]}>" if dma else f"attn_resident_kernel<{AC.TNAME[dtype]},96,288>"
    run_all(hip, [(s, dtype, {"attn_dma": dma}, name) for s in AC.C_WINDOW])


@pytest.mark.parametrize("dtype", DT16)
@pytest.mark.parametrize("shapes,nw", [(AC.C_TEMPORAL, 1), (AC.C_FALL, 3)], ids=["temporal", "fall_through"])
def test_dim88_tile_kernels(hip, shapes, nw, dtype):
    """Sq <= 32: the temporal kernel, one wave; a causal mask or Skv > 288 falls through to three waves"""
    assert all((s.Sq <= 32) == (nw == 1) for s in shapes)
    run_all(hip, [(s, dtype, {}, f"attn_mfma_kernel<{AC.TNAME[dtype]},96,{nw}>") for s in shapes])


# ---- D ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT16)
def test_dim64(hip, dtype):
    run_all(hip, [(s, dtype, {}, f"attn_mfma_kernel<{AC.TNAME[dtype]},64,{1 if s.Sq <= 32 else 2}>") for s in AC.D_SHAPES])


# ---- E ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def f32_shapes(D, Sq):
    out = [Shape(2, 2, Sq, 129, D, False), Shape(2, 2, Sq, 129, D, False, (129, 1))]
    if D == 128:
        out += [Shape(2, 2, Sq, Sq, D, True)] + ([Shape(2, 2, Sq, Sq, D, True, (Sq, 1))] if Sq > 1 else [])
    return out


@pytest.mark.parametrize("D", [64, 88, 128])
@pytest.mark.parametrize("mfma", [1, 0])
def test_fp32(hip, mfma, D):
    # the matrix-core kernel from 8 query rows on, one wave per 32 rows up to three; head_dim 88 runs padded to 96
    waves = {1: None, 7: None, 8: 1, 32: 1, 33: 2, 64: 2, 65: 3}
    name = {Sq: f"attn_mfma_f32_kernel<{ {64: 64, 88: 96, 128: 128}[D]},{nw}>" if mfma and nw else "attn_f32_kernel" for Sq, nw in waves.items()}
    run_all(hip, [(s, F32, {"attn_f32_mfma": mfma}, name[Sq]) for Sq in waves for s in f32_shapes(D, Sq)])


def test_fp32_vector_kernel_refuses_long_rows(hip):
    """the vector kernel keeps a row's scores in the LDS: Skv = 2049 is the library's shape error, nothing is launched, the output is untouched"""
    AC.run_case(hip, Shape(1, 1, 8, 129, 128, False), F32, {"attn_f32_mfma": 0}, "attn_f32_kernel")
    inp = AC.inputs(Shape(1, 1, 8, 2049, 128, False), F32)
    bufs, _ = inp.on("cuda")
    q, kv = bufs[0].view(-1, 128), bufs[1].view(-1, 256)
    g = _poison.Guarded(8, 128, F32, device="cuda")
    hip.set_option("attn_f32_mfma", 0)
    try:
        with pytest.raises(RuntimeError, match=r"stllm_attention\(fp32, vector kernel\): Skv 2049 > 2048"):
            hip.attention(q, kv[:, :128], kv[:, 128:], B=1, H=1, Sq=8, Skv=2049, D=128, scale=inp.scale, out=g.out)
    finally:
        hip.set_option("attn_f32_mfma", 1)
    torch.cuda.synchronize()
    assert AC.last_kernel(hip) == "attn_f32_kernel"   # still the launch before it
    assert g.intact() and bool((g.raw == 0xFF).all()), "a refused call wrote to its output"
