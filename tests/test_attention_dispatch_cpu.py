"""CPU: the dispatch cases of tests/test_attention_dispatch_gpu.py (tests/_attention_case.py) through the host emulation of the same kernel sources
(tests/_hipemu.py), as test_emulated_forward_attention_matches_contract runs the workload's shapes — so that a configuration, its kernel name and its masks can
be checked without a GPU — and the fp64 sensitivity precondition of every planted input set of the device file (reference only, no kernel).
Tolerance: that test's 4 x TOL[dtype] x abs-max (bf16 2^-5, fp16 2^-8), 2e-5 for fp32."""
import pytest
import torch

import _attention_case as AC
import _hipemu
from _attention_case import Shape

pytestmark = [pytest.mark.skipif(not _hipemu.available(), reason="ROCm clang++ not found: cannot build the emulated kernels"),
              pytest.mark.skipif(_hipemu.ON_DEVICE, reason="emulator self-check")]
BF16, F32 = torch.bfloat16, torch.float32


def emulate(shape, dtype, opts, name, **sets):
    with _hipemu.emulated() as hip:
        return AC.run_case(hip, shape, dtype, opts, name, device="cpu", tol=AC.EMU_TOL[dtype], **sets)


# head_dim 128: 33 = one key more than a tile, 96 leaves the fourth key-split wave without a key tile, 129 opens the second window (with a padded batch row)
A_CPU = [Shape(2, 2, 33, 33, 128, True), Shape(2, 2, 96, 96, 128, True), Shape(2, 2, 129, 129, 128, True, (129, 33))]


@pytest.mark.parametrize("planted", [False, True], ids=["random", "planted"])
@pytest.mark.parametrize("q_lds", [1, 0])
@pytest.mark.parametrize("cfg", sorted(AC.DMA_CONFIGS))
@pytest.mark.parametrize("shape", A_CPU, ids=lambda s: s.id)
def test_emulated_dma128_forced(shape, cfg, q_lds, planted):
    ks2, tiles = AC.DMA_CONFIGS[cfg]
    ran = emulate(shape, BF16, {"attn_dma": cfg, "attn_q_lds": q_lds}, AC.dma_name(BF16, ks2, tiles, shape.Sq, q_lds), random=not planted, planted=planted)
    assert [i.planted for i in ran] == [planted]


@pytest.mark.parametrize("shape,opts,name", [
    (Shape(2, 2, 97, 97, 88, False), {"attn_dma": 1}, "attn_dma88_kernel<bf16_t>"),
    (Shape(2, 2, 97, 97, 88, False), {"attn_dma": 0}, "attn_resident_kernel<bf16_t,96,288>"),
    (Shape(2, 2, 16, 16, 88, False), {}, "attn_mfma_kernel<bf16_t,96,1>"),
    (Shape(2, 2, 33, 32, 64, False), {}, "attn_mfma_kernel<bf16_t,64,2>"),
    # the automatic rule and the register-staged kernel at one head (the other branches need B H > 32 or more than 20 query tiles: the device file)
    (Shape(1, 1, 70, 70, 128, True), {"attn_dma": 1}, "attn_dma_kernel<bf16_t,4,128,512> nw=2 q_lds=1 merge_par=1"),
    (Shape(1, 1, 33, 33, 128, True), {"attn_dma": 0}, "attn_resident_kernel<bf16_t,128,128,4> nw=2"),
], ids=lambda x: x.id if isinstance(x, Shape) else None)
def test_emulated_other_kernels(shape, opts, name):
    emulate(shape, BF16, opts, name)


@pytest.mark.parametrize("mfma,name", [(1, "attn_mfma_f32_kernel<128,1>"), (0, "attn_f32_kernel")])
def test_emulated_fp32(mfma, name):
    emulate(Shape(2, 2, 8, 129, 128, False, (129, 1)), F32, {"attn_f32_mfma": mfma}, name)
    emulate(Shape(2, 2, 8, 8, 128, True), F32, {"attn_f32_mfma": mfma}, name)


def test_planted_sets_are_sensitive():
    """every planted input set of the device file: moving a planted boundary by one key displaces the fp64 reference of the rows that see it by at least
    4 x the widest tolerance a comparison applies to it (the emulated one; the device's is 4 x tighter).  Inputs.__init__ asserts the device bound itself."""
    shapes = AC.planted_shapes()
    assert len(shapes) > 60
    worst = {}
    for s in shapes:
        for dtype in (torch.bfloat16, torch.float16):
            inp = AC.inputs(s, dtype, True)
            assert inp.sensitivity >= 4 * AC.EMU_TOL[dtype] and inp.sensitivity >= 4 * AC.tol_of(dtype), (s.id, dtype, inp.sensitivity)
            if inp.sensitivity < worst.get(dtype, (float("inf"),))[0]:
                worst[dtype] = (inp.sensitivity, s.id)
    print({str(k): v for k, v in worst.items()})
    # boundaries that do not exist are declared, never silently dropped: a shape without any runs the random set alone
    free = [s.id for s in AC.A_SHAPES + AC.C_WINDOW + AC.C_TEMPORAL + AC.C_FALL + AC.D_SHAPES if not AC.has_boundary(s)]
    assert free == ["B2H2D88-96x96", "B2H2D88-193x192", "B2H2D88-288x288", "B2H2D88-32x32", "B2H2D64-33x32"]   # no causal mask, no kv_len, Skv on a tile edge
