"""CPU: the two kernels of continuous batching for beam search — stllm_kv_reorder_rows and stllm_beam_candidates_rows.

  1. ABI: the names are declared, exported, listed and bound; the ctypes structure mirrors the header name by name; the version stays 7.
  2. kv_reorder_rows_kernel and beam_kernel<true> of st-llm_amd/csrc/elementwise.hip compiled for the host (tests/hipemu) and called through hip.py, on the
     cases of tests/_engine_beams_case.py (tests/test_engine_beams_gpu.py runs the same functions on the device); the contracts that the Engine tests install
     against the emulated kernels."""
import os
import re

import pytest
import torch

import _engine_beams_case as BC
import _hipemu
import _poison

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
emu = pytest.mark.skipif(not _hipemu.available(), reason="ROCm clang++ not found: cannot build the emulated kernels")
DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


# ---- 1. ABI ----------------------------------------------------------------------------------------------------------------------------------------
def test_abi_declares_exports_and_binds_the_two_entry_points():
    from stllm_amd import hip
    header = open(os.path.join(ROOT, "include", "stllm_hip.h")).read()
    assert re.search(r"^int stllm_beam_candidates_rows\(const stllm_beam_rows_args\* args, void\* stream\);", header, re.M)
    assert re.search(r"^int stllm_kv_reorder_rows\(int dtype, void\* cache, int64_t batch_stride, int64_t row_stride, const int32_t\* src, const int32_t\* lo, "
                     r"const int32_t\* hi,\s+int rows, int nb, int hidden, int capacity, int max_span, void\* stream\);", header, re.M)
    for n in ("stllm_kv_reorder_rows", "stllm_beam_candidates_rows"):
        assert n in hip.EXPORTS
    assert callable(hip.kv_reorder_rows) and callable(hip.beam_candidates_rows) and hip.beam_rows_available("cpu") is False

    class _L:
        pass
    fake = _L()
    for n in hip.EXPORTS:
        setattr(fake, n, _L())
    hip._bind(fake)
    assert fake.stllm_beam_candidates_rows.argtypes[0]._type_ is hip.BeamRowsArgs and len(fake.stllm_beam_candidates_rows.argtypes) == 2
    assert len(fake.stllm_kv_reorder_rows.argtypes) == 13
    body = re.search(r"typedef struct stllm_beam_rows_args \{(.*?)\} stllm_beam_rows_args;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") if decl.strip() for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip().replace("*", " "))]
    assert names == [f[0] for f in hip.BeamRowsArgs._fields_], names
    if os.path.exists(hip.LIB_PATH):
        L = hip.lib()
        assert L.stllm_abi_version() == 7 and hasattr(L, "stllm_kv_reorder_rows") and hasattr(L, "stllm_beam_candidates_rows")


# ---- 2. the kernels, host-emulated ---------------------------------------------------------------------------------------------------------------------
@emu
@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("name", list(BC.REORDER_CASES))
def test_emulated_kv_reorder_rows(name, dtype):
    with _hipemu.emulated() as hip:
        moved = BC.check_reorder(hip, "cpu", DT[dtype], name)
    assert moved > 0, "every case moves something"


@emu
def test_emulated_kv_reorder_rows_refuses_17_rows_per_group():
    with _hipemu.emulated() as hip:
        BC.check_reorder_unsupported(hip, "cpu")


@emu
@pytest.mark.parametrize("name", list(BC.REORDER_CASES))
def test_reorder_contract_of_the_engine_tests_is_the_emulated_kernel(name):
    """the contract that the CPU Engine tests install (BC.kv_reorder_rows) against the PRODUCT: the emulated kv_reorder_rows_kernel on the same bytes, the
    whole allocation bit for bit — an Engine test that passes on the contract says something about the kernel only while the two agree"""
    nb, src, lo, hi = BC.REORDER_CASES[name]
    raw, _ = BC.reorder_buffers(torch.bfloat16, len(src), seed=3)
    span = max(1, max(min(h, BC.CAPACITY) - max(l, 0) for l, h in zip(lo, hi)))
    i32 = lambda x: torch.tensor(x, dtype=torch.int32)
    by_contract, by_kernel = raw.clone(), raw.clone()
    BC.kv_reorder_rows(by_contract[:, :BC.CAPACITY], i32(src), i32(lo), i32(hi), nb=nb, max_span=span)
    with _hipemu.emulated() as hip:
        hip.kv_reorder_rows(by_kernel[:, :BC.CAPACITY], i32(src), i32(lo), i32(hi), nb=nb, max_span=span)
    assert not _poison.bits_equal(by_kernel, raw), "the case moves something"
    assert _poison.bits_equal(by_contract, by_kernel)


@emu
@pytest.mark.parametrize("penalty", [1.0, 1.5])
@pytest.mark.parametrize("k", [6, 10])
@pytest.mark.parametrize("V", [1000, 32000])
def test_emulated_beam_candidates_rows(V, k, penalty):
    with _hipemu.emulated() as hip:
        cs, ct = BC.check_candidates(hip, "cpu", V, k, penalty)
    assert cs.shape == (6, k) and ct.shape == (6, k)


@emu
def test_emulated_candidates_row_that_does_not_fit_raises():
    """V + ld_prev floats must fit the LDS, whatever the rows hold"""
    V = 39500
    lg = torch.zeros(1, V)
    z = torch.zeros(1, dtype=torch.int32)
    cs, ct = torch.full((1, 4), 7.0), torch.full((1, 4), 7, dtype=torch.int32)
    with _hipemu.emulated() as hip:
        hip.beam_candidates_rows(lg, z, torch.zeros(1), 4, prev=torch.zeros((1, 8), dtype=torch.int32), n_prev=z, cand_score=cs, cand_token=ct)
        assert ct[0].tolist() == [0, 1, 2, 3]
        cs.fill_(7.0)
        with pytest.raises(RuntimeError, match="LDS"):
            hip.beam_candidates_rows(lg, z, torch.zeros(1), 4, prev=torch.zeros((1, 1024), dtype=torch.int32), n_prev=z, cand_score=cs, cand_token=ct)
        assert bool((cs == 7.0).all())
