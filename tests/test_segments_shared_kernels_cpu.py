"""CPU: stllm_attention_segments_shared on the host emulator of the real sources (tests/hipemu) — the kernel case and the bit contract of
tests/_segments_shared_case.py, what the entry rejects, the table guard — and the C ABI surface."""
import os
import re

import pytest
import torch

import _hipemu
import _poison
import _segments_shared_case as SSC

torch.set_grad_enabled(False)
needs_emu = pytest.mark.skipif(not _hipemu.available() or _hipemu.ON_DEVICE, reason="ROCm clang++ not found: cannot build the emulated kernels")


@needs_emu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_emulated_attention_segments_shared(dtype):
    """every packed row against fp64 of the same inputs, no NaN although the rows behind P, behind every suffix, all of slot 3 and the q rows behind T are
    NaN, the 8 out rows behind T bit-unchanged, base and slots only read, a poisoned workspace, the same bits twice"""
    case = SSC.SharedSegmentCase(dtype)
    assert case.T == 89 and case.R == 5 and case.max_sfx == 60 and min(case.planted_weights) > 0.9
    with _hipemu.emulated() as hip:
        with _poison.poisoned_allocations() as counts:   # the record workspace starts as 0xFF in every byte
            got = case.run(hip, out=case.out_buffer())
            again = case.run(hip, out=case.out_buffer())
        assert hip.lib().stllm_last_kernel().decode() == "attn_segments_shared"
        if dtype != torch.float32:
            assert counts.refills >= 2, "the 16-bit path takes its workspace from the scratch cache"
        assert _poison.bits_equal(got, again), "the same call twice gives the same bits"
        assert case.unchanged(), "base and slots are read-only"
        case.check(got)


@needs_emu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_emulated_bit_contract_with_attention_shared(dtype):
    """3 segments of n = 9 behind sfx_off = 20, slots 0 .. 2: the bits of stllm_attention_shared(B = 3, G = 1, Sq = 9, causal, sfx_q_off = 20)"""
    with _hipemu.emulated() as hip:
        got, want = SSC.bit_contract(hip, dtype)
    assert _poison.bits_equal(got, want), dtype


@needs_emu
def test_emulated_rejections_and_bad_tables():
    """head_dim 64 and a bad dtype: an error with a message, never another kernel; a table of the wrong length raises in the wrapper; a slot out of range
    and a segment whose rows end behind T write nothing while the others are served"""
    case = SSC.SharedSegmentCase(torch.bfloat16)
    good = case.want.clone()
    with _hipemu.emulated() as hip:
        with pytest.raises(RuntimeError, match="unsupported"):
            case.run(hip, H=4, D=64)
        c = case.flat(case.cache)
        HD = case.HD
        out = case.out_buffer()
        p = lambda t: t.data_ptr()
        rc = hip.lib().stllm_attention_segments_shared(99, p(case.dense), 3 * HD, p(case.base[:, HD:]), 3 * HD, p(case.base[:, 2 * HD:]), 3 * HD, case.P,
                                                       p(c[:, HD:]), case.ML * 3 * HD, 3 * HD, p(c[:, 2 * HD:]), case.ML * 3 * HD, 3 * HD, p(out), HD,
                                                       case.R, case.H, 128, case.T, case.n_slots, case.max_n, case.max_sfx, 128 ** -0.5, p(case.slot),
                                                       p(case.row0), p(case.sfx_off), p(case.sfx_len), None, 0, None)   # dtype code 99: no such dtype
        assert rc != 0 and "unsupported" in hip.lib().stllm_last_error().decode() and _poison.bits_equal(out, case.out_buffer())
        keep = case.slot
        case.slot = case.slot[:4]
        with pytest.raises(RuntimeError, match="entries for R"):
            case.run(hip)
        case.slot = keep
        for name, r, bad in (("slot", 2, 6), ("slot", 2, -1), ("row0", 4, case.T - 3)):
            tab = getattr(case, name).clone()
            keep = tab.clone()
            tab[r] = bad
            setattr(case, name, tab)
            try:
                got = case.run(hip, out=case.out_buffer())
                lo, n = case.row0_h[r], case.n_h[r]
                pat = case.out_buffer()
                assert _poison.bits_equal(got[lo:lo + n], pat[lo:lo + n]) and _poison.bits_equal(got[case.T:], pat[case.T:]), (name, r, bad)
                live = torch.ones(case.T, dtype=torch.bool)
                live[lo:lo + n] = False
                err = float((got[:case.T][live].double() - good[live]).abs().max())
                assert err <= SSC.tol_of(torch.bfloat16) * float(good.abs().max()) and not torch.isnan(got.float()).any()
            finally:
                setattr(case, name, keep)


def test_contract_matches_the_shared_contract_on_identity_tables():
    """A sanity check of the TEST HELPER: the new contract against the shared-prefix contract of tests/_cpu_backend.py where both are defined (no project code)."""
    import _cpu_backend as CB
    both = type("Contracts", (), {"attention_segments_shared": staticmethod(SSC.attention_segments_shared), "attention_shared": staticmethod(CB.attention_shared)})
    got, want = SSC.bit_contract(both, torch.float32)
    assert torch.equal(got, want)


NEW_ENTRY_POINTS = ("stllm_attention_segments_shared", "stllm_attention_segments_shared_workspace_bytes")


def test_abi_declares_and_exports_the_shared_segment_entry_points():
    import ctypes
    from stllm_amd import hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "stllm_hip.h")).read()

    class _L:
        pass
    fake = _L()
    for n in hip.EXPORTS:
        setattr(fake, n, _L())
    hip._bind(fake)
    for name in NEW_ENTRY_POINTS:
        assert name in hip.EXPORTS
        decl = re.search(r"^int(?:64_t)? " + name + r"\(([^;]*?)\);", header, re.S | re.M).group(1)
        assert len(getattr(fake, name).argtypes) == len(decl.split(",")), name
    assert fake.stllm_attention_segments_shared_workspace_bytes.restype is ctypes.c_int64
    assert hip.segments_shared_available("cpu") is False
    if os.path.exists(hip.LIB_PATH):
        L = hip.lib()
        assert L.stllm_abi_version() == 7
        assert all(hasattr(L, n) for n in hip.EXPORTS)
        rec = 132 * 4   # bytes per record; the plans: ksplit_plan(1, 32, 55, 576) has 9 key ranges, ksplit_plan(16, 32, 40, 524) has 1
        assert L.stllm_attention_segments_shared_workspace_bytes(16, 32, 55, 576, 40, 524) == (32 * 55 * 9 + 16 * 32 * 40 * 1) * rec
        assert L.stllm_attention_segments_shared_workspace_bytes(4, 32, 8, 576, 0, 5) == -1
