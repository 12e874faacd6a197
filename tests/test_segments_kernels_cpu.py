"""CPU: stllm_attention_segments / stllm_kv_append_segments on the host emulator of the real sources (tests/hipemu), the case of tests/_segments_case.py;
the two contracts of that file against the ragged-extend contracts; the C ABI surface."""
import os
import re

import pytest
import torch

import _hipemu
import _poison
import _ragged_extend_case as RC
import _segments_case as SC

torch.set_grad_enabled(False)
needs_emu = pytest.mark.skipif(not _hipemu.available() or _hipemu.ON_DEVICE, reason="ROCm clang++ not found: cannot build the emulated kernels")


@needs_emu
@pytest.mark.parametrize("dtype,opts", [(torch.bfloat16, (0, 1, -1)), (torch.float16, (0, 1, -1)), (torch.float32, (-1,))])
def test_emulated_attention_segments(dtype, opts):
    """every packed row against fp64 of the same inputs, no NaN although every row a pad lane could reach is NaN, the 8 rows behind T and the cache
    bit-unchanged, the kernel that was forced (and the rule's own choice), the same bits twice"""
    case = SC.SegmentCase(dtype)
    assert case.T == 89 and case.R == 5 and case.dominating_weight > 0.9
    with _hipemu.emulated() as hip:
        try:
            for opt in opts:
                hip.set_option("attn_ksplit", opt)
                with _poison.poisoned_allocations() as counts:   # the key-split workspace starts as 0xFF in every byte
                    got = case.run(hip, out=case.out_buffer())
                    again = case.run(hip, out=case.out_buffer())
                ran = hip.lib().stllm_last_kernel().decode()
                if dtype == torch.float32:
                    assert ran == "attn_f32_kernel"
                else:
                    assert ("ksplit" in ran) == (opt != 0), (ran, opt)   # the rule: 5 x 2 x 2 query tiles, 240 keys -> the key-split pair
                    assert counts.allocations >= 1
                assert _poison.bits_equal(got, again), "the same call twice gives the same bits"
                assert _poison.bits_equal(case.cache, case.before), "the cache is read-only"
                case.check(got, f"attn_ksplit={opt} ({ran})")
        finally:
            hip.set_option("attn_ksplit", -1)


@needs_emu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_emulated_identity_tables_equal_the_ragged_entry_bit_for_bit(dtype):
    """slot[r] = r, row0[r] = r * Sq, every n_r = Sq, T = R * Sq: the output of stllm_attention_offset_ragged, under both forced settings"""
    q_off, Sq = [170, 33, 200], 40
    rc = RC.KernelCase(dtype, q_off=q_off, n_new=[Sq] * 3, poison=False)
    HD, f = rc.HD, rc.flat(rc.cache)
    st = (rc.ML * 3 * HD, 3 * HD)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32)
    with _hipemu.emulated() as hip:
        try:
            for opt in ((0, 1) if dtype != torch.float32 else (-1,)):
                hip.set_option("attn_ksplit", opt)
                want = rc.run(hip)
                ran = hip.lib().stllm_last_kernel().decode()
                got = hip.attention_segments(rc.dense[:, :HD], f[:, HD:2 * HD], f[:, 2 * HD:], i32([0, 1, 2]), i32([0, Sq, 2 * Sq]), rc.q_off, rc.kv_len, H=rc.H,
                                             D=128, T=3 * Sq, n_slots=3, max_n=Sq, max_kv=rc.max_kv, scale=128 ** -0.5, k_strides=st, v_strides=st)
                assert ran == hip.lib().stllm_last_kernel().decode()
                assert _poison.bits_equal(got, want), (dtype, opt, ran)
        finally:
            hip.set_option("attn_ksplit", -1)


@needs_emu
def test_emulated_bad_tables_write_nothing():
    """a slot outside [0, n_slots), a negative first row and a segment that would end behind T: their rows of `out` keep the pattern, the good segment is served"""
    case = SC.SegmentCase(torch.bfloat16)
    good = case.want.clone()
    with _hipemu.emulated() as hip:
        for name, r, bad in (("slot", 2, 6), ("slot", 2, -1), ("row0", 0, -1), ("row0", 4, case.T - 3)):
            tab = getattr(case, name).clone()
            keep = tab.clone()
            tab[r] = bad
            setattr(case, name, tab)
            try:
                for opt in (0, 1):
                    hip.set_option("attn_ksplit", opt)
                    got = case.run(hip, out=case.out_buffer())
                    lo, n = case.row0_h[r], case.n_h[r]
                    pat = case.out_buffer()
                    assert _poison.bits_equal(got[lo:lo + n], pat[lo:lo + n]) and _poison.bits_equal(got[case.T:], pat[case.T:]), (name, r, bad, opt)
                    live = torch.ones(case.T, dtype=torch.bool)
                    live[lo:lo + n] = False
                    err = float((got[:case.T][live].double() - good[live]).abs().max())
                    assert err <= SC.tol_of(torch.bfloat16) * float(good.abs().max()) and not torch.isnan(got.float()).any()
            finally:
                hip.set_option("attn_ksplit", -1)
                setattr(case, name, keep)


@needs_emu
def test_emulated_attention_segments_rejects_what_it_does_not_serve():
    """head_dim 64, and fp32 beyond the vector kernel's 2048 keys: STLLM_ERR_UNSUPPORTED with a message, never another kernel"""
    q, c = SC.rnd(8, 3 * 128), SC.rnd(2 * 8, 3 * 128)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32)
    tabs = i32([0, 1]), i32([0, 4]), i32([3, 1]), i32([5, 4])
    with _hipemu.emulated() as hip:
        with pytest.raises(RuntimeError, match="unsupported"):
            hip.attention_segments(q[:, :128].bfloat16(), c[:, 128:256].bfloat16(), c[:, 256:].bfloat16(), *tabs, H=2, D=64, T=8, n_slots=2, max_n=4, max_kv=5,
                                   scale=1.0, k_strides=(8 * 384, 384), v_strides=(8 * 384, 384))
        with pytest.raises(RuntimeError, match="unsupported"):
            hip.attention_segments(q[:, :128], c[:, 128:256], c[:, 256:], *tabs, H=1, D=128, T=8, n_slots=2, max_n=4, max_kv=2049, scale=1.0,
                                   k_strides=(8 * 384, 384), v_strides=(8 * 384, 384))


@needs_emu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_emulated_kv_append_segments(dtype):
    """exact against the explicit loop; the q columns, the unnamed slot, the n = 0 segment, the segments with bad tables and the position at max_len
    untouched; the contract restates the same thing; identity tables give stllm_kv_append_spans' bits"""
    cache, src, tabs, T, max_n, want = SC.append_case(dtype)
    ref = cache.clone()
    with _hipemu.emulated() as hip:
        hip.kv_append_segments(src, cache, *tabs, T=T, max_n=max_n)
        assert _poison.bits_equal(cache, want)
        assert _poison.bits_equal(cache[1], ref[1]) and _poison.bits_equal(cache[2], ref[2]) and _poison.bits_equal(cache[:, :, :136], ref[:, :, :136])
        assert not _poison.bits_equal(cache[3], ref[3]) and not _poison.bits_equal(cache[0, 5:7], ref[0, 5:7])
        got = ref.clone()
        SC.kv_append_segments(src, got, *tabs, T=T, max_n=max_n)
        assert _poison.bits_equal(got, want)
        c0, s0, pos0, n, S, w0 = RC.append_case(dtype)
        c1 = c0.clone()
        hip.kv_append_spans(s0, c0, pos0, n, S=S)
        B = c1.shape[0]
        hip.kv_append_segments(s0, c1, torch.arange(B, dtype=torch.int32), torch.arange(B, dtype=torch.int32) * S, pos0, n, T=B * S, max_n=S)
        assert _poison.bits_equal(c0, w0) and _poison.bits_equal(c1, c0)


def test_contract_matches_the_ragged_contract_on_identity_tables():
    """A sanity check of the TEST HELPER: the new contract against the ragged-extend contract where both are defined (it runs no project code)."""
    rc = RC.KernelCase(torch.float32, poison=False)
    HD, f = rc.HD, rc.flat(rc.cache)
    st = (rc.ML * 3 * HD, 3 * HD)
    B, Sq = rc.B, rc.Sq
    want = RC.attention_offset_ragged(rc.dense[:, :HD], f[:, HD:2 * HD], f[:, 2 * HD:], rc.q_off, rc.kv_len, B=B, H=rc.H, Sq=Sq, max_kv=rc.max_kv, D=128,
                                      scale=128 ** -0.5, q_strides=(Sq * 3 * HD, 3 * HD), k_strides=st, v_strides=st)
    got = SC.attention_segments(rc.dense[:, :HD], f[:, HD:2 * HD], f[:, 2 * HD:], torch.arange(B, dtype=torch.int32), torch.arange(B, dtype=torch.int32) * Sq,
                                rc.q_off, rc.kv_len, H=rc.H, D=128, T=B * Sq, n_slots=B, max_n=Sq, max_kv=rc.max_kv, scale=128 ** -0.5, k_strides=st, v_strides=st)
    assert torch.equal(got, want)


NEW_ENTRY_POINTS = ("stllm_attention_segments", "stllm_attention_segments_workspace_bytes", "stllm_kv_append_segments")


def test_abi_declares_and_exports_the_segment_entry_points():
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
    assert fake.stllm_attention_segments_workspace_bytes.restype is ctypes.c_int64
    assert hip.segments_available("cpu") is False
    if os.path.exists(hip.LIB_PATH):
        L = hip.lib()
        assert L.stllm_abi_version() == 7
        assert all(hasattr(L, n) for n in hip.EXPORTS)
        assert L.stllm_attention_segments_workspace_bytes(16, 32, 40, 1100) == L.stllm_attention_offset_workspace_bytes(16, 32, 40, 1100) > 0
        assert L.stllm_attention_segments_workspace_bytes(4, 32, 0, 5) == -1
