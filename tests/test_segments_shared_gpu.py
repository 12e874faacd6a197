"""GPU (-m gpu): stllm_attention_segments_shared on the device — the kernel case and the bit contract of tests/_segments_shared_case.py (the three launches of
the 16-bit path, the fp32 vector kernel)."""
import pytest
import torch

import _poison
import _segments_shared_case as SSC

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


@pytest.fixture(scope="module")
def hip():
    from stllm_amd import hip as h
    h.lib()
    return h


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_attention_segments_shared_on_device(hip, dtype):
    """tests/test_segments_shared_kernels_cpu.py::test_emulated_attention_segments_shared on the device: every packed row against fp64, no NaN although the
    rows behind P, behind every suffix, all of slot 3 and the q rows behind T are NaN, the 8 out rows behind T unchanged, a poisoned workspace, base and
    slots unchanged, the same bits twice"""
    case = SSC.SharedSegmentCase(DT[dtype])
    assert case.T == 89 and case.max_sfx == 60 and min(case.planted_weights) > 0.9
    case.to("cuda")
    with _poison.poisoned_allocations() as counts:
        got = case.run(hip, out=case.out_buffer())
        again = case.run(hip, out=case.out_buffer())
    torch.cuda.synchronize()
    assert hip.lib().stllm_last_kernel().decode() == "attn_segments_shared"
    if dtype != "fp32":
        assert counts.refills >= 2, "the 16-bit path takes its workspace from the scratch cache"
    assert _poison.bits_equal(got, again), "the same call twice gives the same bits"
    assert case.unchanged(), "base and slots are read-only for the attention"
    case.check(got, "on the device")


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_bit_contract_with_attention_shared_on_device(hip, dtype):
    """3 segments of n = 9 behind sfx_off = 20, slots 0 .. 2: the bits of stllm_attention_shared(B = 3, G = 1, Sq = 9, causal, sfx_q_off = 20)"""
    got, want = SSC.bit_contract(hip, DT[dtype], "cuda")
    assert _poison.bits_equal(got, want), dtype
