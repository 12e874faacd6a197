"""GPU (-m gpu): serving.Engine(state="device") on the device — the Engine cases of tests/test_segments_gpu.py (the same vetted prompts, two slots, the
full-width two-layer decoder) with the selection state on the device: fp32 ids against generate() of every request alone and against the host-state Engine;
bf16 to completion through both kinds of step."""
import pytest
import torch

import _poison
import _segments_case as SC
from _util import T
from test_segments_gpu import WIDE_SEEDS, WIDE_VIDEO, _llm

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def llm():
    return _llm(spread=6.0)


@pytest.mark.parametrize("with_prefix", [False, True])
def test_device_state_gives_every_request_the_ids_of_generate_alone_on_device(llm, with_prefix):
    """fp32: 5 requests of different prompt lengths and max_new_tokens over 2 slots, greedy, with an EOS id that request 1 emits mid-way; with and without a
    shared video prefix.  The ids of generate() alone (whose margins are asserted) and of the host-state Engine."""
    from stllm_amd import hip, runtime
    model, lm = llm, llm.model
    prompts = [T(f"seg.greq{i}.{s}", (n, 4096), 0.05).cuda() for i, (n, s) in enumerate(zip(SC.REQ_PROMPTS, WIDE_SEEDS[with_prefix]))]
    video = T(WIDE_VIDEO[0], (WIDE_VIDEO[1], 4096), 0.05).cuda() if with_prefix else None
    k = dict(do_sample=False, min_length=0)
    with runtime.use_dtype("fp32"):
        free = SC.alone(model, prompts, video, eos_token_id=None, **k)
        k["eos_token_id"] = int(free[1][1])
        with SC.scored_runs() as scored:
            want = SC.alone(model, prompts, video, **k)
        print("from-scratch margins:", [f"{m:.4f}" for m in scored])
        assert min(scored) >= SC.MARGIN, ("precondition: the from-scratch runs are not near a tie", min(scored))
        assert want[1].tolist() == free[1][:2].tolist()
        prefix = None
        if with_prefix:
            prefix = lm.new_cache(1, WIDE_VIDEO[1], "cuda")
            lm.prefill(video[None], None, cache=prefix)
            before = [x.clone() for x in prefix.qkv]
        host, _ = SC.serve(model, prompts, 2, 40, prefix=prefix, **k)
        with _poison.poisoned_allocations():
            got, eng = SC.serve(model, prompts, 2, 40, prefix=prefix, state="device", **k)
        for i, (g, h, w) in enumerate(zip(got, host, want)):
            assert g.dtype == torch.long and g.tolist() == w.tolist() and g.tolist() == h.tolist(), (i, g.tolist(), h.tolist(), w.tolist())
        assert eng.steps["segments"] >= 3 and eng.steps["decode"] >= 1, eng.steps
        if with_prefix:
            assert all(_poison.bits_equal(x, y) for x, y in zip(prefix.qkv, before)), "the prefix is only read"
    assert hip.gemm_workspace_ok()


def test_device_state_bf16_runs_both_kinds_of_step(llm):
    """bf16 (the serving dtype): the same requests run to completion through admission and decode steps; the lengths are the budgets; ids are not compared (a
    16-bit near-tie may legitimately differ from the from-scratch run)"""
    from stllm_amd import runtime
    prompts = [T(f"seg.greq{i}.{s}", (n, 4096), 0.05).cuda() for i, (n, s) in enumerate(zip(SC.REQ_PROMPTS, WIDE_SEEDS[False]))]
    try:
        with runtime.use_dtype("bf16"), _poison.poisoned_allocations():
            llm.model.repack()
            llm._lm_packed = {}
            got, eng = SC.serve(llm, prompts, 2, 40, state="device", do_sample=False, min_length=1, eos_token_id=None)
        assert [g.numel() for g in got] == SC.REQ_MAX_NEW and eng.steps["segments"] >= 3 and eng.steps["decode"] >= 1
        assert all(bool(((g >= 0) & (g < llm.vocab_size)).all()) for g in got)
    finally:
        llm.model.repack()
        llm._lm_packed = {}
