"""GPU (-m gpu): poisoned-allocation runs (tests/_poison.py) of the packed segment step and the serving loop on the device, bf16: twice clean (A, B), once
with every torch.empty & co result, every hand-out of the persistent scratch and every released cache row filled with 0xFF (P).  On the DEFINED outputs:
A == B and P == A bit for bit, P finite, poison count > 0."""
import pytest
import torch

import _poison
import _segments_case as SC
from _util import T

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def abp(run, what):
    a, b = run(), run()
    with _poison.poisoned_allocations() as counts:
        p = run()
    print(f"{what}: {counts}")
    _poison.compare(a, b, p, counts, what)
    return counts


@pytest.fixture(scope="module")
def llm():
    from stllm_amd import synth
    from stllm_amd.models.st_llm import STLLMForCausalLM, StllmConfig
    m = STLLMForCausalLM(StllmConfig(num_hidden_layers=2), device="cuda")
    synth.fill_module_(m, 0, "")
    m.lm_head.weight.mul_(6.0)
    return m


def _live(cache):
    D = cache.hidden
    return [[buf[b, :n, D:].clone() for b, n in enumerate(cache.row_lens())] for buf in cache.qkv]


def test_step_segments_on_device(llm):
    from stllm_amd import runtime
    emb = T("seg.wide", (4, 40, 4096), 0.05).cuda()

    def run():
        h32, h16, cache, _ = SC.segment_step(llm, emb, 48, "cuda")
        _, h = llm.model.decode_step(emb[:, 36:37], cache)
        return dict(hidden=h32.clone(), logits=llm.logits_from(h16, 3, 1)[:, 0].float().clone(), after=h.float().clone(), cache=_live(cache))
    with runtime.use_dtype("bf16"):
        counts = abp(run, "load_row + step_segments + decode_step, bf16")
    assert counts.allocations >= 3


def test_engine_run_on_device(llm):
    from stllm_amd import runtime
    lm = llm.model
    prompts = [T(f"seg.greq{i}.{s}", (n, 4096), 0.05).cuda() for i, (n, s) in enumerate(zip(SC.REQ_PROMPTS, [1, 0, 12, 2, 0]))]
    video = T("seg.greq.video.0", (11, 4096), 0.05).cuda()

    def run():
        prefix = lm.new_cache(1, 11, "cuda")
        lm.prefill(video[None], None, cache=prefix)
        got, eng = SC.serve(llm, prompts, 2, 40, prefix=prefix, do_sample=False, min_length=1, eos_token_id=None)
        assert eng.steps["segments"] >= 3 and eng.steps["decode"] >= 1
        return dict(ids=got, prefix=_live(prefix))
    with runtime.use_dtype("bf16"):
        counts = abp(run, "Engine.run: 5 requests, 2 slots, shared prefix, bf16")
    assert counts.refills >= 5
