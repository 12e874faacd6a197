"""CPU: poisoned-allocation runs (tests/_poison.py) of the packed segment step and the serving loop on the test-only contract backend: every path runs
twice clean (A, B) and once with every torch.empty & co result, every hand-out of the persistent scratch and every released cache row filled with 0xFF
(P).  On the DEFINED outputs: A == B and P == A bit for bit, P finite, poison count > 0."""
import pytest
import torch

import _poison
import _segments_case as SC
from _util import T, small_llama

torch.set_grad_enabled(False)


def abp(run, what):
    a, b = run(), run()
    with _poison.poisoned_allocations() as counts:
        p = run()
    print(f"{what}: {counts}")
    _poison.compare(a, b, p, counts, what)
    return counts


@pytest.fixture(scope="module")
def small():
    return small_llama(SC.SMALL, lm_head_spread=6.0)


def _live(cache):
    D = cache.hidden
    return [[buf[b, :n, D:].clone() for b, n in enumerate(cache.row_lens())] for buf in cache.qkv]


def test_step_segments(small):
    """load_row into three slots, one packed step (1, 9 and 1 tokens, one slot empty, one unnamed), then a decode step on the now ragged slots"""
    from stllm_amd import runtime
    emb = T("seg.emb", (4, 40, 256), 0.05)

    def run():
        h32, h16, cache, _ = SC.segment_step(small, emb, 48, "cpu")
        _, h = small.model.decode_step(emb[:, 36:37], cache)
        return dict(hidden=h32.clone(), logits=small.logits_from(h16, 3, 1)[:, 0].float().clone(), after=h.float().clone(), cache=_live(cache))
    with SC.installed(), runtime.use_dtype("fp32"):
        counts = abp(run, "load_row + step_segments + decode_step")
    assert counts.allocations >= 3, "the slot cache, the packed scratch and the attention output"


def test_engine_run(small):
    """5 requests over 2 slots with a shared video prefix: admissions into released (re-poisoned) slots, decode steps with a free slot riding along"""
    from stllm_amd import runtime
    lm = small.model
    prompts = [T(f"seg.req{i}.{s}", (n, 256), 0.05) for i, (n, s) in enumerate(zip(SC.REQ_PROMPTS, [0, 2, 4, 7, 0]))]
    video = T("seg.req.video.0", (11, 256), 0.05)

    def run():
        prefix = lm.new_cache(1, 11, "cpu")
        lm.prefill(video[None], None, cache=prefix)
        got, eng = SC.serve(small, prompts, 2, 40, prefix=prefix, do_sample=False, min_length=1, eos_token_id=None)
        assert eng.steps["segments"] >= 3 and eng.steps["decode"] >= 1
        return dict(ids=got, prefix=_live(prefix))
    with SC.installed(), runtime.use_dtype("fp32"):
        counts = abp(run, "Engine.run: 5 requests, 2 slots, shared prefix")
    assert counts.refills >= 5, "every released slot is undefined again"
