"""CPU: the generate host path (generation.py, STLLMForCausalLM.generate, Chat.answer / answer_many) makes the calls of LlamaModel.prefill / extend /
decode_step and logits_from that it made before the prompt-cache setup was written once and the options became one object — same order, same shapes,
same lengths, same caches.  The recorded trace (tests/golden/generate_trace.json) was written by tests/golden/make_generate_trace.py on the commit before
that change; the recorder is replayed here.  Plus the one behaviour that changed on purpose: batching="groups" passes stop_sequences / return_lengths on."""
import importlib.util
import json
import os

import pytest
import torch

import _cpu_backend as CB
from _util import GOLDEN, T
from test_ragged_cpu import CFG, _build

torch.set_grad_enabled(False)
_spec = importlib.util.spec_from_file_location("make_generate_trace", os.path.join(GOLDEN, "make_generate_trace.py"))
MT = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MT)

with open(MT.OUT) as _f:
    WANT = json.load(_f)["cases"]


@pytest.fixture(scope="module")
def stllm():
    m = _build(CFG)
    m.lm_head.weight.mul_(6.0)   # what the recorder does: spread the logits so that the rows take different paths
    return m


@pytest.fixture(scope="module")
def got(stllm):
    return json.loads(MT.dumps(MT.record(stllm)))["cases"]   # through JSON, as the recorded trace went


def test_the_recorded_cases_are_the_cases_of_the_recorder(got):
    assert list(got) == list(WANT) and len(WANT) == 49


@pytest.mark.parametrize("case", list(WANT))
def test_generate_makes_the_recorded_calls(got, case):
    have, want = got[case], WANT[case]
    for i, (h, w) in enumerate(zip(have, want)):
        assert h == w, f"{case}: entry {i} differs"
    assert len(have) == len(want), f"{case}: {len(have)} entries, recorded {len(want)}"


@pytest.mark.parametrize("side", ["right", "left"])
def test_length_groups_stop_rows_one_by_one_and_return_their_lengths(stllm, side):
    """batching="groups" on a mixed-length padded batch with stop_sequences: every row stops where it stops when generated alone, return_lengths gives
    the per-row counts in row order, and the ids are those of per-row generation, padded with pad_token_id"""
    from stllm_amd import runtime
    model = stllm
    prompts = [T(f"gtrace.prompt{i}", (n, 4096), 0.05) for i, n in enumerate(MT.LENS)]
    emb, mask = MT.padded(prompts, side)
    k = dict(max_new_tokens=8, min_length=1)
    with CB.installed(), runtime.use_dtype("fp32"):
        free = [model.generate(inputs_embeds=p[None], **k)[0].tolist() for p in prompts]
        # a token that ends one row several steps before the others end
        pick = next(((r, t) for r, ids in enumerate(free) for t in range(1, 4) if ids[t] not in ids[:t]
                     and all(ids[t] not in o[:t + 4] for j, o in enumerate(free) if j != r)), None)
        assert pick is not None, ("no token separates the rows early enough", free)
        r, t = pick
        stops = [torch.tensor([free[r][t]])]
        alone = [model.generate(inputs_embeds=p[None], stop_sequences=stops, return_lengths=True, **k) for p in prompts]
        ids, lengths = model.generate(inputs_embeds=emb, attention_mask=mask, stop_sequences=stops, return_lengths=True, **k)
        bare = model.generate(inputs_embeds=emb, attention_mask=mask, stop_sequences=stops, **k)
    want = [n[0] for _, n in alone]
    assert lengths == want and lengths[r] == t + 1 and max(lengths) >= lengths[r] + 3, (pick, lengths, want)
    assert ids.shape == (len(prompts), max(want)) and torch.equal(bare, ids)
    for b, (a, _) in enumerate(alone):
        assert ids[b, : want[b]].tolist() == a[0, : want[b]].tolist(), (side, b)
        assert (ids[b, want[b]:] == 0).all()
