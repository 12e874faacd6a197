"""CPU: serving.Engine(num_beams > 1) on the contract backend (tests/_engine_beams_case.installed: the contracts of stllm_kv_reorder_rows
and stllm_beam_candidates_rows over those of the segment steps), fp32, the SMALL model: every request's ids equal generate(num_beams=nb) of that request
alone in both states, under the near-tie guard; the launches of a step; what is not served; Engine(num_beams=1) launches what it launched before;
Chat.answer_queue(num_beams=5) against Chat.answer; a poisoned-allocation run."""
import numpy as np
import pytest
import torch

import _cpu_backend as CB
import _engine_beams_case as BC
import _poison
from _util import T, small_llama
from test_segments_cpu import LAYER, stllm  # noqa: F401  (stllm: the chat fixture)

torch.set_grad_enabled(False)
SMALL = BC.SC.SMALL


@pytest.fixture(scope="module")
def model():
    return small_llama(SMALL, lm_head_spread=6.0)


def _fp32():
    from stllm_amd import runtime
    return runtime.use_dtype("fp32")


# ---- 1. ids ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["none", "prefix", "base"])
@pytest.mark.parametrize("nb", [3, 5])
def test_beam_engine_gives_every_request_the_ids_of_generate_alone(model, nb, mode):
    """five requests of different prompt lengths and max_new_tokens over 2 slots, with an EOS that the beams emit mid-way: hypotheses finish early, and
    is_done ends at least one request before its budget while another runs to its limit (asserted in check_engine, for generate() and for the Engine)"""
    with BC.installed(), _fp32():
        BC.check_engine(model, "small", nb, mode, "cpu")


def test_beam_engine_with_repetition_and_length_penalty(model):
    with BC.installed(), _fp32():
        BC.check_engine(model, "small", 3, "none", "cpu", extra=dict(repetition_penalty=1.3, length_penalty=2.0, min_length=2))


def test_beam_engine_with_a_stop_sequence(model):
    """two ids of request 0's free run and one of request 3's as stop sequences: the first beam that ends in one closes its request, the open beams become
    hypotheses"""
    with BC.installed(), _fp32():
        prompts = BC.requests("small", 3, 256)
        free, _ = BC.alone(model, prompts, 3, do_sample=False, min_length=1, eos_token_id=BC.SEEDS["small"][(3, False)][1])
        stop = [free[0][2:4].clone(), free[3][1:2].clone()]
        out, want = BC.check_engine(model, "small", 3, "none", "cpu", extra=dict(stop_sequences=stop))
        assert any(w.numel() < f.numel() for w, f in zip(want, free)), "a stop sequence cut a run short"


def test_poisoned_allocations_do_not_change_the_beam_engine_ids(model):
    with BC.installed(), _fp32():
        clean, _ = BC.check_engine(model, "small", 3, "prefix", "cpu")
        dirty, _ = BC.check_engine(model, "small", 3, "prefix", "cpu", poisoned=True)
    assert _poison.bits_equal(clean, dirty)


# ---- 2. launches -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", ["host", "device"])
def test_launches_of_a_beam_step(model, state):
    """one kv_reorder_rows per layer and step at the most, none in a step whose tables are all the identity (the host knows them); one
    beam_candidates_rows per step in the device state and none in the host state; one read of the candidate buffer per device step"""
    from stllm_amd import generation, serving
    nb, layers = 3, SMALL["num_hidden_layers"]
    k = dict(do_sample=False, min_length=1, eos_token_id=None)
    with BC.installed(), _fp32():
        prompts = BC.requests("small", nb, 256)
        # the expectation comes from OUTSIDE the Engine: the beam indices that generate() of every request alone hands to its own re-order
        # (_CacheStepper.advance), step by step — chosen[i][t]: the beams that request i's step t continues
        chosen, advance = [], generation._CacheStepper.advance

        def spy(self, next_tokens, beam_idx=None, on_device=False):
            chosen[-1].append(beam_idx.tolist())
            return advance(self, next_tokens, beam_idx, on_device=on_device)
        generation._CacheStepper.advance = spy
        try:
            for p, n in zip(prompts, BC.REQ_MAX_NEW):
                chosen.append([])
                model.generate(inputs_embeds=p[None], max_new_tokens=n, num_beams=nb, selection="device" if state == "device" else "torch", **k)
        finally:
            generation._CacheStepper.advance = advance
        assert [len(c) for c in chosen] == [n - 1 for n in BC.REQ_MAX_NEW]
        eng = serving.Engine(model, 2, BC.MAX_LEN, num_beams=nb, state=state, **k)
        index_of = {eng.submit(p, max_new_tokens=n): i for i, (p, n) in enumerate(zip(prompts, BC.REQ_MAX_NEW))}
        reads, read = [], eng._read_candidates
        eng._read_candidates = lambda buf: (reads.append(1), read(buf))[1]
        moved = idle = 0
        done = [0] * len(prompts)                    # steps that request i has behind it (counted here, from what step() returns and whom it serves)
        while not eng.idle():
            # a request that is in a slot when the step begins has `done` >= 1 steps behind it: behind its admission (done == 1) its rows are fanned out, later
            # they move iff the beams that its last step chose are not 0 .. nb - 1 in order
            live = [index_of[r.handle] for r in eng.running.values()]
            expect = any(done[i] == 1 or chosen[i][done[i] - 1] != list(range(nb)) for i in live)
            queued = [index_of[r.handle] for r in eng.queue]
            reads.clear()
            with BC.counting() as calls:
                eng.step()
                still = {index_of[r.handle] for r in eng.queue}
                for i in live + [i for i in queued if i not in still]:     # served by this step: who was in a slot, and who was admitted
                    done[i] += 1
                assert calls.count("kv_reorder_rows") == (layers if expect else 0), (expect, calls)
                assert calls.count("beam_candidates_rows") == (1 if state == "device" else 0)
                assert len(reads) == (1 if state == "device" else 0)
                assert ("attention_segments" in calls) != ("kv_append_rows" in calls), "one decoder pass: a segment step or a decode step"
            moved, idle = moved + expect, idle + (not expect)
        assert moved >= 3 and idle >= 1, (moved, idle, "both a step that re-orders and one whose tables are the identity ran")
        assert eng.steps["segments"] >= 3 and eng.steps["decode"] >= 1


def test_engine_with_one_beam_launches_what_it_launched_before(model):
    """Engine(num_beams=1): the call lists of tests/test_segments_cpu.py::test_engine_call_lists_and_slot_bookkeeping, and neither new entry point"""
    from stllm_amd import serving
    lm = model.model
    prompts = BC.SC.REQ_PROMPTS
    reqs = [T(f"seg.req{i}.0", (n, 256), 0.05) for i, n in enumerate(prompts)]
    with BC.installed(), _fp32():
        eng = serving.Engine(model, 2, 40, num_beams=1, do_sample=False, min_length=1, eos_token_id=None, max_new_tokens=4)
        eng.submit(reqs[0])
        with BC.counting() as calls:
            assert eng.step() == []
            assert calls == ["gather_rows", "gather_rows"] + LAYER * 2 + ["gather_rows", "rmsnorm", "gemm"], calls
        ref = lm.new_cache(2, 40, "cpu")
        ref.set_lens([5, 0])
        with BC.counting() as want_calls:
            lm.decode_step(lm.embed_tokens(torch.tensor([[5], [0]])), ref)
            want_calls = list(want_calls)
        with BC.counting() as calls:
            assert eng.step() == []
            assert calls == want_calls + ["gemm"], (calls, want_calls)
        eng.submit(reqs[1], max_new_tokens=2)
        with BC.counting() as calls:
            eng.run()
            assert "kv_reorder_rows" not in calls and "beam_candidates_rows" not in calls
        assert eng.cache.batch == 2 and eng.cache.row_lens() == [0, 0]


# ---- 3. what is not served ---------------------------------------------------------------------------------------------------------------------------
def test_what_stays_unserved_raises_and_names_the_alternative(model):
    from stllm_amd import serving

    class Never:
        def __call__(self, ids, scores):
            return False
    with BC.installed(), _fp32():
        with pytest.raises(NotImplementedError, match="num_beams=1"):
            serving.Engine(model, 2, 40, num_beams=3, do_sample=True)
        with pytest.raises(NotImplementedError, match="stop_sequences, or state='host'"):
            serving.Engine(model, 2, 40, num_beams=3, state="device", stopping_criteria=[Never()])
        with pytest.raises(NotImplementedError, match="16"):
            serving.Engine(model, 1, 40, num_beams=17)
        eng = serving.Engine(model, 2, 40, num_beams=3, stopping_criteria=[Never()])     # the host state serves them
        with pytest.raises(ValueError, match="positions"):
            eng.submit(T("beams.long", (38, 256), 0.05), max_new_tokens=4)               # one row's positions: prompt + max_new_tokens - 1
        eng.submit(T("beams.long", (37, 256), 0.05), max_new_tokens=4)
        # the device state: a budget whose history does not fit the LDS next to a logits row is refused when it is submitted, not by a launch in run()
        from stllm_amd import hip
        V = model.vocab_size
        fits = hip.SEL_LDS_BYTES // 4 - V
        assert hip.beam_rows_fit(V, fits) and not hip.beam_rows_fit(V, fits + 1)
        dev = serving.Engine(model, 2, 40, num_beams=3, state="device")
        with pytest.raises(ValueError, match="LDS.*state='host'"):
            dev.submit(T("beams.long", (4, 256), 0.05), max_new_tokens=fits + 1)
        assert dev.idle() and dev.ld_hist < fits
        with pytest.raises(ValueError, match="positions"):                               # the host state has no such limit: the positions decide
            eng.submit(T("beams.long", (4, 256), 0.05), max_new_tokens=fits + 1)
    with CB.installed(), _fp32(), pytest.raises(NotImplementedError, match="kv_reorder_rows"):   # a backend without the two entry points
        serving.Engine(model, 2, 40, num_beams=3)


# ---- 4. Chat.answer_queue ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("share", [False, True])
def test_chat_answer_queue_with_five_beams_equals_answer_per_question(stllm, share):
    """three questions over two slots behind a prefilled video, num_beams = 5: Chat.answer(num_beams=5)'s (text, ids) per question; with share_prefix the
    video is the Engine's base"""
    import _ragged_extend_case as RC
    from stllm_amd.conversation import Chat
    frames = T("input.frames2", (2, 3, 224, 224))
    k = dict(max_new_tokens=4, num_beams=5)
    with BC.installed(), _fp32():
        chat = Chat(stllm, device="cpu")
        img_list = []
        chat.upload_video(frames.view(6, 224, 224), None, img_list)
        prefix = chat.prefill_video(img_list)
        want = [chat.answer(img_list, q, **k) for q in RC.CHAT_QUESTIONS]
        with BC.counting() as calls:
            got = chat.answer_queue(img_list, RC.CHAT_QUESTIONS, slots=2, prefix=prefix, share_prefix=share, **k)
            assert calls.count("kv_reorder_rows") >= 2 and calls.count("attention_segments_shared" if share else "attention_segments") >= 2 * 2
        assert len(got) == 3
        for (t0, i0), (t1, i1) in zip(want, got):
            assert np.array_equal(i0, i1) and t0 == t1
        if share:   # state= reaches the Engine: one question through the device state
            dev = chat.answer_queue(img_list, RC.CHAT_QUESTIONS[:1], slots=2, prefix=prefix, share_prefix=share, state="device", **k)
            t0, i0 = chat.answer(img_list, RC.CHAT_QUESTIONS[0], selection="device", **k)
            assert np.array_equal(i0, dev[0][1]) and t0 == dev[0][0]
