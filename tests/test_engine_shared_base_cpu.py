"""CPU: the packed segment step on a shared base and serving.Engine(base=) on the test-only contract backend (tests/_cpu_backend.py plus the
contracts of tests/_segments_case.py and tests/_segments_shared_case.py, fp32): KVCache.release on a based cache, LlamaModel.step_segments on a cache with a
base against from-scratch prefills of [video, row], serving.Engine(base=) against generate() of every request alone with host and device state,
Chat.answer_queue(share_prefix=True) against Chat.answer.  Every cache is allocated under _poison.poisoned_allocations()."""
import contextlib

import numpy as np
import pytest
import torch

import _cpu_backend as CB
import _poison
import _segments_shared_case as SSC
import _select_ref as R
import _select_slots_ref as SR
from _util import T, small_llama

torch.set_grad_enabled(False)
SMALL = SSC.SMALL
LAYER = ["rmsnorm", "gemm", "kv_append_segments", "attention_segments_shared", "gemm", "rmsnorm", "gemm", "gemm"]
# the prompts and the video of tests/test_segments_cpu.py (copied): vetted there such that, with the video in front, the from-scratch run's top-1 / top-2
# margin is >= 1.8e-2 x max |score| at every generated step; the reference runs here are those runs, and the test asserts >= MARGIN itself
REQ_SEEDS, VIDEO = [0, 2, 4, 7, 0], ("seg.req.video.0", 11)


@contextlib.contextmanager
def _backend():
    from stllm_amd import runtime
    with SSC.installed(), CB._patched({"select_slots": SR.select_slots, "select_tokens": R.select_tokens}), runtime.use_dtype("fp32"):
        yield


def _requests(D=256):
    return [T(f"seg.req{i}.{s}", (n, D), 0.05) for i, (n, s) in enumerate(zip(SSC.REQ_PROMPTS, REQ_SEEDS))]


# ---- 1. KVCache.release, LlamaModel.step_segments on a cache with a base ---------------------------------------------------------------------------------
def test_step_segments_on_a_base_matches_from_scratch_prefills():
    """an 11-token video shared by 4 slots; a FIRST call admits 17, 33 and 5 tokens into slots 0, 2 and 3, a SECOND appends 1, 9 and 1 to slots 0, 1 and 2
    (slot 1 empty before): every row's last hidden state and suffix K / V against a from-scratch prefill of [video, row], slot 3 bit-unchanged by the
    second call, the base bit-unchanged; the call list of a step"""
    model = small_llama(SMALL)
    video, emb = T(VIDEO[0], (VIDEO[1], 256), 0.05), T("seg.emb", (4, 40, 256), 0.05)
    with _backend(), _poison.poisoned_allocations() as counts, SSC.counting() as calls:
        cache = SSC.check_two_calls(model, video, emb, "cpu", SSC.MODEL_TOL["fp32"], "fp32 contract")
        assert counts.allocations > 0
        assert "attention_segments_shared" in calls and "attention_segments" not in calls and "attention_shared" not in calls
        first = calls.index("kv_append_segments") - 4
        assert calls[first:first + 4 + 2 * len(LAYER)] == ["gather_rows", "gather_rows"] + LAYER * 2 + ["gather_rows", "rmsnorm"]
        # release: back to the base's length, through truncate (so the suffix is poison again)
        cache.release(2)
        assert cache.row_lens() == [11 + 18, 11 + 9, 11, 11 + 5]
        assert all(bool(torch.isnan(x[2, :34]).all()) and bool(torch.isfinite(x[0, :18, 256:]).all()) for x in cache.qkv), "slot 2's suffix is undefined again"
        for s in (0, 1, 3):
            cache.release(s)
        assert cache.lens is None and cache.len == 11 and cache.row_lens() == [11] * 4


def test_step_segments_on_a_base_error_paths():
    from stllm_amd import hip, runtime
    model = small_llama(SMALL)
    lm = model.model
    emb = T("seg.emb", (4, 40, 256), 0.05)
    with _backend():
        two = lm.new_cache(2, 12, "cpu")
        lm.prefill(emb[:2, :12], None, cache=two)
        with pytest.raises(NotImplementedError, match="one base row"):
            lm.step_segments(emb[0, :2], two.share(rows=2, max_new=4), [(0, 1), (1, 1)])
        one = lm.new_cache(1, 12, "cpu")
        lm.prefill(emb[:1, :12], None, cache=one)
        c = one.share(rows=2, max_new=4)
        with pytest.raises(AssertionError, match="KV cache full"):
            lm.step_segments(emb[0, :5], c, [(0, 5)])
        with pytest.raises(AssertionError, match="distinct"):
            lm.step_segments(emb[0, :2], c, [(0, 1), (0, 1)])
        assert c.row_lens() == [12, 12]
        with runtime.use_decode_weights("int8"), pytest.raises(NotImplementedError, match="decode_step"):
            lm.step_segments(emb[0, :2], c, [(0, 1), (1, 1)])
    with runtime.use_dtype("bf16x3"), pytest.raises(NotImplementedError, match="bf16x3"):
        lm.step_segments(emb[0, :2], c, [(0, 1), (1, 1)])
    assert hip.segments_shared_available("cpu") is False
    import _segments_case as SC
    with SC.installed(), runtime.use_dtype("fp32"), pytest.raises(NotImplementedError, match="attention_segments_shared"):
        lm.step_segments(emb[0, :2], c, [(0, 1), (1, 1)])


# ---- 2. serving.Engine(base=) ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", ["host", "device"])
def test_engine_on_a_base_gives_every_request_the_ids_of_generate_alone(state, monkeypatch):
    """5 requests of different prompt lengths and max_new_tokens over 2 slots behind ONE prefilled video, greedy, with an EOS id that request 1 emits mid-way:
    the ids of generate([video, prompt]) alone; both kinds of step; no load_row; idle slots at the video's length; the base only read"""
    from stllm_amd.models.llama import KVCache
    model = small_llama(SMALL, lm_head_spread=6.0)
    lm = model.model
    prompts = _requests()
    video = T(VIDEO[0], (VIDEO[1], 256), 0.05)
    k = dict(do_sample=False, min_length=0)
    loads = []
    load_row = KVCache.load_row
    monkeypatch.setattr(KVCache, "load_row", lambda self, *a, **kw: (loads.append(a), load_row(self, *a, **kw))[1])
    with _backend():
        free = SSC.alone(model, prompts, video, eos_token_id=None, **k)
        k["eos_token_id"] = int(free[1][1])          # request 1 (max_new_tokens = 3) ends on its second token
        with SSC.scored_runs() as scored:
            want = SSC.alone(model, prompts, video, **k)
        print("from-scratch margins:", [f"{m:.4f}" for m in scored])
        assert min(scored) >= SSC.MARGIN, ("precondition: the from-scratch runs are not near a tie", min(scored))
        assert want[1].tolist() == free[1][:2].tolist() and any(w.numel() == n for w, n in zip(want, SSC.REQ_MAX_NEW)), "one ends on EOS, one runs to its limit"
        with _poison.poisoned_allocations():
            prefix = lm.new_cache(1, VIDEO[1], "cpu")
            lm.prefill(video[None], None, cache=prefix)
            before = [x.clone() for x in prefix.qkv]
            with SSC.counting() as calls:
                got, eng = SSC.serve(model, prompts, 2, 40, prefix, submit_prefix=prefix if state == "device" else None, state=state, **k)
                assert "attention_segments_shared" in calls and "attention_shared" in calls and "attention_segments" not in calls
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.tolist() == w.tolist(), (state, i, g.tolist(), w.tolist())
        assert eng.steps["segments"] >= 3 and eng.steps["decode"] >= 1, eng.steps
        assert eng.cache.base is prefix and eng.cache.row_lens() == [VIDEO[1]] * 2 and eng.cache.qkv[0].shape[1] == 40 - VIDEO[1]
        assert not loads, "an admission copies nothing"
        assert prefix.len == VIDEO[1] and all(_poison.bits_equal(x, y) for x, y in zip(prefix.qkv, before)), "the base is only read"
        other = lm.new_cache(1, VIDEO[1], "cpu")
        lm.prefill(video[None], None, cache=other)
        with pytest.raises(ValueError, match="one base per Engine"):
            eng.submit(prompts[0], prefix=other)
        with pytest.raises(ValueError, match="positions"):        # the fit check counts the base: 11 + 27 + 4 - 1 > 40
            eng.submit(T("seg.long", (27, 256), 0.05), max_new_tokens=4)
        eng.submit(T("seg.long", (26, 256), 0.05), max_new_tokens=4)


def test_engine_base_must_be_a_one_row_uniform_cache_without_a_base():
    from stllm_amd import serving
    model = small_llama(SMALL)
    lm = model.model
    emb = T("seg.emb", (4, 40, 256), 0.05)
    with _backend():
        two = lm.new_cache(2, 12, "cpu")
        lm.prefill(emb[:2, :12], None, cache=two)
        one = lm.new_cache(1, 12, "cpu")
        lm.prefill(emb[:1, :12], None, cache=one)
        for bad in (two, one.share(rows=1, max_new=4)):
            with pytest.raises(NotImplementedError, match="one-row uniform"):
                serving.Engine(model, 2, 40, base=bad)
        with pytest.raises(ValueError, match="total positions"):
            serving.Engine(model, 2, 12, base=one)


# ---- 3. Chat.answer_queue(share_prefix=True) ---------------------------------------------------------------------------------------------------------------
CFG = dict(vit_model="eva_clip_g", image_size=224, num_query_token=32, video_input="mean", use_mask=False, mvm_decode=False,
           qformer_text_input=False, max_txt_len=32, end_sym=" 2")


@pytest.fixture(scope="module")
def stllm():
    """the chat fixture of tests/test_ragged_extend_cpu.py"""
    from stllm_amd import synth
    from stllm_amd.models import st_llm
    from stllm_amd.models.blip2 import Blip2Base
    from stllm_amd.tokenizer import IdTokenizer
    old = (Blip2Base.vit_depth, Blip2Base.qformer_layers, Blip2Base.init_tokenizer)
    Blip2Base.vit_depth, Blip2Base.qformer_layers = 1, 2
    Blip2Base.init_tokenizer = classmethod(lambda cls, truncation_side="right": IdTokenizer(0, 1, 2, 32000))
    try:
        m = st_llm.STLLMForCausalLM.from_config(dict(CFG, llama_model=dict(num_hidden_layers=2)), device="cpu")
    finally:
        Blip2Base.vit_depth, Blip2Base.qformer_layers, Blip2Base.init_tokenizer = old
    synth.fill_module_(m, 0, "")
    m.lm_head.weight.mul_(6.0)
    return m


def test_chat_answer_queue_share_prefix_equals_answer_per_question(stllm):
    """three questions of different lengths about one video over TWO slots that share the prefilled video: per question the (text, ids) of Chat.answer for it
    alone; without prefix= the option raises"""
    from stllm_amd.conversation import Chat
    import _ragged_extend_case as RC
    frames = T("input.frames2", (2, 3, 224, 224))
    questions = RC.CHAT_QUESTIONS
    k = dict(max_new_tokens=4)
    with _backend():
        chat = Chat(stllm, device="cpu")
        img_list = []
        chat.upload_video(frames.view(6, 224, 224), None, img_list)
        with SSC.scored_runs() as scored:
            want = [chat.answer(img_list, q, num_beams=1, **k) for q in questions]
        assert min(scored) >= SSC.MARGIN, ("precondition: the from-scratch runs are not near a tie", min(scored))
        with _poison.poisoned_allocations():
            prefix = chat.prefill_video(img_list)
            with SSC.counting() as calls:
                got = chat.answer_queue(img_list, questions, slots=2, prefix=prefix, share_prefix=True, **k)
                assert calls.count("attention_segments_shared") >= 2 * 2 and "attention_segments" not in calls, "at least two admission steps of two layers"
        assert len(got) == 3
        for (t0, i0), (t1, i1) in zip(want, got):
            assert np.array_equal(i0, i1) and t0 == t1
        with pytest.raises(ValueError, match="needs prefix="):
            chat.answer_queue(img_list, questions, slots=2, share_prefix=True, **k)
