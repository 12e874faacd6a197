"""CPU: the packed segment step and the serving loop on the test-only contract backend (tests/_cpu_backend.py plus the contracts of
tests/_ragged_extend_case.py and tests/_segments_case.py, fp32): KVCache.load_row / release, LlamaModel.step_segments against from-scratch prefills,
serving.Engine against generate() of every request alone, the call lists of its two kinds of step, Chat.answer_queue against Chat.answer."""
import numpy as np
import pytest
import torch

import _cpu_backend as CB
import _poison
import _segments_case as SC
from _util import T, small_llama

torch.set_grad_enabled(False)
SMALL = SC.SMALL
LAYER = ["rmsnorm", "gemm", "kv_append_segments", "attention_segments", "gemm", "rmsnorm", "gemm", "gemm"]


# ---- 1. KVCache.load_row / release, LlamaModel.step_segments -----------------------------------------------------------------------------------------
def test_step_segments_matches_a_from_scratch_prefill_of_every_row():
    """slots holding 17, 0 and 33 positions, ONE call with 1, 9 and 1 tokens: the last token's hidden row of every segment, and the K / V the slot holds
    afterwards, against a prefill of that row's full sequence alone; one pass of the per-op layer body, T = 11 rows everywhere"""
    from stllm_amd import runtime
    model = small_llama(SMALL)
    emb = T("seg.emb", (4, 40, 256), 0.05)
    with SC.installed(), runtime.use_dtype("fp32"):
        with SC.counting() as calls:
            h32, h16, cache, _ = SC.segment_step(model, emb, 48, "cpu")
        step = calls[-(4 + 2 * len(LAYER)):]
        assert step == ["gather_rows", "gather_rows"] + LAYER * 2 + ["gather_rows", "rmsnorm"], step
        assert h32.shape == (3, 256) and h16.shape == (3, 256)
        for b in range(3):
            want, alone = SC.from_scratch(model, emb, b, "cpu")
            err, scale = float((h32[b] - want).abs().max()), float(want.abs().max())
            print(f"step_segments row {b}: hidden err {err:.3e} (bound {SC.MODEL_TOL['fp32']:.0e} x {scale:.3f})")
            assert err <= SC.MODEL_TOL["fp32"] * scale, (b, err, scale)
            L = SC.STEP_HAVE[b] + SC.STEP_NEW[b]
            for x, y in zip(cache.qkv, alone.qkv):
                assert float((x[b, :L, 256:] - y[0, :L, 256:]).abs().max()) <= SC.MODEL_TOL["fp32"] * float(y[0, :L, 256:].abs().max()), b


def test_step_segments_leaves_an_unnamed_slot_bit_unchanged():
    """the fourth slot is named by no segment: its bytes in every layer (the don't-care rows behind its length included) and its length stay; so do the
    positions in front of the named slots' new ones"""
    from stllm_amd import runtime
    model = small_llama(SMALL)
    emb = T("seg.emb", (4, 40, 256), 0.05)
    with SC.installed(), runtime.use_dtype("fp32"), _poison.poisoned_allocations() as counts:
        h32, _, cache, before = SC.segment_step(model, emb, 48, "cpu")
    assert counts.allocations > 0 and bool(torch.isfinite(h32).all())
    for x, y in zip(cache.qkv, before):
        assert _poison.bits_equal(x[3], y[3]), "the unnamed slot"
        for b, (P, n) in enumerate(zip(SC.STEP_HAVE, SC.STEP_NEW)):
            assert _poison.bits_equal(x[b, :P], y[b, :P]) and _poison.bits_equal(x[b, P + n:], y[b, P + n:]) and _poison.bits_equal(x[b, :, :256], y[b, :, :256])
            assert bool(torch.isfinite(x[b, P:P + n, 256:]).all())


def test_load_row_release_and_the_error_paths():
    from stllm_amd import hip, runtime
    model = small_llama(SMALL)
    lm = model.model
    emb = T("seg.emb", (4, 40, 256), 0.05)
    with SC.installed(), runtime.use_dtype("fp32"):
        src = lm.new_cache(2, 12, "cpu")
        lm.prefill(emb[:2, :12], None, cache=src)
        c = lm.new_cache(3, 20, "cpu")
        c.set_lens([0, 0, 0])
        c.load_row(2, src, src_row=1)
        assert c.row_lens() == [0, 0, 12] and all(torch.equal(x[2, :12, 256:], y[1, :12, 256:]) for x, y in zip(c.qkv, src.qkv))
        c.load_row(0, src)
        c.release(2)
        assert c.row_lens() == [12, 0, 0]
        c.release(0)
        assert c.lens is None and c.len == 0
        with pytest.raises(NotImplementedError, match="base"):
            c.load_row(0, src.share(rows=2, max_new=4))
        ragged = lm.new_cache(2, 12, "cpu")
        ragged.set_lens([3, 5])
        with pytest.raises(NotImplementedError, match="uniform"):
            c.load_row(0, ragged)
        c.load_row(0, src)
        with pytest.raises(AssertionError, match="distinct"):
            lm.step_segments(emb[0, :2], c, [(0, 1), (0, 1)])
        with pytest.raises(AssertionError, match="distinct"):
            lm.step_segments(emb[0, :2], c, [(0, 1), (3, 1)])
        with pytest.raises(AssertionError, match="at least one token"):
            lm.step_segments(emb[0, :2], c, [(0, 2), (1, 0)])
        with pytest.raises(AssertionError, match="KV cache full"):
            lm.step_segments(emb[0, :9], c, [(0, 9)])
        with pytest.raises(NotImplementedError, match="base"):
            lm.step_segments(emb[0, :2], src.share(rows=2, max_new=4), [(0, 1), (1, 1)])
        assert c.row_lens() == [12, 0, 0]
        with runtime.use_decode_weights("int8"), pytest.raises(NotImplementedError, match="decode_step"):
            lm.step_segments(emb[0, :2], c, [(0, 1), (1, 1)])
    with runtime.use_dtype("bf16x3"), pytest.raises(NotImplementedError, match="bf16x3"):
        lm.step_segments(emb[0, :2], c, [(0, 1), (1, 1)])
    assert hip.segments_available("cpu") is False
    with CB.installed(), runtime.use_dtype("fp32"), pytest.raises(NotImplementedError, match="attention_segments"):
        lm.step_segments(emb[0, :2], c, [(0, 1), (1, 1)])


# ---- 2. serving.Engine ---------------------------------------------------------------------------------------------------------------------------------
# Id-equality cases: the prompts are T("seg.req{i}.{seed}") with seeds vetted on the CPU such that, with and without the video in front, the from-scratch
# run's top-1 / top-2 margin of the processed scores is >= 1.8e-2 x max |score| at every generated step (fp32, the model-level bound is 2e-4); the tests
# assert >= MARGIN = 1e-2 themselves (scored_runs).
REQ_SEEDS, VIDEO = [0, 2, 4, 7, 0], ("seg.req.video.0", 11)


def _requests(D=256, device="cpu"):
    return [T(f"seg.req{i}.{s}", (n, D), 0.05).to(device) for i, (n, s) in enumerate(zip(SC.REQ_PROMPTS, REQ_SEEDS))]


@pytest.mark.parametrize("with_prefix", [False, True])
def test_engine_gives_every_request_the_ids_of_generate_alone(with_prefix):
    """5 requests of different prompt lengths and max_new_tokens over 2 slots, greedy; with an EOS id that one request emits mid-way, so that its slot is
    taken by the next request while the neighbour keeps decoding"""
    from stllm_amd import runtime
    model = small_llama(SMALL, lm_head_spread=6.0)
    lm = model.model
    prompts = _requests()
    video = T(VIDEO[0], (VIDEO[1], 256), 0.05) if with_prefix else None
    k = dict(do_sample=False, min_length=0)   # (no EOS suppression: the runs with the EOS id are the free runs, cut where it appears)
    with SC.installed(), runtime.use_dtype("fp32"):
        free = SC.alone(model, prompts, video, eos_token_id=None, **k)
        eos = int(free[1][1])          # request 1 (max_new_tokens = 3) ends on its second token
        k["eos_token_id"] = eos
        with SC.scored_runs() as scored:
            want = SC.alone(model, prompts, video, **k)
        assert min(scored) >= SC.MARGIN, ("precondition: the from-scratch runs are not near a tie", min(scored))
        assert want[1].tolist() == free[1][:2].tolist() and any(w.numel() == n for w, n in zip(want, SC.REQ_MAX_NEW)), "one ends on EOS, one runs to its limit"
        prefix = None
        if with_prefix:
            prefix = lm.new_cache(1, VIDEO[1], "cpu")
            lm.prefill(video[None], None, cache=prefix)
            before = [x.clone() for x in prefix.qkv]
        got, eng = SC.serve(model, prompts, 2, 40, prefix=prefix, **k)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.tolist() == w.tolist(), (i, g.tolist(), w.tolist())
        assert eng.steps["segments"] >= 3 and eng.steps["decode"] >= 1, eng.steps
        if with_prefix:
            assert prefix.len == VIDEO[1] and all(_poison.bits_equal(x, y) for x, y in zip(prefix.qkv, before)), "the prefix is only read"


def test_engine_call_lists_and_slot_bookkeeping():
    """an admission step is ONE segment pass (no decode_step launch: no kv_append_rows, no decode attention); a step without admissions is exactly
    decode_step's list on the slot cache; running rows do not stall while a request is admitted"""
    from stllm_amd import runtime, serving
    model = small_llama(SMALL, lm_head_spread=6.0)
    lm = model.model
    prompts = _requests()
    with SC.installed(), runtime.use_dtype("fp32"):
        eng = serving.Engine(model, 2, 40, do_sample=False, min_length=1, eos_token_id=None, max_new_tokens=4)
        a = eng.submit(prompts[0])
        with SC.counting() as calls:
            assert eng.step() == []
            assert calls == ["gather_rows", "gather_rows"] + LAYER * 2 + ["gather_rows", "rmsnorm", "gemm"], calls
        assert eng.cache.row_lens() == [5, 0] and sorted(eng.running) == [0]
        ref = lm.new_cache(2, 40, "cpu")
        ref.set_lens([5, 0])
        with SC.counting() as want_calls:
            lm.decode_step(lm.embed_tokens(torch.tensor([[5], [0]])), ref)
            want_calls = list(want_calls)
        with SC.counting() as calls:
            assert eng.step() == []
            assert calls == want_calls + ["gemm"] and "attention_segments" not in calls, (calls, want_calls)
        assert eng.cache.row_lens() == [6, 0], "the free slot rode along and is empty again"
        b = eng.submit(prompts[1], max_new_tokens=2)
        with SC.counting() as calls:
            assert eng.step() == []
            assert calls.count("attention_segments") == 2 and calls.count("kv_append_segments") == 2 and "kv_append_rows" not in calls, calls
        assert eng.cache.row_lens() == [7, 9], "the running request went on while the other was admitted"
        done = eng.step()
        assert [h for h, _ in done] == [a, b] and done[0][1].numel() == 4 and done[1][1].numel() == 2
        assert eng.step() == [] and eng.idle() and eng.cache.row_lens() == [0, 0]
        with pytest.raises(ValueError, match="positions"):
            eng.submit(T("seg.long", (38, 256), 0.05), max_new_tokens=4)
        for bad in (dict(num_beams=2), dict(selection="device")):
            with pytest.raises(NotImplementedError):
                serving.Engine(model, 2, 40, **bad)


def test_engine_sampling_draws_per_request():
    """do_sample with a generator per request: a request's ids do not depend on what shares the batch with it"""
    from stllm_amd import runtime, serving
    model = small_llama(SMALL, lm_head_spread=6.0)
    prompts = _requests()
    k = dict(do_sample=True, top_p=0.9, temperature=0.8, min_length=1, eos_token_id=None, max_new_tokens=5)
    with SC.installed(), runtime.use_dtype("fp32"):
        want = [model.generate(inputs_embeds=p[None], generator=torch.Generator().manual_seed(7 + i), **k)[0] for i, p in enumerate(prompts[:3])]
        eng = serving.Engine(model, 2, 40, **k)
        hs = [eng.submit(p, generator=torch.Generator().manual_seed(7 + i)) for i, p in enumerate(prompts[:3])]
        got = dict(eng.run())
        for h, w in zip(hs, want):
            assert got[h].tolist() == w.tolist()


# ---- 3. Chat.answer_queue ------------------------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("with_prefix", [True, False])
def test_chat_answer_queue_equals_answer_per_question(stllm, with_prefix):
    """three questions of different lengths about one video over TWO slots (K < N): per question the (text, ids) of Chat.answer for it alone"""
    from stllm_amd import runtime
    from stllm_amd.conversation import Chat
    import _ragged_extend_case as RC
    frames = T("input.frames2", (2, 3, 224, 224))
    questions = RC.CHAT_QUESTIONS
    k = dict(max_new_tokens=4)
    with SC.installed(), runtime.use_dtype("fp32"):
        chat = Chat(stllm, device="cpu")
        img_list = []
        chat.upload_video(frames.view(6, 224, 224), None, img_list)
        prefix = chat.prefill_video(img_list) if with_prefix else None
        with SC.scored_runs() as scored:
            want = [chat.answer(img_list, q, num_beams=1, **k) for q in questions]
        assert min(scored) >= SC.MARGIN, ("precondition: the from-scratch runs are not near a tie", min(scored))
        with SC.counting() as calls:
            got = chat.answer_queue(img_list, questions, slots=2, prefix=prefix, **k)
            assert calls.count("attention_segments") >= 2 * 2, "at least two admission steps of two layers"
        assert len(got) == 3
        for (t0, i0), (t1, i1) in zip(want, got):
            assert np.array_equal(i0, i1) and t0 == t1
        one = chat.answer_queue(img_list, questions[:1], slots=8, prefix=prefix, **k)
        assert np.array_equal(one[0][1], want[0][1])
