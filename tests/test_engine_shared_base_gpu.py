"""GPU (-m gpu): the packed segment step on a shared base and serving.Engine(base=) on the device — LlamaModel.step_segments on a cache with
a base against from-scratch prefills of [video, row], serving.Engine(base=) against generate() of every request alone (host and device state),
Chat.answer_queue(share_prefix=True) against Chat.answer.  The model is the suite's two-layer full-width one (4096 wide, 32 heads, lm_head x 6), built as
tests/test_segments_gpu.py builds it; every cache is allocated under _poison.poisoned_allocations()."""
import numpy as np
import pytest
import torch

import _poison
import _ragged_extend_case as RC
import _segments_shared_case as SSC
from _util import T

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
CFG = dict(vit_model="eva_clip_g", image_size=224, num_query_token=32, video_input="mean", use_mask=False, mvm_decode=False,
           qformer_text_input=False, max_txt_len=32, end_sym=" 2")
# tests/test_segments_gpu.py's WIDE_SEEDS[True] / WIDE_VIDEO (copied): prompts T("seg.greq{i}.{seed}", (n, 4096)) vetted on the CPU contract backend (fp32, the
# same model) behind that video: every generated step's from-scratch margin is >= 1.8e-2 x max |score|; the test asserts >= MARGIN on this run's own reference
WIDE_SEEDS = [1, 0, 12, 2, 0]
WIDE_VIDEO = ("seg.greq.video.0", 11)


def _llm(layers=2, spread=None):
    from stllm_amd import synth
    from stllm_amd.models.st_llm import STLLMForCausalLM, StllmConfig
    m = STLLMForCausalLM(StllmConfig(num_hidden_layers=layers), device="cuda")
    synth.fill_module_(m, 0, "")
    if spread:
        m.lm_head.weight.mul_(spread)
    return m


@pytest.fixture(scope="module")
def llm():
    return _llm(spread=6.0)


def _prompts():
    return [T(f"seg.greq{i}.{s}", (n, 4096), 0.05).cuda() for i, (n, s) in enumerate(zip(SSC.REQ_PROMPTS, WIDE_SEEDS))]


def _prefilled(lm, video):
    prefix = lm.new_cache(1, WIDE_VIDEO[1], "cuda")
    lm.prefill(video[None], None, cache=prefix)
    return prefix, [x.clone() for x in prefix.qkv]


# ---- 1. LlamaModel.step_segments on a cache with a base ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16"])
def test_step_segments_on_a_base_matches_from_scratch_prefills_on_device(llm, mode):
    """the two-call case of tests/test_engine_shared_base_cpu.py at full width: an 11-token video shared by 4 slots, 17 / 33 / 5 tokens admitted into slots
    0 / 2 / 3, then 1 / 9 / 1 appended to slots 0 / 1 / 2"""
    from stllm_amd import hip, runtime
    video, emb = T(WIDE_VIDEO[0], (WIDE_VIDEO[1], 4096), 0.05).cuda(), T("seg.wide", (4, 40, 4096), 0.05).cuda()
    try:
        with runtime.use_dtype(mode), _poison.poisoned_allocations() as counts:
            SSC.check_two_calls(llm, video, emb, "cuda", SSC.MODEL_TOL[mode], mode)
            assert counts.allocations > 0 and hip.gemm_workspace_ok()
    finally:
        llm.model.repack()
        llm._lm_packed = {}


# ---- 2. serving.Engine(base=) ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", ["host", "device"])
def test_engine_on_a_base_gives_every_request_the_ids_of_generate_alone_on_device(llm, state):
    """fp32: 5 requests of different prompt lengths and max_new_tokens over 2 slots behind ONE prefilled video, greedy, with an EOS id that request 1 emits
    mid-way: the ids of generate([video, prompt]) alone, both kinds of step, the base bit-unchanged"""
    from stllm_amd import hip, runtime
    model, lm = llm, llm.model
    prompts = _prompts()
    video = T(WIDE_VIDEO[0], (WIDE_VIDEO[1], 4096), 0.05).cuda()
    k = dict(do_sample=False, min_length=0)
    with runtime.use_dtype("fp32"):
        free = SSC.alone(model, prompts, video, eos_token_id=None, **k)
        k["eos_token_id"] = int(free[1][1])
        with SSC.scored_runs() as scored:
            want = SSC.alone(model, prompts, video, **k)
        print("from-scratch margins:", [f"{m:.4f}" for m in scored])
        assert min(scored) >= SSC.MARGIN, ("precondition: the from-scratch runs are not near a tie", min(scored))
        assert want[1].tolist() == free[1][:2].tolist()
        with _poison.poisoned_allocations():
            prefix, before = _prefilled(lm, video)
            got, eng = SSC.serve(model, prompts, 2, 40, prefix, state=state, **k)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.tolist() == w.tolist(), (state, i, g.tolist(), w.tolist())
        assert eng.steps["segments"] >= 3 and eng.steps["decode"] >= 1, eng.steps
        assert all(_poison.bits_equal(x, y) for x, y in zip(prefix.qkv, before)), "the base is only read"
    assert hip.gemm_workspace_ok()


def test_engine_on_a_base_bf16_runs_both_kinds_of_step(llm):
    """bf16 (the serving dtype): the same requests run to completion through admission and decode steps with finite logits and the expected lengths; ids are
    not compared (a 16-bit near-tie may legitimately differ from the from-scratch run)"""
    from stllm_amd import runtime
    prompts = _prompts()
    video = T(WIDE_VIDEO[0], (WIDE_VIDEO[1], 4096), 0.05).cuda()
    seen = []
    logits_from = llm.logits_from
    try:
        with runtime.use_dtype("bf16"), _poison.poisoned_allocations():
            llm.model.repack()
            llm._lm_packed = {}
            llm.logits_from = lambda *a, **kw: (seen.append(logits_from(*a, **kw)), seen[-1])[1]
            prefix, before = _prefilled(llm.model, video)
            del seen[:]
            got, eng = SSC.serve(llm, prompts, 2, 40, prefix, do_sample=False, min_length=1, eos_token_id=None)
        assert [g.numel() for g in got] == SSC.REQ_MAX_NEW and eng.steps["segments"] >= 3 and eng.steps["decode"] >= 1
        assert len(seen) == eng.steps["segments"] + eng.steps["decode"] and all(bool(torch.isfinite(x.float()).all()) for x in seen), "finite logits in every step"
        assert all(_poison.bits_equal(x, y) for x, y in zip(prefix.qkv, before)), "the base is only read"
    finally:
        llm.__dict__.pop("logits_from", None)
        llm.model.repack()
        llm._lm_packed = {}


# ---- 3. Chat.answer_queue(share_prefix=True) ---------------------------------------------------------------------------------------------------------------
def test_chat_answer_queue_share_prefix_on_device():
    """fp32: three questions (vetted for tests/test_ragged_extend_gpu.py) over two slots that share the prefilled video: Chat.answer per question"""
    from stllm_amd import runtime, synth
    from stllm_amd.conversation import Chat
    from stllm_amd.models import st_llm
    from stllm_amd.models.blip2 import Blip2Base
    from stllm_amd.tokenizer import IdTokenizer
    old = (Blip2Base.vit_depth, Blip2Base.qformer_layers, Blip2Base.init_tokenizer)
    Blip2Base.vit_depth, Blip2Base.qformer_layers = 1, 2
    Blip2Base.init_tokenizer = classmethod(lambda cls, truncation_side="right": IdTokenizer(0, 1, 2, 32000))
    try:
        model = st_llm.STLLMForCausalLM.from_config(dict(CFG, llama_model=dict(num_hidden_layers=2)), device="cuda")
    finally:
        Blip2Base.vit_depth, Blip2Base.qformer_layers, Blip2Base.init_tokenizer = old
    synth.fill_module_(model, 0, "")
    model.lm_head.weight.mul_(6.0)
    k = dict(max_new_tokens=4)
    with runtime.use_dtype("fp32"):
        chat = Chat(model, device="cuda")
        img_list = []
        chat.upload_video(T("input.frames2", (2, 3, 224, 224)).view(6, 224, 224).cuda(), None, img_list)
        with SSC.scored_runs() as scored:
            want = [chat.answer(img_list, q, num_beams=1, **k) for q in RC.CHAT_QUESTIONS]
        print("from-scratch margins:", [f"{m:.4f}" for m in scored])
        assert min(scored) >= SSC.MARGIN, ("precondition: the from-scratch runs are not near a tie", min(scored))
        with _poison.poisoned_allocations():
            prefix = chat.prefill_video(img_list)
            got = chat.answer_queue(img_list, RC.CHAT_QUESTIONS, slots=2, prefix=prefix, share_prefix=True, **k)
        for (t0, i0), (t1, i1) in zip(want, got):
            assert np.array_equal(i0, i1) and t0 == t1
