"""GPU (-m gpu): continuous batching for beam search on the device — stllm_kv_reorder_rows and stllm_beam_candidates_rows on the cases of
tests/_engine_beams_case.py (the functions tests/test_engine_beams_kernels_cpu.py runs on the emulated kernels), serving.Engine(num_beams > 1) against
generate(num_beams=nb) of every request alone in both states (fp32, the two-layer full-width model of tests/test_segments_gpu.py), the reference's ids,
Chat.answer_queue(num_beams=5), bf16, a poisoned-allocation run."""
import numpy as np
import pytest
import torch

import _engine_beams_case as BC
import _poison
import _ragged_extend_case as RC
from _util import T, golden

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


@pytest.fixture(scope="module")
def hip():
    from stllm_amd import hip as h
    h.lib()
    return h


@pytest.fixture(scope="module")
def llm():
    from test_segments_gpu import _llm
    return _llm(spread=6.0)


# ---- 1. the kernels --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("name", list(BC.REORDER_CASES))
def test_kv_reorder_rows_on_device(hip, name, dtype):
    assert BC.check_reorder(hip, "cuda", DT[dtype], name) > 0


def test_kv_reorder_rows_refuses_17_rows_per_group_on_device(hip):
    BC.check_reorder_unsupported(hip, "cuda")


@pytest.mark.parametrize("penalty", [1.0, 1.5])
@pytest.mark.parametrize("k", [6, 10])
@pytest.mark.parametrize("V", [1000, 32000])
def test_beam_candidates_rows_on_device(hip, V, k, penalty):
    BC.check_candidates(hip, "cuda", V, k, penalty)


# ---- 2. serving.Engine(num_beams > 1) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["none", "prefix", "base"])
@pytest.mark.parametrize("nb", [3, 5])
def test_beam_engine_gives_every_request_the_ids_of_generate_alone_on_device(llm, nb, mode):
    """fp32: five requests over 2 slots with nb beams, both states, with an EOS that the beams emit mid-way: is_done ends at least one request before its
    budget while another runs to its limit (asserted in check_engine); under the guard"""
    from stllm_amd import hip, runtime
    with runtime.use_dtype("fp32"):
        BC.check_engine(llm, "wide", nb, mode, "cuda")
    assert hip.gemm_workspace_ok()


def test_beam_engine_with_penalties_on_device(llm):
    from stllm_amd import runtime
    with runtime.use_dtype("fp32"):
        BC.check_engine(llm, "wide", 3, "none", "cuda", extra=dict(repetition_penalty=1.3, length_penalty=2.0, min_length=2))


def test_beam_engine_with_a_stop_sequence_on_device(llm):
    from stllm_amd import runtime
    with runtime.use_dtype("fp32"):
        prompts = BC.requests("wide", 3, 4096, "cuda")
        free, _ = BC.alone(llm, prompts, 3, do_sample=False, min_length=1, eos_token_id=BC.SEEDS["wide"][(3, False)][1])
        stop = [free[0][2:4].clone(), free[3][1:2].clone()]
        _, want = BC.check_engine(llm, "wide", 3, "none", "cuda", extra=dict(stop_sequences=stop))
        assert any(w.numel() < f.numel() for w, f in zip(want, free)), "a stop sequence cut a run short"


def test_poisoned_allocations_do_not_change_the_beam_engine_ids_on_device(llm):
    from stllm_amd import runtime
    with runtime.use_dtype("fp32"):
        clean, _ = BC.check_engine(llm, "wide", 3, "base", "cuda")
        dirty, _ = BC.check_engine(llm, "wide", 3, "base", "cuda", poisoned=True)
    assert _poison.bits_equal(clean, dirty)


def test_beam_engine_bf16_runs_both_kinds_of_step(llm):
    """bf16 (the serving dtype): a run with admission and decode steps returns ids in range and of the right lengths; no identity claim"""
    from stllm_amd import runtime
    prompts = BC.requests("wide", 5, 4096, "cuda")
    try:
        with runtime.use_dtype("bf16"), _poison.poisoned_allocations():
            llm.model.repack()
            llm._lm_packed = {}
            for state in ("host", "device"):
                got, eng, _ = BC.serve(llm, prompts, 5, 2, BC.MAX_LEN, state=state, do_sample=False, min_length=1, eos_token_id=None)
                assert [g.numel() for g in got] == BC.REQ_MAX_NEW and all(0 <= int(g.min()) and int(g.max()) < 32000 for g in got)
                assert eng.steps["segments"] >= 3 and eng.steps["decode"] >= 1 and eng.steps["reorder"] >= 1
    finally:
        llm.model.repack()
        llm._lm_packed = {}


# ---- 3. the reference's ids --------------------------------------------------------------------------------------------------------------------------------
def test_beam_engine_returns_the_reference_ids():
    """tests/golden/generate.npz: the 5-beam and the 3-beam-with-penalties prompts (the ids test_generate_on_device_matches_reference_ids checks for
    generate()), the prompts of one lm_head scale submitted to ONE Engine together, fp32"""
    from stllm_amd import runtime, serving
    from test_model_gpu import build_stllm
    g = golden("generate")
    cfg = dict(vit_model="eva_clip_g", image_size=224, num_query_token=32, video_input="mean", use_mask=False, mvm_decode=False,
               qformer_text_input=False, max_txt_len=32, end_sym=" 2")
    model = build_stllm(cfg, vit_depth=1, qf_layers=2, llm_layers=2)
    w0 = model.lm_head.weight.detach().clone()
    modes = {1: dict(num_beams=5), 2: dict(num_beams=3, repetition_penalty=1.3, length_penalty=2.0)}
    with runtime.use_dtype("fp32"):
        for scale, seeds in ((4.0, (3, 4)), (8.0, (4, 5))):
            model.lm_head.weight.copy_(w0 * scale)
            for mi, kw in modes.items():
                for state in ("host", "device"):
                    eng = serving.Engine(model, 2, 24, state=state, max_new_tokens=6, do_sample=False, min_length=1, **kw)
                    hs = [eng.submit(T(f"gen.emb{seed}", (1, 9, 4096), 0.05).cuda()[0]) for seed in seeds]
                    got = dict(eng.run())
                    for h, seed in zip(hs, seeds):
                        assert got[h].tolist() == g[f"s{scale:g}_p{seed}_m{mi}"].tolist(), (scale, seed, kw, state, got[h].tolist())
                    assert eng.steps["segments"] >= 1 and eng.steps["decode"] >= 1


# ---- 4. Chat.answer_queue ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("share", [False, True])
def test_chat_answer_queue_with_five_beams_on_device(share):
    """fp32: three questions over two slots behind the prefilled video, num_beams = 5: Chat.answer(num_beams=5) per question"""
    from stllm_amd import runtime, synth
    from stllm_amd.conversation import Chat
    from stllm_amd.models import st_llm
    from stllm_amd.models.blip2 import Blip2Base
    from stllm_amd.tokenizer import IdTokenizer
    from test_segments_gpu import CFG
    old = (Blip2Base.vit_depth, Blip2Base.qformer_layers, Blip2Base.init_tokenizer)
    Blip2Base.vit_depth, Blip2Base.qformer_layers = 1, 2
    Blip2Base.init_tokenizer = classmethod(lambda cls, truncation_side="right": IdTokenizer(0, 1, 2, 32000))
    try:
        model = st_llm.STLLMForCausalLM.from_config(dict(CFG, llama_model=dict(num_hidden_layers=2)), device="cuda")
    finally:
        Blip2Base.vit_depth, Blip2Base.qformer_layers, Blip2Base.init_tokenizer = old
    synth.fill_module_(model, 0, "")
    model.lm_head.weight.mul_(6.0)
    k = dict(max_new_tokens=4, num_beams=5)
    with runtime.use_dtype("fp32"):
        chat = Chat(model, device="cuda")
        img_list = []
        chat.upload_video(T("input.frames2", (2, 3, 224, 224)).view(6, 224, 224).cuda(), None, img_list)
        prefix = chat.prefill_video(img_list)
        want = [chat.answer(img_list, q, **k) for q in RC.CHAT_QUESTIONS]
        got = chat.answer_queue(img_list, RC.CHAT_QUESTIONS, slots=2, prefix=prefix, share_prefix=share, **k)
        for (t0, i0), (t1, i1) in zip(want, got):
            assert np.array_equal(i0, i1) and t0 == t1
