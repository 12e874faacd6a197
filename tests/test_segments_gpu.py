"""GPU (-m gpu): the packed segment step on the device — stllm_attention_segments (tile kernel and key-split pair, forced on, forced off and by the rule;
fp32 vector kernel) and stllm_kv_append_segments on the cases of tests/_segments_case.py, LlamaModel.step_segments against from-scratch prefills,
serving.Engine against generate() of every request alone, Chat.answer_queue against Chat.answer."""
import numpy as np
import pytest
import torch

import _poison
import _ragged_extend_case as RC
import _segments_case as SC
from _util import T

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
CFG = dict(vit_model="eva_clip_g", image_size=224, num_query_token=32, video_input="mean", use_mask=False, mvm_decode=False,
           qformer_text_input=False, max_txt_len=32, end_sym=" 2")


@pytest.fixture(scope="module")
def hip():
    from stllm_amd import hip as h
    h.lib()
    return h


# ---- 1. the kernels --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_attention_segments_on_device(hip, dtype):
    """tests/test_segments_kernels_cpu.py::test_emulated_attention_segments on the device: every packed row against fp64, no NaN although every row a pad
    lane could reach is NaN, the 8 rows behind T unchanged, a poisoned workspace, the cache unchanged, the same bits twice"""
    td = DT[dtype]
    case = SC.SegmentCase(td)
    assert case.T == 89 and case.dominating_weight > 0.9
    host_cache = case.cache.clone()
    case.to("cuda")
    try:
        for opt in ((0, 1, -1) if dtype != "fp32" else (-1,)):
            hip.set_option("attn_ksplit", opt)
            with _poison.poisoned_allocations() as counts:
                got = case.run(hip, out=case.out_buffer())
                again = case.run(hip, out=case.out_buffer())
            ran = hip.lib().stllm_last_kernel().decode()
            if dtype == "fp32":
                assert ran == "attn_f32_kernel", ran
            else:
                assert ran == ("attn_mfma_kernel" if opt == 0 else "attn_ksplit_kernel"), (opt, ran)   # the rule: 20 query-tile triples, 240 keys
                assert counts.allocations >= 1
            assert _poison.bits_equal(got, again), "the same call twice gives the same bits"
            case.check(got, f"attn_ksplit={opt} -> {ran}")
    finally:
        hip.set_option("attn_ksplit", -1)
    assert _poison.bits_equal(case.cache.cpu(), host_cache), "the cache is read-only for the attention"


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_identity_tables_equal_the_ragged_entry_bit_for_bit(hip, dtype):
    q_off, Sq = [170, 33, 200], 40
    rc = RC.KernelCase(DT[dtype], q_off=q_off, n_new=[Sq] * 3, poison=False).to("cuda")
    HD, f = rc.HD, rc.flat(rc.cache)
    st = (rc.ML * 3 * HD, 3 * HD)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device="cuda")
    try:
        for opt in ((0, 1) if dtype != "fp32" else (-1,)):
            hip.set_option("attn_ksplit", opt)
            want = rc.run(hip)
            ran = hip.lib().stllm_last_kernel().decode()
            got = hip.attention_segments(rc.dense[:, :HD], f[:, HD:2 * HD], f[:, 2 * HD:], i32([0, 1, 2]), i32([0, Sq, 2 * Sq]), rc.q_off, rc.kv_len, H=rc.H,
                                         D=128, T=3 * Sq, n_slots=3, max_n=Sq, max_kv=rc.max_kv, scale=128 ** -0.5, k_strides=st, v_strides=st)
            assert ran == hip.lib().stllm_last_kernel().decode()
            assert _poison.bits_equal(got, want), (dtype, opt, ran)
    finally:
        hip.set_option("attn_ksplit", -1)


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_kv_append_segments_on_device(hip, dtype):
    cache, src, tabs, T_, max_n, want = SC.append_case(DT[dtype])
    buf = torch.empty((cache.shape[0], cache.shape[1] + 1, cache.shape[2]), dtype=cache.dtype, device="cuda")
    buf[:, :cache.shape[1]] = cache.cuda()
    buf[:, cache.shape[1]:] = 7.0
    dev = buf[:, :cache.shape[1]]                     # cache row stride > max_len x row stride, as on the host
    hip.kv_append_segments(src.cuda(), dev, *[t.cuda() for t in tabs], T=T_, max_n=max_n)
    assert _poison.bits_equal(dev.cpu(), want) and bool((buf[:, cache.shape[1]:] == 7.0).all())
    c0, s0, pos0, n, S, w0 = RC.append_case(DT[dtype])
    B = c0.shape[0]
    d0, d1 = c0.cuda(), c0.cuda()
    hip.kv_append_spans(s0.cuda(), d0, pos0.cuda(), n.cuda(), S=S)
    ar = torch.arange(B, dtype=torch.int32, device="cuda")
    hip.kv_append_segments(s0.cuda(), d1, ar, ar * S, pos0.cuda(), n.cuda(), T=B * S, max_n=S)
    assert _poison.bits_equal(d0.cpu(), w0) and _poison.bits_equal(d1, d0), "identity tables: stllm_kv_append_spans' bits"


# ---- 2. LlamaModel.step_segments ---------------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16"])
def test_step_segments_matches_a_from_scratch_prefill_on_device(llm, mode):
    """slots holding 17, 0 and 33 positions, one call with 1, 9 and 1 tokens, every cache allocated under poison: each row's hidden state against a
    from-scratch prefill of that row's full sequence, and the unnamed fourth slot bit-unchanged in every layer.  As in tests/test_ragged_extend_gpu.py the
    model is the full-width (4096, 32 heads) two-layer one of the suite's model-level GPU tests — the widths the kernels are dispatched for —, not the
    256-wide model of the CPU suites; slots, tokens, bound and poison are the same."""
    from stllm_amd import runtime
    tol = SC.MODEL_TOL[mode]
    emb = T("seg.wide", (4, 40, 4096), 0.05).cuda()
    try:
        with runtime.use_dtype(mode), _poison.poisoned_allocations() as counts:
            h32, h16, cache, before = SC.segment_step(llm, emb, 48, "cuda")
            assert counts.allocations > 0 and bool(torch.isfinite(h32).all())
            for x, y in zip(cache.qkv, before):
                assert _poison.bits_equal(x[3], y[3]), "the slot that no segment names is untouched"
            for b in range(3):
                want, alone = SC.from_scratch(llm, emb, b, "cuda")
                err, scale = float((h32[b] - want).abs().max()), float(want.abs().max())
                print(f"[{mode}] step_segments row {b}: hidden err {err:.3e} (bound {tol:.0e} x {scale:.3f})")
                assert err <= tol * scale, (mode, b, err, scale)
                L = SC.STEP_HAVE[b] + SC.STEP_NEW[b]
                for x, y in zip(cache.qkv, alone.qkv):
                    kv, ref = x[b, :L, 4096:].float(), y[0, :L, 4096:].float()
                    assert float((kv - ref).abs().max()) <= tol * float(ref.abs().max()), ("cache rows", mode, b)
    finally:
        llm.model.repack()
        llm._lm_packed = {}


# ---- 3. serving.Engine -----------------------------------------------------------------------------------------------------------------------------------
# prompts T("seg.greq{i}.{seed}", (n, 4096)) vetted on the CPU contract backend (fp32, the same two-layer full-width model): every generated step's
# from-scratch margin is >= 1.8e-2 x max |score|; the test asserts >= MARGIN on this run's own reference
WIDE_SEEDS = {False: [1, 1, 5, 3, 0], True: [1, 0, 12, 2, 0]}
WIDE_VIDEO = ("seg.greq.video.0", 11)


@pytest.mark.parametrize("with_prefix", [False, True])
def test_engine_gives_every_request_the_ids_of_generate_alone_on_device(llm, with_prefix):
    """fp32: 5 requests of different prompt lengths and max_new_tokens over 2 slots, greedy, with an EOS id that request 1 emits mid-way (its slot is taken
    while the neighbour keeps decoding); with and without a shared video prefix"""
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
        with _poison.poisoned_allocations():
            got, eng = SC.serve(model, prompts, 2, 40, prefix=prefix, **k)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.tolist() == w.tolist(), (i, g.tolist(), w.tolist())
        assert eng.steps["segments"] >= 3 and eng.steps["decode"] >= 1, eng.steps
        if with_prefix:
            assert all(_poison.bits_equal(x, y) for x, y in zip(prefix.qkv, before)), "the prefix is only read"
    assert hip.gemm_workspace_ok()


def test_engine_bf16_runs_both_kinds_of_step(llm):
    """bf16 (the serving dtype): the same requests run to completion through admission and decode steps with finite logits; ids are not compared (a 16-bit
    near-tie may legitimately differ from the from-scratch run)"""
    from stllm_amd import runtime
    prompts = [T(f"seg.greq{i}.{s}", (n, 4096), 0.05).cuda() for i, (n, s) in enumerate(zip(SC.REQ_PROMPTS, WIDE_SEEDS[False]))]
    try:
        with runtime.use_dtype("bf16"), _poison.poisoned_allocations():
            llm.model.repack()
            llm._lm_packed = {}
            got, eng = SC.serve(llm, prompts, 2, 40, do_sample=False, min_length=1, eos_token_id=None)
        assert [g.numel() for g in got] == SC.REQ_MAX_NEW and eng.steps["segments"] >= 3 and eng.steps["decode"] >= 1
    finally:
        llm.model.repack()
        llm._lm_packed = {}


# ---- 4. Chat.answer_queue ------------------------------------------------------------------------------------------------------------------------------
def test_chat_answer_queue_on_device():
    """fp32: three questions (vetted for tests/test_ragged_extend_gpu.py) over two slots behind the prefilled video: Chat.answer per question"""
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
        prefix = chat.prefill_video(img_list)
        with SC.scored_runs() as scored:
            want = [chat.answer(img_list, q, num_beams=1, **k) for q in RC.CHAT_QUESTIONS]
        print("from-scratch margins:", [f"{m:.4f}" for m in scored])
        assert min(scored) >= SC.MARGIN, ("precondition: the from-scratch runs are not near a tie", min(scored))
        got = chat.answer_queue(img_list, RC.CHAT_QUESTIONS, slots=2, prefix=prefix, **k)
        for (t0, i0), (t1, i1) in zip(want, got):
            assert np.array_equal(i0, i1) and t0 == t1
