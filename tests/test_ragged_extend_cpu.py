"""CPU: the ragged extend — stllm_attention_offset_ragged / stllm_kv_append_spans on the host emulator of the real sources (tests/hipemu); LlamaModel.extend on a
ragged cache, generate() behind a ragged per-prompt prefix, return_cache and Chat.follow_up on the test-only contract backend (tests/_cpu_backend.py plus the
two contracts of tests/_ragged_extend_case.py, fp32); the C ABI surface."""
import os
import re

import numpy as np
import pytest
import torch

import _cpu_backend as CB
import _hipemu
import _poison
import _ragged_extend_case as RC
from _util import T, small_llama

torch.set_grad_enabled(False)
needs_emu = pytest.mark.skipif(not _hipemu.available() or _hipemu.ON_DEVICE, reason="ROCm clang++ not found: cannot build the emulated kernels")
SMALL = RC.SMALL


# ---- 1. the kernels, emulated from source ----------------------------------------------------------------------------------------------------------
@needs_emu
@pytest.mark.parametrize("dtype,opts", [(torch.bfloat16, (0, 1)), (torch.float16, (0, 1)), (torch.float32, (-1,))])
def test_emulated_attention_offset_ragged(dtype, opts):
    """the case of tests/_ragged_extend_case.py: live rows against fp64 of the same inputs, pad rows exactly zero, the guard around the output intact, the
    cache bit-identical afterwards, the kernel that was forced, the same bits twice"""
    case = RC.KernelCase(dtype)
    with _hipemu.emulated() as hip:
        try:
            for opt in opts:
                hip.set_option("attn_ksplit", opt)
                g = _poison.Guarded(case.B * case.Sq, case.HD, dtype)
                with _poison.poisoned_allocations() as counts:   # the key-split workspace starts as 0xFF in every byte
                    got = case.run(hip, out=g.out)
                    again = case.run(hip)
                ran = hip.lib().stllm_last_kernel().decode()
                assert ("ksplit" in ran) == (opt == 1), (ran, opt)
                assert dtype != torch.float32 or ran == "attn_f32_kernel"
                assert counts.allocations >= 1 and g.intact(), "no byte around the output rows was written"
                assert _poison.bits_equal(got.contiguous(), again), "the same call twice gives the same bits"
                assert _poison.bits_equal(case.cache, case.before), "the cache is read-only"
                case.check(got, f"attn_ksplit={opt} ({ran})")
        finally:
            hip.set_option("attn_ksplit", -1)


@needs_emu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_emulated_uniform_tables_equal_the_offset_entry_bit_for_bit(dtype):
    """q_off[b] = P, kv_len[b] = P + Sq: the output of stllm_attention_offset(q_off = P, Skv = P + Sq), under both forced settings"""
    P, Sq, B = 170, 40, 2
    case = RC.KernelCase(dtype, q_off=[P] * B, n_new=[Sq] * B, poison=False)
    HD, f = case.HD, case.flat(case.cache)
    st = (case.ML * 3 * HD, 3 * HD)
    with _hipemu.emulated() as hip:
        try:
            for opt in (0, 1):
                hip.set_option("attn_ksplit", opt)
                got = case.run(hip)
                ran = hip.lib().stllm_last_kernel().decode()
                want = hip.attention(case.dense[:, :HD], f[:, HD:2 * HD], f[:, 2 * HD:], B=B, H=case.H, Sq=Sq, Skv=P + Sq, D=128, scale=128 ** -0.5, causal=True,
                                     q_off=P, q_strides=(Sq * 3 * HD, 3 * HD), k_strides=st, v_strides=st)
                assert ran == hip.lib().stllm_last_kernel().decode() and ("ksplit" in ran) == (opt == 1)
                assert _poison.bits_equal(got, want), (dtype, opt, ran)
        finally:
            hip.set_option("attn_ksplit", -1)


@needs_emu
def test_emulated_attention_offset_ragged_rejects_what_it_does_not_serve():
    """head_dim 64, and fp32 beyond the vector kernel's 2048 keys: STLLM_ERR_UNSUPPORTED with a message, never another kernel"""
    q, c = RC.rnd(2 * 4, 3 * 128), RC.rnd(2 * 8, 3 * 128)
    tabs = torch.tensor([3, 1], dtype=torch.int32), torch.tensor([5, 4], dtype=torch.int32)
    with _hipemu.emulated() as hip:
        with pytest.raises(RuntimeError, match="unsupported"):
            hip.attention_offset_ragged(q[:, :128].bfloat16(), c[:, 128:256].bfloat16(), c[:, 256:].bfloat16(), *tabs, B=2, H=2, Sq=4, max_kv=5, D=64, scale=1.0,
                                        q_strides=(4 * 384, 384), k_strides=(8 * 384, 384), v_strides=(8 * 384, 384))
        with pytest.raises(RuntimeError, match="unsupported"):
            hip.attention_offset_ragged(q[:, :128], c[:, 128:256], c[:, 256:], *tabs, B=2, H=1, Sq=4, max_kv=2049, D=128, scale=1.0,
                                        q_strides=(4 * 384, 384), k_strides=(8 * 384, 384), v_strides=(8 * 384, 384))


@needs_emu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_emulated_kv_append_spans(dtype):
    """exact; the q columns, the pad rows, the n = 0 row and the position at max_len untouched; the contract backend restates the same thing"""
    cache, src, pos0, n, S, want = RC.append_case(dtype)
    ref = cache.clone()
    with _hipemu.emulated() as hip:
        hip.kv_append_spans(src, cache, pos0, n, S=S)
    assert torch.equal(cache, want)
    assert torch.equal(cache[2], ref[2]) and torch.equal(cache[:, :, :136], ref[:, :, :136])
    got = ref.clone()
    RC.kv_append_spans(src, got, pos0, n, S=S)
    assert torch.equal(got, want)


def test_contract_matches_the_offset_contract_on_uniform_tables():
    """A sanity check of the TEST HELPER, not coverage of the feature: the new contract (tests/_ragged_extend_case.py) against the backend's own offset
    attention (dense masked softmax) where both are defined.  It runs no project code and passes without the feature."""
    B, H, Sq, P, D = 2, 2, 7, 33, 128
    q, k, v = T("re.q", (B * Sq, H * D), 0.8), T("re.k", (B * (P + Sq), H * D), 0.8), T("re.v", (B * (P + Sq), H * D))
    tabs = torch.tensor([P] * B, dtype=torch.int32), torch.tensor([P + Sq] * B, dtype=torch.int32)
    got = RC.attention_offset_ragged(q, k, v, *tabs, B=B, H=H, Sq=Sq, max_kv=P + Sq, D=D, scale=D ** -0.5)
    want = CB.attention(q, k, v, B=B, H=H, Sq=Sq, Skv=P + Sq, D=D, scale=D ** -0.5, causal=True, q_off=P)
    assert float((got - want).abs().max()) <= 2e-5


# ---- 2. ABI ----------------------------------------------------------------------------------------------------------------------------------------
NEW_ENTRY_POINTS = ("stllm_attention_offset_ragged", "stllm_attention_offset_ragged_workspace_bytes", "stllm_kv_append_spans")


def test_abi_declares_and_exports_the_ragged_extend_entry_points():
    import ctypes
    from stllm_amd import hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "stllm_hip.h")).read()

    class _L:
        pass
    fake = _L()
    for n in hip.EXPORTS:
        setattr(fake, n, _L())
    hip._bind(fake)
    for name in NEW_ENTRY_POINTS:
        assert name in hip.EXPORTS
        decl = re.search(r"^int(?:64_t)? " + name + r"\(([^;]*?)\);", header, re.S | re.M).group(1)
        assert len(getattr(fake, name).argtypes) == len(decl.split(",")), name
    assert fake.stllm_attention_offset_ragged_workspace_bytes.restype is ctypes.c_int64
    if os.path.exists(hip.LIB_PATH):
        L = hip.lib()
        assert L.stllm_abi_version() == 7
        assert all(hasattr(L, n) for n in hip.EXPORTS)
        assert L.stllm_attention_offset_ragged_workspace_bytes(4, 32, 40, 1100) == L.stllm_attention_offset_workspace_bytes(4, 32, 40, 1100) > 0
        assert L.stllm_attention_offset_ragged_workspace_bytes(4, 32, 0, 5) == -1


# ---- 3. LlamaModel.extend on a ragged cache (contract backend, fp32) -------------------------------------------------------------------------------
PREFIXES, SUFFIXES = [9, 4, 6], [5, 0, 3]
UNIFORM_LAYER = ["rmsnorm", "gemm", "attention", "gemm", "rmsnorm", "gemm", "gemm"]                                 # the parent's extend, per layer
RAGGED_LAYER = ["rmsnorm", "gemm", "kv_append_spans", "attention_offset_ragged", "gemm", "rmsnorm", "gemm", "gemm"]


def _suffix_batch(emb, prefixes, suffixes):
    S = max(suffixes)
    new = torch.zeros(len(prefixes), S, emb.shape[2])
    for b, (p, n) in enumerate(zip(prefixes, suffixes)):
        new[b, :n] = emb[b, p:p + n]
    return new


def test_ragged_extend_matches_every_row_alone_and_leaves_an_empty_row_alone():
    from stllm_amd import runtime
    model = small_llama(SMALL)
    lm = model.model
    emb = T("rex.emb", (3, 20, 256), 0.05)
    with RC.installed(), runtime.use_dtype("fp32"):
        rg = RC.ragged_prefix(lm, emb, PREFIXES, 24, "cpu")
        assert rg.lens == PREFIXES
        before = [b.clone() for b in rg.qkv]
        with RC.counting() as calls:
            hid, h16 = lm.extend(_suffix_batch(emb, PREFIXES, SUFFIXES), rg, lengths=SUFFIXES)
            assert calls == ["gather_rows", "gather_rows"] + RAGGED_LAYER * 2 + ["rmsnorm"], calls
        assert rg.lens == [14, 4, 9] and rg.len == 14 and hid.shape == (3, 5, 256) and bool(torch.isfinite(hid).all())
        for x, y in zip(rg.qkv, before):
            assert _poison.bits_equal(x[1], y[1]), "the row that appends nothing is untouched"   # (the rows behind its length are uninitialised: bits, not values)
        for b in (0, 2):
            P, n = PREFIXES[b], SUFFIXES[b]
            cb = lm.new_cache(1, 24, "cpu")
            lm.prefill(emb[b:b + 1, :P], None, cache=cb)
            _, hb = lm.extend(emb[b:b + 1, P:P + n], cb)
            assert torch.allclose(h16.view(3, 5, -1)[b, :n], hb, atol=1e-5), b
            for x, y in zip(rg.qkv, cb.qkv):
                assert torch.allclose(x[b, :P + n, 256:], y[0, :P + n, 256:], atol=1e-5), b
        # a second block behind the now ragged rows, every row full (lengths=None), and an admission into an EMPTY row of a fresh cache
        _, h2 = lm.extend(emb[:, 14:16], rg)
        assert rg.lens == [16, 6, 11]
        fresh = lm.new_cache(2, 24, "cpu")
        _, hf = lm.extend(emb[:2, :6], fresh, lengths=[6, 0])
        assert fresh.lens == [6, 0]
        alone = lm.new_cache(1, 24, "cpu")
        _, ha = lm.prefill(emb[:1, :6], None, cache=alone)
        assert torch.allclose(hf.view(2, 6, -1)[0], ha, atol=1e-5)


def test_ragged_extend_then_decode_matches_the_per_token_loop():
    from stllm_amd import runtime
    model = small_llama(SMALL)
    lm = model.model
    emb = T("rex.emb", (3, 20, 256), 0.05)
    with RC.installed(), runtime.use_dtype("fp32"):
        rg = RC.ragged_prefix(lm, emb, PREFIXES, 24, "cpu")
        lm.extend(_suffix_batch(emb, PREFIXES, SUFFIXES), rg, lengths=SUFFIXES)
        steps = []
        for t in range(2):
            _, h = lm.decode_step(emb[:, 16 + t:17 + t], rg)
            steps.append(h.clone())
        assert rg.lens == [16, 6, 11]
        for b, (P, n) in enumerate(zip(PREFIXES, SUFFIXES)):
            cb = lm.new_cache(1, 24, "cpu")
            lm.prefill(emb[b:b + 1, :P], None, cache=cb)
            for i in range(n):
                lm.decode_step(emb[b:b + 1, P + i:P + i + 1], cb)
            for t in range(2):
                _, hb = lm.decode_step(emb[b:b + 1, 16 + t:17 + t], cb)
                assert torch.allclose(steps[t][b], hb[0], atol=1e-5), (b, t)


def test_every_call_served_before_keeps_its_launches():
    """lengths=None on a uniform cache and lengths=[>= 1 ...] behind a uniform prefix: the call lists of the parent commit, written out"""
    from stllm_amd import runtime
    model = small_llama(SMALL)
    lm = model.model
    emb = T("rex.emb", (3, 20, 256), 0.05)
    with RC.installed(), runtime.use_dtype("fp32"):
        for lengths, lens_after in ((None, None), ([3, 1, 2], [11, 9, 10]), ([3, 3, 3], None)):
            c = lm.new_cache(3, 24, "cpu")
            lm.prefill(emb[:, :8], None, cache=c)
            with RC.counting() as calls:
                lm.extend(emb[:, 8:11], c, lengths=lengths)
                assert calls == UNIFORM_LAYER * 2 + ["rmsnorm"], (lengths, calls)
            assert c.lens == lens_after and c.len == 11


def test_ragged_extend_error_paths():
    from stllm_amd import runtime
    model = small_llama(SMALL)
    lm = model.model
    emb = T("rex.emb", (3, 20, 256), 0.05)
    with RC.installed(), runtime.use_dtype("fp32"):
        base = lm.new_cache(1, 7, "cpu")
        lm.prefill(emb[:1, :7], None, cache=base)
        s = base.share(rows=2, max_new=10)
        with pytest.raises(NotImplementedError, match=r"fork\(\)"):
            lm.extend(emb[:2, 7:10], s, lengths=[3, 0])                 # a row that appends nothing, on a shared base
        lm.extend(emb[:2, 7:10], s, lengths=[3, 1])                     # (the uniform shared path is untouched: it makes the suffix ragged)
        with pytest.raises(NotImplementedError, match=r"fork\(\)"):
            lm.extend(emb[:2, 10:12], s)
        _, h = lm.extend(emb[:2, 10:12], s.fork())                      # ... and forked it goes through
        assert bool(torch.isfinite(h).all())
        rg = RC.ragged_prefix(lm, emb, PREFIXES, 12, "cpu")
        with pytest.raises(AssertionError, match="KV cache full"):
            lm.extend(emb[:, :4], rg)                                   # 9 + 4 > 12
        with pytest.raises(AssertionError):
            lm.extend(emb[:, :2], rg, lengths=[3, 0, 1])                # a length beyond S
    with runtime.use_dtype("bf16x3"), pytest.raises(NotImplementedError, match="bf16x3"):
        lm.extend(emb[:, :2], rg)
    # a backend without the two entry points (the contract backend alone, tensors off the device) says so before anything runs
    from stllm_amd import hip
    assert hip.ragged_extend_available("cpu") is False
    with CB.installed(), runtime.use_dtype("fp32"):
        rg = RC.ragged_prefix(lm, emb, PREFIXES, 24, "cpu")
        before = [b.clone() for b in rg.qkv]
        with pytest.raises(NotImplementedError, match="ragged prefix.*decode_step"):
            lm.extend(emb[:, :2], rg)
        assert rg.lens == PREFIXES and all(_poison.bits_equal(x, y) for x, y in zip(rg.qkv, before))


# ---- 4. generate behind a ragged per-prompt prefix, return_cache (small model, fp32) ---------------------------------------------------------------
# Id-equality cases: seeds vetted on the CPU such that the from-scratch run's top-1 / top-2 margin of the processed scores is >= 1e-2 x max |score| at every
# generated step — 50 x the fp32 model-level bound of 2e-4; every test asserts that precondition itself (scored_runs).
MARGIN = RC.MARGIN
GEN_PREFIXES, GEN_QUESTIONS = [7, 4, 6], [5, 2, 4]


def _gen_inputs():
    video = [T(f"rex.video{i}", (n, 256), 0.05) for i, n in enumerate(GEN_PREFIXES)]
    qs = [T(f"rex.q{i}", (n, 256), 0.05) for i, n in enumerate(GEN_QUESTIONS)]
    return video, qs


def _pad(rows):
    lens = torch.tensor([r.shape[0] for r in rows])
    return torch.nn.utils.rnn.pad_sequence(rows, batch_first=True), (torch.arange(int(lens.max()))[None, :] < lens[:, None]).long()


def test_generate_behind_a_ragged_prefix_equals_every_prompt_alone():
    from stllm_amd import runtime
    model = small_llama(SMALL, lm_head_spread=6.0)
    lm = model.model
    video, qs = _gen_inputs()
    emb, mask = _pad(qs)
    k = dict(max_new_tokens=5, do_sample=False, min_length=1)
    with RC.installed(), runtime.use_dtype("fp32"):
        vemb, _ = _pad(video)
        prefix = RC.ragged_prefix(lm, vemb, GEN_PREFIXES, max(GEN_PREFIXES), "cpu")
        before = [b.clone() for b in prefix.qkv]
        with RC.scored_runs() as scored:
            alone = [model.generate(inputs_embeds=torch.cat([v, q])[None], **k)[0] for v, q in zip(video, qs)]
        assert min(scored) >= MARGIN, ("precondition: the from-scratch runs are not near a tie", min(scored))
        with RC.counting() as calls:
            got = model.generate(inputs_embeds=emb, attention_mask=mask, prefix_cache=prefix, batching="ragged", **k)
            assert calls.count("attention_offset_ragged") == 2 and calls.count("kv_append_spans") == 2
        for i, a in enumerate(alone):
            assert got[i, : a.numel()].tolist() == a.tolist(), i
        assert prefix.lens == GEN_PREFIXES and all(torch.equal(x, y) for x, y in zip(prefix.qkv, before)), "the prefix is left as it was"
        same = model.generate(inputs_embeds=emb[:, :2], prefix_cache=prefix, batching="ragged", **k)   # equal-length questions behind ragged rows
        for i, (v, q) in enumerate(zip(video, qs)):
            assert same[i].tolist() == model.generate(inputs_embeds=torch.cat([v, q[:2]])[None], **k)[0].tolist()
        with pytest.raises(NotImplementedError, match="different lengths"):
            model.generate(inputs_embeds=emb, attention_mask=mask, prefix_cache=prefix, batching="ragged", share_prefix=True, **k)


@pytest.mark.parametrize("selection", ["torch", "device"])
def test_return_cache_holds_every_rows_own_tokens(selection):
    import _select_ref
    from stllm_amd import generation, runtime
    model = small_llama(SMALL, lm_head_spread=6.0)
    lm = model.model
    _, qs = _gen_inputs()
    emb, mask = _pad(qs)
    with RC.installed(), CB._patched({"select_tokens": _select_ref.select_tokens, "beam_candidates": _select_ref.beam_candidates}), runtime.use_dtype("fp32"):
        free = model.generate(inputs_embeds=emb, attention_mask=mask, batching="ragged", max_new_tokens=6, min_length=1)
        stop = [free[0, 1:2].clone()]                          # row 0 ends after two tokens, the others go on (and are fed while it idles)
        assert all(int(stop[0]) not in free[b, :5].tolist() for b in (1, 2)), ("precondition: the stop token separates the rows", free)
        k = dict(max_new_tokens=6, min_length=1, stop_sequences=stop, selection=selection)
        ids, n_gen, cont = model.generate(inputs_embeds=emb, attention_mask=mask, batching="ragged", return_lengths=True, return_cache=True, **k)
        assert isinstance(cont, generation.Continuation) and n_gen[0] == 2 and max(n_gen) == 6
        assert torch.equal(ids, model.generate(inputs_embeds=emb, attention_mask=mask, batching="ragged", **k))
        assert cont.cache.lens == [q.shape[0] + n - 1 for q, n in zip(qs, n_gen)]
        assert cont.pending.tolist() == [int(ids[b, n - 1]) for b, n in enumerate(n_gen)]
        for b, (q, n) in enumerate(zip(qs, n_gen)):
            whole = torch.cat([q, lm.embed_tokens(ids[b:b + 1, :n - 1])[0]])
            fresh = lm.new_cache(1, 16, "cpu")
            lm.prefill(whole[None], None, cache=fresh)
            for x, y in zip(cont.cache.qkv, fresh.qkv):
                L = cont.cache.lens[b]
                assert float((x[b, :L, 256:] - y[0, :L, 256:]).abs().max()) <= RC.MODEL_TOL["fp32"] * float(y[0, :L, 256:].abs().max()), b
        with pytest.raises(NotImplementedError, match="beams"):
            model.generate(inputs_embeds=emb, attention_mask=mask, batching="ragged", num_beams=2, return_cache=True)
        with pytest.raises(ValueError, match="use_cache"):
            model.generate(inputs_embeds=emb[:1], use_cache=False, return_cache=True)


# ---- 5. Chat.answer_many(keep=True) + follow_up ----------------------------------------------------------------------------------------------------
CFG = dict(vit_model="eva_clip_g", image_size=224, num_query_token=32, video_input="mean", use_mask=False, mvm_decode=False,
           qformer_text_input=False, max_txt_len=32, end_sym=" 2")


@pytest.fixture(scope="module")
def stllm():
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
    m.lm_head.weight.mul_(6.0)   # spread the logits so that the rows take different paths (tests/test_ragged_cpu.py)
    return m


def test_chat_follow_up_equals_the_from_scratch_concatenation(stllm):
    """three questions of different lengths about one video, then a second turn of different lengths: every row's second answer is what generate() gives
    for that row alone on [video, BOS + question, answer 1, turn 2] prefilled from scratch — the dialogue lives on the generated ids"""
    from stllm_amd import runtime
    from stllm_amd.conversation import Chat, Dialogue
    model = stllm
    frames = T("input.frames2", (2, 3, 224, 224))
    questions, turns = RC.CHAT_QUESTIONS, RC.CHAT_TURNS
    k = dict(max_new_tokens=4, num_beams=1)
    with RC.installed(), runtime.use_dtype("fp32"):
        chat = Chat(model, device="cpu")
        img_list = []
        chat.upload_video(frames.view(6, 224, 224), None, img_list)
        prefix = chat.prefill_video(img_list)
        with RC.scored_runs() as scored:
            want1 = [chat.answer(img_list, q, **k) for q in questions]
        first, dlg = chat.answer_many(img_list, questions, prefix=prefix, keep=True, **k)
        assert isinstance(dlg, Dialogue) and dlg.cache.batch == 3
        for (t0, i0), (t1, i1) in zip(want1, first):
            assert np.array_equal(i0, i1) and t0 == t1
        raw1 = chat.LLM.generate(inputs_embeds=torch.nn.utils.rnn.pad_sequence([chat.get_context_emb_ids(img_list, q)[0][0] for q in questions], batch_first=True),
                                 attention_mask=(torch.arange(38)[None, :] < torch.tensor([32 + 1 + len(q) for q in questions])[:, None]).long(),
                                 batching="ragged", return_lengths=True, repetition_penalty=1.5, min_length=1, stop_sequences=chat.stopping_criteria[0].stops, **k)
        ids1 = [row[:n].tolist() for row, n in zip(*raw1)]           # the generated ids of turn 1, before _decoded strips a leading <unk> / <s>
        assert dlg.pending.tolist() == [i[-1] for i in ids1]
        nv = img_list[0].shape[1]
        assert dlg.cache.lens == [nv + 1 + len(q) + len(i) - 1 for q, i in zip(questions, ids1)]
        with RC.counting() as calls:
            second = chat.follow_up(dlg, turns, **k)
            assert calls.count("attention_offset_ragged") == 2 and calls.count("kv_append_spans") == 2, "one ragged extend, no prefill of the history"
        assert dlg.turns == 2
        with RC.scored_runs() as scored2:
            for b in range(3):
                whole = torch.cat([chat.get_context_emb_ids(img_list, questions[b])[0][0], chat.model.embed_tokens(torch.tensor([ids1[b] + turns[b]]))[0]])
                ref = chat.LLM.generate(inputs_embeds=whole[None], repetition_penalty=1.5, min_length=1, stop_sequences=chat.stopping_criteria[0].stops, **k)
                assert np.array_equal(chat._decoded(ref[0])[1], second[b][1]), (b, ref, second[b])
        assert min(scored + scored2) >= MARGIN, ("precondition: the from-scratch runs are not near a tie", min(scored + scored2))
        # a third turn, one token each; then a turn that does not fit the model's positions
        third = chat.follow_up(dlg, [[5], [6], [7]], **k)
        assert len(third) == 3 and dlg.turns == 3
        with pytest.raises(ValueError, match="limit"):
            chat.follow_up(dlg, turns, max_new_tokens=2048)
    tk, seen = chat.model.llama_tokenizer, []
    orig = tk.encode_ids
    tk.encode_ids = lambda text, add_special_tokens=True: seen.append((text, add_special_tokens)) or orig(text, add_special_tokens)
    try:
        assert chat.turn_ids("7 8") == [7, 8] == chat.turn_ids("7 8", closed=False)   # (the test tokenizer keeps the numbers only)
    finally:
        del tk.encode_ids
    assert seen == [("Human: 7 8 ###Assistant: ", False), ("###Human: 7 8 ###Assistant: ", False)]
