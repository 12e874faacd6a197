"""CPU: the prefix KV cache — attention with a query offset, LlamaModel.extend, KVCache.fork / truncate, generate(prefix_cache=...), Chat.prefill_video /
answer(prefix=...) — on the test-only contract backend (tests/_cpu_backend.py, fp32), plus the offset attention kernels themselves on the host
emulator (tests/hipemu) and the C ABI surface."""
import os
import re

import numpy as np
import pytest
import torch

import _cpu_backend as CB
import _hipemu
from _util import T, golden

torch.set_grad_enabled(False)
TOL = 2e-4   # x logits abs-max: the fp32 bound of tests/test_model_gpu.py::test_kv_cache_decode_matches_reprefill for the same kind of comparison
CFG = dict(vit_model="eva_clip_g", image_size=224, num_query_token=32, video_input="mean", use_mask=False, mvm_decode=False,
           qformer_text_input=False, max_txt_len=32, end_sym=" 2")


def dense_ref(q, k, v, B, H, Sq, Skv, D, q_off, causal=True, lens=None):
    """softmax(scale Q K^T + mask) V in fp64 with the mask written out densely: key j visible to query i iff j <= q_off + i (and j < lens[b])"""
    q = q.double().view(B, Sq, H, D).transpose(1, 2)
    k = k.double().view(B, Skv, H, D).transpose(1, 2)
    v = v.double().view(B, Skv, H, D).transpose(1, 2)
    s = q @ k.transpose(-1, -2) * D ** -0.5
    if causal:
        s = s.masked_fill(torch.arange(Skv)[None, :] > torch.arange(Sq)[:, None] + q_off, float("-inf"))
    if lens is not None:
        for b, n in enumerate(lens):
            s[b, :, :, n:] = float("-inf")
    return (s.softmax(-1) @ v).transpose(1, 2).reshape(B * Sq, H * D)


OFFSET_CASES = [(1, 2, 1, 70, 71, None), (1, 2, 48, 0, 48, None), (2, 1, 7, 33, 40, None), (1, 2, 40, 200, 240, None),
                (1, 1, 20, 30, 90, None),                       # q_off + Sq < Skv: keys behind the last query stay invisible
                (2, 1, 40, 100, 140, [140, 120])]               # kv_len


@pytest.mark.parametrize("B,H,Sq,q_off,Skv,lens", OFFSET_CASES)
def test_offset_attention_contract_matches_dense_masked_softmax(B, H, Sq, q_off, Skv, lens):
    D = 128
    q, k, v = T("pc.q", (B * Sq, H * D), 0.8), T("pc.k", (B * Skv, H * D), 0.8), T("pc.v", (B * Skv, H * D))
    kl = None if lens is None else torch.tensor(lens, dtype=torch.int32)
    got = CB.attention(q, k, v, B=B, H=H, Sq=Sq, Skv=Skv, D=D, scale=D ** -0.5, causal=True, kv_len=kl, q_off=q_off)
    want = dense_ref(q, k, v, B, H, Sq, Skv, D, q_off, lens=lens)
    assert float((got.double() - want).abs().max()) <= 2e-5


@pytest.mark.skipif(not _hipemu.available() or _hipemu.ON_DEVICE, reason="host emulation of the kernel sources needs ROCm's clang++")
@pytest.mark.parametrize("dtype,tol", [(torch.bfloat16, 2 * 2.0 ** -8), (torch.float16, 2 * 2.0 ** -10), (torch.float32, 2e-5)])
def test_offset_attention_kernels_emulated(dtype, tol):
    """the kernels of stllm_attention_offset compiled for the host (tests/hipemu): the tile kernels with the offset and the key-split pair, forced on and
    off, against the dense fp64 reference; q_off = 0 through hip.attention is stllm_attention as before"""
    D = 128
    with _hipemu.emulated() as hip:
        try:
            for B, H, Sq, q_off, Skv, lens in [(1, 2, 40, 200, 240, None), (2, 1, 7, 33, 40, None), (1, 1, 1, 70, 71, None), (2, 1, 40, 100, 140, [140, 120]),
                                               (1, 1, 130, 300, 430, None)]:
                q, k, v = T("pc.q", (B * Sq, H * D), 0.8, dtype=dtype), T("pc.k", (B * Skv, H * D), 0.8, dtype=dtype), T("pc.v", (B * Skv, H * D), dtype=dtype)
                if q_off == 200:
                    k[230] = (q[5] * 6).to(dtype)      # a late dominating key in the last key range: the merge has to rescale the earlier ranges
                want = dense_ref(q, k, v, B, H, Sq, Skv, D, q_off, lens=lens)
                kl = None if lens is None else torch.tensor(lens, dtype=torch.int32)
                for opt in (0, 1):
                    hip.set_option("attn_ksplit", opt)
                    got = hip.attention(q, k, v, B=B, H=H, Sq=Sq, Skv=Skv, D=D, scale=D ** -0.5, causal=True, kv_len=kl, q_off=q_off)
                    ran = hip.lib().stllm_last_kernel().decode()
                    assert ("ksplit" in ran) == (opt == 1 and dtype != torch.float32), (ran, opt)
                    err = float((got.double() - want).abs().max())
                    assert err <= tol, (dtype, (B, H, Sq, q_off, Skv), ran, err)
        finally:
            hip.set_option("attn_ksplit", -1)
        with pytest.raises(RuntimeError, match="q_off"):
            hip.attention(q, k, v, B=B, H=H, Sq=Sq, Skv=Skv, D=D, scale=D ** -0.5, causal=True, q_off=Skv - Sq + 1)


@pytest.fixture(scope="module")
def llm():
    from stllm_amd import synth
    from stllm_amd.models.st_llm import STLLMForCausalLM, StllmConfig
    m = STLLMForCausalLM(StllmConfig(num_hidden_layers=2), device="cpu")
    synth.fill_module_(m, 0, "")
    return m


def _last_logits(model, h16, B, S):
    return model.logits_from(h16.view(B, S, -1)[:, -1].contiguous(), B, 1)[:, 0]


def test_extend_matches_prefill_of_the_whole_prompt(llm):
    from stllm_amd import runtime
    lm = llm.model
    B, Sa, Sb = 2, 11, 9
    emb = T("input.inputs_embeds", (B, Sa + Sb, 4096), 0.05)
    a, b = emb[:, :Sa], emb[:, Sa:]
    with CB.installed(), runtime.use_dtype("fp32"):
        whole = lm.new_cache(B, 32, "cpu")
        _, h = lm.prefill(emb, None, cache=whole)
        want = _last_logits(llm, h, B, Sa + Sb)
        one = lm.new_cache(B, 32, "cpu")
        lm.prefill(a, None, cache=one)
        hid, h = lm.extend(b, one)
        got1 = _last_logits(llm, h, B, Sb)
        two = lm.new_cache(B, 32, "cpu")
        lm.prefill(a, None, cache=two)
        lm.extend(b[:, :4], two)
        _, h = lm.extend(b[:, 4:], two)
        got2 = _last_logits(llm, h, B, Sb - 4)
        empty = lm.new_cache(B, 32, "cpu")
        _, h = lm.extend(emb, empty)                      # P = 0: a plain prefill
        assert torch.equal(_last_logits(llm, h, B, Sa + Sb), want) and empty.len == Sa + Sb
        with pytest.raises(AssertionError):
            lm.extend(emb, one)                           # 20 + 20 > 32
    assert hid.shape == (B, Sb, 4096) and one.len == two.len == whole.len == Sa + Sb
    scale = float(want.abs().max())
    for got, c in ((got1, one), (got2, two)):
        assert float((got - want).abs().max()) <= TOL * scale
        for x, y in zip(c.qkv, whole.qkv):
            assert float((x[:, :Sa + Sb] - y[:, :Sa + Sb]).abs().max()) <= TOL * float(y[:, :Sa + Sb].abs().max())


def test_extend_then_decode_matches_token_by_token_forward(llm):
    from stllm_amd import runtime
    lm = llm.model
    B, Sa, Sb, n_new = 2, 8, 5, 3
    emb = T("input.inputs_embeds", (B, Sa + Sb + n_new, 4096), 0.05)
    with CB.installed(), runtime.use_dtype("fp32"):
        c1 = lm.new_cache(B, 24, "cpu")
        lm.prefill(emb[:, :Sa], None, cache=c1)
        _, h = lm.extend(emb[:, Sa:Sa + Sb], c1)
        got = [_last_logits(llm, h, B, Sb)]
        for t in range(n_new):
            _, h = lm.decode_step(emb[:, Sa + Sb + t:Sa + Sb + t + 1], c1)
            got.append(llm.logits_from(h, B, 1)[:, 0])
        c2 = lm.new_cache(B, 24, "cpu")
        lm.prefill(emb[:, :Sa], None, cache=c2)
        o = lm(inputs_embeds=emb[:, Sa:Sa + Sb], past_key_values=c2)       # the per-token loop
        want = [llm.logits_from(o._h16, B, 1)[:, 0]]
        for t in range(n_new):
            o = lm(inputs_embeds=emb[:, Sa + Sb + t:Sa + Sb + t + 1], past_key_values=c2)
            want.append(llm.logits_from(o._h16, B, 1)[:, 0])
    assert c1.len == c2.len == Sa + Sb + n_new
    scale = max(float(w.abs().max()) for w in want)
    for g, w in zip(got, want):
        assert float((g - w).abs().max()) <= TOL * scale


def test_stack_entry_equals_per_op_body_and_lora_active_equals_merged(llm, monkeypatch):
    from stllm_amd import runtime
    from stllm_amd.models import llama as llama_mod
    from stllm_amd.models.st_llm import STLLMForCausalLM, StllmConfig
    from stllm_amd import synth
    lm = llm.model
    emb = T("input.inputs_embeds", (1, 14, 4096), 0.05)

    def run(model):
        c = model.model.new_cache(1, 16, "cpu")
        model.model.prefill(emb[:, :8], None, cache=c)
        _, h = model.model.extend(emb[:, 8:], c)
        return h.clone(), c
    with CB.installed(), runtime.use_dtype("fp32"):
        h_stack, c_stack = run(llm)
        monkeypatch.setattr(llama_mod, "STACK_ENTRY", False)
        h_op, c_op = run(llm)
        monkeypatch.setattr(llama_mod, "STACK_ENTRY", True)
        assert torch.equal(h_stack, h_op) and all(torch.equal(x[:, :14], y[:, :14]) for x, y in zip(c_stack.qkv, c_op.qkv))
        m = STLLMForCausalLM(StllmConfig(num_hidden_layers=2), device="cpu")
        synth.fill_module_(m, 0, "")
        m.add_lora(16, 32)
        for i, mod in enumerate(m._lora_modules()):
            mod.B.copy_(T(f"lora.B{i}", tuple(mod.B.shape), 0.02))
        h_act, _ = run(m)
        assert not torch.equal(h_act, h_stack), "the adapters must move the result"
        m.merge_adapter()
        h_mrg, _ = run(m)
    assert float((h_act - h_mrg).abs().max()) <= TOL * float(h_mrg.abs().max())
    with runtime.use_dtype("bf16x3"), pytest.raises(NotImplementedError, match="bf16x3"):
        lm.extend(emb[:, 8:], c_stack)


def test_kv_cache_fork_and_truncate(llm):
    from stllm_amd.models.llama import KVCache
    c = KVCache(2, 2, 10, 8, torch.float32, "cpu")
    for i, b in enumerate(c.qkv):
        b.copy_(torch.arange(b.numel()).view_as(b).float() + 1000 * i)
    c.len = 6
    f = c.fork(rows=6, max_len=12)
    assert f.len == 6 and f.batch == 6 and f.max_len == 12 and len(f.qkv) == 2
    for src, dst in zip(c.qkv, f.qkv):
        assert torch.equal(dst[:, :6], src[:, :6].repeat_interleave(3, dim=0))       # what generation's stepper does by hand for the beams
    same = c.fork()
    assert same.batch == 2 and same.max_len == 10 and all(torch.equal(x[:, :6], y[:, :6]) and x.data_ptr() != y.data_ptr() for x, y in zip(c.qkv, same.qkv))
    f.truncate(4)
    assert f.len == 4 and c.len == 6
    with pytest.raises(AssertionError):
        f.truncate(5)
    with pytest.raises(AssertionError):
        c.fork(rows=3)


def _build(cfg, vit_depth=1, qf_layers=2, llm_layers=2):
    from stllm_amd import synth
    from stllm_amd.models import st_llm
    from stllm_amd.models.blip2 import Blip2Base
    from stllm_amd.tokenizer import IdTokenizer
    old = (Blip2Base.vit_depth, Blip2Base.qformer_layers, Blip2Base.init_tokenizer)
    Blip2Base.vit_depth, Blip2Base.qformer_layers = vit_depth, qf_layers
    Blip2Base.init_tokenizer = classmethod(lambda cls, truncation_side="right": IdTokenizer(0, 1, 2, 32000))
    try:
        m = st_llm.STLLMForCausalLM.from_config(dict(cfg, llama_model=dict(num_hidden_layers=llm_layers)), device="cpu")
    finally:
        Blip2Base.vit_depth, Blip2Base.qformer_layers, Blip2Base.init_tokenizer = old
    synth.fill_module_(m, 0, "")
    return m


@pytest.fixture(scope="module")
def stllm():
    return _build(CFG)


def test_generate_behind_a_prefix_matches_reference_fixture(stllm):
    """tests/golden/generate.npz: ids of the REFERENCE's generate for 9-embedding prompts.  Split as prefix 5 + suffix 4, generate(prefix_cache=...) must
    return the same ids — twice on the same prefix object, whose bytes and length stay what they were."""
    from stllm_amd import runtime
    g = golden("generate")
    model = stllm
    w0 = model.lm_head.weight.detach().clone()
    modes = [dict(num_beams=1), dict(num_beams=5), dict(num_beams=3, repetition_penalty=1.3, length_penalty=2.0)]
    try:
        with CB.installed(), runtime.use_dtype("fp32"):
            for scale, seed in [(4.0, 3), (4.0, 4), (8.0, 4), (8.0, 5)]:
                model.lm_head.weight.copy_(w0 * scale)
                model._lm_packed = {}
                emb = T(f"gen.emb{seed}", (1, 9, 4096), 0.05)
                prefix = model.model.new_cache(1, 5, "cpu")
                model.model.prefill(emb[:, :5], None, cache=prefix)
                before = [b.clone() for b in prefix.qkv]
                for mi, kw in enumerate(modes):
                    k = dict(dict(max_new_tokens=6, do_sample=False, min_length=1, top_p=0.9, repetition_penalty=1.0, length_penalty=1,
                                  temperature=1.0), **kw)
                    for again in range(2):
                        ids = model.generate(inputs_embeds=emb[:, 5:], prefix_cache=prefix, **k)[0].tolist()
                        assert ids == g[f"s{scale:g}_p{seed}_m{mi}"].tolist(), (scale, seed, kw, again, ids)
                        assert prefix.len == 5 and all(torch.equal(x, y) for x, y in zip(prefix.qkv, before))
            with pytest.raises(NotImplementedError, match="prefix"):
                e2 = T("gen.emb3", (2, 4, 4096), 0.05)
                model.generate(inputs_embeds=e2, attention_mask=torch.tensor([[1, 1, 1, 1], [1, 1, 0, 0]]), prefix_cache=prefix)
    finally:
        model.lm_head.weight.copy_(w0)
        model._lm_packed = {}


def test_chat_answers_two_questions_on_one_video_prefix(stllm):
    from stllm_amd import runtime
    from stllm_amd.conversation import Chat
    model = stllm
    frames = T("input.frames2", (2, 3, 224, 224))
    with CB.installed(), runtime.use_dtype("fp32"):
        chat = Chat(model, device="cpu")
        img_list = []
        chat.upload_video(frames.view(6, 224, 224), None, img_list)
        prefix = chat.prefill_video(img_list)
        nv = img_list[0].shape[1]
        assert prefix.n_tokens == nv == prefix.cache.len
        before = [b.clone() for b in prefix.cache.qkv]
        for question in ([21, 22, 23], [400, 17, 9000, 5, 77]):
            kw = dict(max_new_tokens=4, num_beams=3, do_sample=False)
            text0, ids0 = chat.answer(img_list, question, **kw)
            text1, ids1 = chat.answer(img_list, question, prefix=prefix, **kw)
            assert np.array_equal(ids0, ids1) and text0 == text1, (question, ids0, ids1)
            assert prefix.cache.len == nv and all(torch.equal(x, y) for x, y in zip(prefix.cache.qkv, before))
        # the reference's truncation rule (keep the last max_length - max_new_tokens embeddings) would cut into the cached positions: the uncached path
        kw = dict(max_new_tokens=4, max_length=nv + 2, num_beams=1)
        text0, ids0 = chat.answer(img_list, [21, 22, 23], **kw)
        text1, ids1 = chat.answer(img_list, [21, 22, 23], prefix=prefix, **kw)
        assert np.array_equal(ids0, ids1)


def test_abi_exports_and_header():
    from stllm_amd import hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "stllm_hip.h")).read()
    for name in ("stllm_attention_offset", "stllm_attention_offset_workspace_bytes", "stllm_llama_layers_extend"):
        assert name in hip.EXPORTS
        assert re.search(r"\b" + name + r"\(", header), name
    if os.path.exists(hip.LIB_PATH):
        L = hip.lib()
        assert L.stllm_abi_version() == 7
        assert all(hasattr(L, n) for n in hip.EXPORTS)
        assert L.stllm_attention_offset_workspace_bytes(1, 32, 40, 2088) > 0 and L.stllm_attention_offset_workspace_bytes(1, 32, 0, 5) == -1
