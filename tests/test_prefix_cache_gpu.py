"""GPU (-m gpu): the prefix KV cache on the device — stllm_attention_offset (offset tile kernels and the key-split kernel pair, forced on and off),
LlamaModel.extend against the whole-prompt prefill and the per-token loop, the C stack entry against the per-op body, generate(prefix_cache=...)
against the reference's ids (tests/golden/generate.npz) and Chat.answer(prefix=...)."""
import numpy as np
import pytest
import torch

import _poison

from _util import T, golden

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
OUT_TOL = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -10, "fp32": 2e-5}   # tests/test_kernels_gpu.py


@pytest.fixture(scope="module")
def hip():
    from stllm_amd import hip as h
    h.lib()
    return h


def check(got, ref, tol, what):
    got = got.detach().double().cpu()
    ref = ref.double()
    assert got.shape == ref.shape, f"{what}: {got.shape} vs {ref.shape}"
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    scale = max(ref.abs().max().item(), 1e-6)
    err = (got - ref).abs().max().item()
    print(f"[{what}] max err {err:.3e} (bound {tol:.1e} x {scale:.3e})")
    assert err <= tol * scale, f"{what}: max err {err:.3e} > {tol:.1e} * {scale:.3e}"


def dense_ref(q, k, v, q_off):
    """fp64 softmax(scale Q K^T + mask) V, q [B, Sq, H, D], k / v [B, Skv, H, D]; key j visible to query i iff j <= q_off + i"""
    B, Sq, H, D = q.shape
    Skv = k.shape[1]
    s = q.transpose(1, 2) @ k.transpose(1, 2).transpose(-1, -2) * D ** -0.5
    s = s.masked_fill(torch.arange(Skv)[None, :] > torch.arange(Sq)[:, None] + q_off, float("-inf"))
    return (s.softmax(-1) @ v.transpose(1, 2)).transpose(1, 2).reshape(B * Sq, H * D)


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("Sq,q_off", [(40, 512), (96, 2048), (7, 33), (200, 200), (1, 700)])
def test_offset_attention_matches_fp64(hip, dtype, Sq, q_off):
    """B = 2, operands inside one fused cache buffer [B, max_len, 3 hidden] with the strides decode_step passes; the key-split pair forced on, forced off
    and the automatic choice; a late dominating key in the last key range makes the merge rescale every earlier range."""
    td = hip.torch_dtype(dtype)
    B, H, D = 2, 4, 128
    HD, Skv = H * D, q_off + Sq
    ML = Skv + 5
    buf = T("pc.cache", (B, ML, 3 * HD), 1.0)
    buf[..., :2 * HD] *= 0.3
    buf = buf.to(td)
    buf[:, q_off + min(3, Sq - 1), HD:2 * HD] = (buf[:, q_off + Sq - 1, :HD].float() * 6).to(td)   # visible to the last query row(s) only
    q64 = buf[:, q_off:Skv, :HD].double().view(B, Sq, H, D)
    k64 = buf[:, :Skv, HD:2 * HD].double().view(B, Skv, H, D)
    v64 = buf[:, :Skv, 2 * HD:].double().view(B, Skv, H, D)
    ref = dense_ref(q64, k64, v64, q_off)
    buf[:, Skv:] = float("nan")                  # the cache rows at or behind Skv are never read (include/stllm_hip.h: memory regions)
    dbuf = buf.cuda()
    full = dbuf.view(B * ML, 3 * HD)
    st = (ML * 3 * HD, 3 * HD)
    tol = 2 * OUT_TOL[dtype] if dtype != "fp32" else 2e-5
    try:
        for opt in (0, 1, -1):
            hip.set_option("attn_ksplit", opt)
            g = _poison.Guarded(B * Sq, HD, td, device="cuda")            # the output inside a 0xFF-filled buffer: rows around it, columns [HD, ldo)
            with _poison.poisoned_allocations() as counts:                 # the key-split workspace "needs no initialisation": 0xFF in every byte
                out = hip.attention(full[q_off:, :HD], full[:, HD:2 * HD], full[:, 2 * HD:], B=B, H=H, Sq=Sq, Skv=Skv, D=D, scale=D ** -0.5, causal=True,
                                    q_strides=st, k_strides=st, v_strides=st, q_off=q_off, out=g.out)
            assert g.intact(), "a byte outside the output rows was written"
            assert counts.allocations > 0 or dtype == "fp32"
            ran = hip.lib().stllm_last_kernel().decode()
            if dtype == "fp32":
                assert ran in ("attn_mfma_f32_kernel", "attn_f32_kernel"), ran
            elif opt >= 0:
                assert ran == ("attn_ksplit_kernel" if opt else "attn_mfma_kernel"), (opt, ran)
            check(out, ref, tol, f"offset attention {dtype} Sq={Sq} q_off={q_off} attn_ksplit={opt} -> {ran}")
    finally:
        hip.set_option("attn_ksplit", -1)
    assert _poison.bits_equal(dbuf.cpu(), buf), "the cache buffer is read-only for the attention"


def _last_logits(model, h16, B, S):
    return model.logits_from(h16.view(B, S, -1)[:, -1].contiguous(), B, 1)[:, 0]


@pytest.mark.parametrize("mode,tol", [("fp32", 2e-4), ("bf16", 5e-2), ("fp16", 5e-2)])
def test_extend_matches_prefill_and_per_token_loop(mode, tol, monkeypatch):
    """the set-up of test_model_gpu.py::test_kv_cache_decode_matches_reprefill (B = 2, 3 layers, full width) and its bounds: prefill(A|B) vs
    prefill(A) + extend(B) vs prefill(A) + extend(B1) + extend(B2); extend + decode steps vs forward(past_key_values=...) token by token; the C stack
    entry vs the per-op body, bit for bit."""
    from stllm_amd import runtime, synth
    from stllm_amd.models import llama as llama_mod
    from stllm_amd.models.st_llm import STLLMForCausalLM, StllmConfig
    model = STLLMForCausalLM(StllmConfig(num_hidden_layers=3), device="cuda")
    synth.fill_module_(model, 0, "")
    lm = model.model
    B, Sa, Sb, n_new = 2, 37, 21, 3
    emb = T("input.inputs_embeds", (B, Sa + Sb + n_new, 4096), 0.05).cuda()
    a, b, new = emb[:, :Sa], emb[:, Sa:Sa + Sb], emb[:, Sa + Sb:]
    ML = Sa + Sb + n_new
    with runtime.use_dtype(mode):
        whole = lm.new_cache(B, ML, "cuda")
        _, h = lm.prefill(emb[:, :Sa + Sb], None, cache=whole)
        want = _last_logits(model, h, B, Sa + Sb)
        one = lm.new_cache(B, ML, "cuda")
        lm.prefill(a, None, cache=one)
        _, h1 = lm.extend(b, one)
        got1 = _last_logits(model, h1, B, Sb)
        two = lm.new_cache(B, ML, "cuda")
        lm.prefill(a, None, cache=two)
        lm.extend(b[:, :8], two)
        _, h = lm.extend(b[:, 8:], two)
        got2 = _last_logits(model, h, B, Sb - 8)
        # per-op body == C stack entry
        monkeypatch.setattr(llama_mod, "STACK_ENTRY", False)
        op = lm.new_cache(B, ML, "cuda")
        lm.prefill(a, None, cache=op)
        _, h_op = lm.extend(b, op)
        monkeypatch.setattr(llama_mod, "STACK_ENTRY", True)
        assert torch.equal(h_op, h1) and all(torch.equal(x[:, :Sa + Sb], y[:, :Sa + Sb]) for x, y in zip(op.qkv, one.qkv))
        # extend + decode steps vs the per-token loop
        steps = []
        for t in range(n_new):
            _, h = lm.decode_step(new[:, t:t + 1], one)
            steps.append(model.logits_from(h, B, 1)[:, 0])
        loop = lm.new_cache(B, ML, "cuda")
        lm.prefill(a, None, cache=loop)
        o = lm(inputs_embeds=b, past_key_values=loop)
        loop_logits = [model.logits_from(o._h16, B, 1)[:, 0]]
        for t in range(n_new):
            o = lm(inputs_embeds=new[:, t:t + 1], past_key_values=loop)
            loop_logits.append(model.logits_from(o._h16, B, 1)[:, 0])
    assert one.len == loop.len == ML and two.len == whole.len == Sa + Sb
    scale = float(want.abs().max())
    for name, got in (("extend(B)", got1), ("extend(B1) + extend(B2)", got2), ("per-token loop", loop_logits[0])):
        err = float((got - want).abs().max())
        print(f"[{mode}] {name} vs whole prefill: logits err {err:.3e} (bound {tol:.0e} x {scale:.2f})")
        assert err <= tol * scale, (name, err, scale)
    for c in (two,):
        for x, y in zip(c.qkv, whole.qkv):
            err = float((x[:, :Sa + Sb].float() - y[:, :Sa + Sb].float()).abs().max())
            assert err <= tol * float(y[:, :Sa + Sb].float().abs().max()), ("cache rows", err)
    for t, (g, w) in enumerate(zip([got1] + steps, loop_logits)):
        err = float((g - w).abs().max())
        assert err <= tol * scale, f"step {t}: extend + decode vs per-token loop {err:.3e}"


def _build_stllm(cfg, vit_depth=1, qf_layers=2, llm_layers=2):
    from stllm_amd import synth
    from stllm_amd.models import st_llm
    from stllm_amd.models.blip2 import Blip2Base
    from stllm_amd.tokenizer import IdTokenizer
    old = (Blip2Base.vit_depth, Blip2Base.qformer_layers, Blip2Base.init_tokenizer)
    Blip2Base.vit_depth, Blip2Base.qformer_layers = vit_depth, qf_layers
    Blip2Base.init_tokenizer = classmethod(lambda cls, truncation_side="right": IdTokenizer(0, 1, 2, 32000))
    try:
        m = st_llm.STLLMForCausalLM.from_config(dict(cfg, llama_model=dict(num_hidden_layers=llm_layers)), device="cuda")
    finally:
        Blip2Base.vit_depth, Blip2Base.qformer_layers, Blip2Base.init_tokenizer = old
    synth.fill_module_(m, 0, "")
    return m


def test_generate_behind_a_prefix_on_device_matches_reference_ids():
    """tests/golden/generate.npz (ids of the REFERENCE's generate) with every 9-embedding prompt split as prefix 5 + suffix 4: the same ids in fp32, twice on
    one prefix object that stays untouched; Chat.answer(prefix=...) == Chat.answer() with 5 beams for two questions in a row; bf16 / fp16: valid ids."""
    from stllm_amd import hip, runtime
    from stllm_amd.conversation import Chat
    g = golden("generate")
    cfg = dict(vit_model="eva_clip_g", image_size=224, num_query_token=32, video_input="mean", use_mask=False, mvm_decode=False,
               qformer_text_input=False, max_txt_len=32, end_sym=" 2")
    model = _build_stllm(cfg)
    w0 = model.lm_head.weight.detach().clone()
    modes = [dict(num_beams=1), dict(num_beams=5), dict(num_beams=3, repetition_penalty=1.3, length_penalty=2.0)]
    with runtime.use_dtype("fp32"):
        for scale, seed in [(4.0, 3), (4.0, 4), (8.0, 4), (8.0, 5)]:
            model.lm_head.weight.copy_(w0 * scale)
            emb = T(f"gen.emb{seed}", (1, 9, 4096), 0.05).cuda()
            prefix = model.model.new_cache(1, 5, "cuda")
            model.model.prefill(emb[:, :5], None, cache=prefix)
            before = [b.clone() for b in prefix.qkv]
            for mi, kw in enumerate(modes):
                k = dict(dict(max_new_tokens=6, do_sample=False, min_length=1, top_p=0.9, repetition_penalty=1.0, length_penalty=1,
                              temperature=1.0), **kw)
                for again in range(2):
                    ids = model.generate(inputs_embeds=emb[:, 5:], prefix_cache=prefix, **k)[0].tolist()
                    assert ids == g[f"s{scale:g}_p{seed}_m{mi}"].tolist(), (scale, seed, kw, again, ids)
                    assert prefix.len == 5 and all(torch.equal(x, y) for x, y in zip(prefix.qkv, before))
        chat = Chat(model, device="cuda")
        img_list = []
        chat.upload_video(T("input.frames2", (2, 3, 224, 224)).view(6, 224, 224).cuda(), None, img_list)
        vp = chat.prefill_video(img_list)
        for question in ([21, 22, 23], [400, 17, 9000, 5, 77]):
            _, ids0 = chat.answer(img_list, question, max_new_tokens=5, num_beams=5, do_sample=False)
            _, ids1 = chat.answer(img_list, question, max_new_tokens=5, num_beams=5, do_sample=False, prefix=vp)
            assert np.array_equal(ids0, ids1), (question, ids0, ids1)
        assert vp.cache.len == img_list[0].shape[1]
    for mode in ("bf16", "fp16"):
        with runtime.use_dtype(mode):
            model.model.repack()
            model._lm_packed = {}
            emb = T("gen.emb3", (1, 9, 4096), 0.05).cuda()
            prefix = model.model.new_cache(1, 5, "cuda")
            model.model.prefill(emb[:, :5], None, cache=prefix)
            out = model.generate(inputs_embeds=emb[:, 5:], prefix_cache=prefix, max_new_tokens=6, num_beams=5, min_length=1)
            assert out.shape[0] == 1 and 1 <= out.shape[1] <= 6 and int(out.max()) < 32000 and prefix.len == 5
    assert hip.gemm_workspace_ok()
