"""CPU: the host side of the LoRA adapters (models/lora.py, LlamaModel with active adapters, checkpoint key layouts, rejections) on the
test-only contract backend (tests/_cpu_backend.py), against the reference-pinned oracle fed with `W + s·B·A` (fp64) as a plain weight.
peft is not available: there is no reference fixture for this branch."""
import os

import pytest
import torch

import _cpu_backend as CB
import stllm_oracle as O
from _util import T

torch.set_grad_enabled(False)
TOL = 2e-4   # the fp32 tolerance of tests/test_model_gpu.py MODES (the contract backend computes in fp32)
CFG = dict(vit_model="eva_clip_g", image_size=224, num_query_token=32, video_input="mean", use_mask=False, mvm_decode=False,
           qformer_text_input=False, max_txt_len=32, end_sym=" 2")


def llm(n_layers=2, r=0, b_std=0.0, alpha=32):
    from stllm_amd import synth
    from stllm_amd.models.st_llm import STLLMForCausalLM, StllmConfig
    m = STLLMForCausalLM(StllmConfig(num_hidden_layers=n_layers), device="cpu")
    synth.fill_module_(m, 0, "")
    if r:
        m.add_lora(r, alpha)
        for i, mod in enumerate(m._lora_modules()):
            mod.B.copy_(T(f"lora.B{i}", tuple(mod.B.shape), b_std))
    return m


def oracle_sds(m):
    base, mg = {}, {}
    for k, v in m.state_dict().items():
        if "lora_" not in k:
            base[k.replace(".base_layer.", ".")] = mg[k.replace(".base_layer.", ".")] = v.detach().float()
    for li, l in enumerate(m.model.layers):
        for t in ("q_proj", "v_proj"):
            mod = getattr(l.self_attn, t)
            w = mod.base_layer.weight.double() + mod.scaling * (mod.B.double() @ mod.A.double())
            mg[f"model.layers.{li}.self_attn.{t}.weight"] = w.float()
    return base, mg


def test_from_config_builds_adapters_with_peft_names_and_fresh_model_equals_base():
    from stllm_amd import runtime
    from stllm_amd.models.blip2 import Blip2Base
    from stllm_amd.models import st_llm
    from stllm_amd.tokenizer import IdTokenizer
    from stllm_amd import synth
    old = (Blip2Base.vit_depth, Blip2Base.qformer_layers, Blip2Base.init_tokenizer)
    Blip2Base.vit_depth, Blip2Base.qformer_layers = 1, 2
    Blip2Base.init_tokenizer = classmethod(lambda cls, truncation_side="right": IdTokenizer(0, 1, 2, 32000))
    try:
        m = st_llm.STLLMForCausalLM.from_config(dict(CFG, llama_model=dict(num_hidden_layers=1), lora_r=16), device="cpu")
    finally:
        Blip2Base.vit_depth, Blip2Base.qformer_layers, Blip2Base.init_tokenizer = old
    sd = m.state_dict()
    for t in ("q_proj", "v_proj"):
        p = f"model.layers.0.self_attn.{t}."
        assert sd[p + "lora_A.default.weight"].shape == (16, 4096)
        assert sd[p + "lora_B.default.weight"].shape == (4096, 16)
        assert sd[p + "base_layer.weight"].shape == (4096, 4096)
        assert float(sd[p + "lora_B.default.weight"].abs().max()) == 0.0            # peft's init: B = 0 ...
        a = sd[p + "lora_A.default.weight"]
        assert 0 < float(a.abs().max()) <= 1 / 64 + 1e-7                            # ... A ~ U(-1/sqrt(4096), 1/sqrt(4096))
    assert "model.layers.0.self_attn.k_proj.weight" in sd and not any("k_proj.lora" in k for k in sd)
    assert m.model.layers[0].self_attn.q_proj.scaling == 2.0                       # lora_alpha 32 (default) / r 16
    # a fresh model (B = 0) == the same model without adapters, bit for bit
    synth.fill_module_(m, 0, "")
    for mod in m._lora_modules():
        mod.B.zero_()
    emb = T("input.inputs_embeds", (2, 11, 4096), 0.05)
    with CB.installed(), runtime.use_dtype("fp32"):
        fresh = m(samples=None, inputs_embeds=emb).logits.clone()
        m.merge_and_unload()
        plain = m(samples=None, inputs_embeds=emb).logits
    assert torch.equal(fresh, plain)


def test_forward_with_active_adapters_matches_oracle_on_merged_weights():
    from stllm_amd import runtime
    m = llm(2, 16, 0.05)
    emb = T("input.inputs_embeds", (2, 23, 4096), 0.05)
    mask = torch.ones(2, 23, dtype=torch.long)
    mask[1, 17:] = 0
    base, mg = oracle_sds(m)
    hb, hm = O.llama_forward(emb, mask, base), O.llama_forward(emb, mask, mg)
    lb, lm_ = O.lm_logits(hb, base), O.lm_logits(hm, mg)
    v = mask.bool()
    for a, b in ((hm, hb), (lm_, lb)):   # the guard: a build that ignores the adapters cannot pass
        assert float((a[v] - b[v]).abs().max()) >= 10 * TOL * float(a[v].abs().max())
    with CB.installed(), runtime.use_dtype("fp32"):
        out = m(samples=None, inputs_embeds=emb, attention_mask=mask, output_hidden_states=True)
    for got, want in ((out.hidden_states[-1], hm), (out.logits, lm_)):
        assert float((got[v] - want[v]).abs().max()) <= TOL * float(want[v].abs().max())


def test_decode_with_adapters_uses_the_adapted_cache():
    from stllm_amd import runtime
    m = llm(2, 8, 0.05)
    emb = T("input.inputs_embeds", (1, 13, 4096), 0.05)
    with CB.installed(), runtime.use_dtype("fp32"):
        full = m(samples=None, inputs_embeds=emb).logits
        o1 = m(samples=None, inputs_embeds=emb[:, :12], use_cache=True)
        o2 = m(samples=None, inputs_embeds=emb[:, 12:], past_key_values=o1.past_key_values)
        ids_a = m.generate(inputs_embeds=emb, max_new_tokens=4, num_beams=3, min_length=1)
        m.merge_adapter()
        merged = m(samples=None, inputs_embeds=emb).logits
        ids_m = m.generate(inputs_embeds=emb, max_new_tokens=4, num_beams=3, min_length=1)
        m.unmerge_adapter()
        base_only = llm(2)(samples=None, inputs_embeds=emb).logits
    scale = float(full.abs().max())
    assert float((merged - base_only).abs().max()) >= 10 * TOL * scale     # the adapters matter ...
    assert float((o2.logits[:, -1] - full[:, 12]).abs().max()) <= TOL * scale   # ... and the decode step sees them (cache rows and its own q / v)
    assert float((merged - full).abs().max()) <= TOL * scale
    assert torch.equal(ids_a, ids_m)


def test_merge_unmerge_and_unload():
    from stllm_amd import runtime
    m = llm(1, 64, 0.05, alpha=16)
    _, mg = oracle_sds(m)
    w0 = {k: v.clone() for k, v in m.state_dict().items()}
    with CB.installed(), runtime.use_dtype("fp32"):
        m.merge_adapter()
        for t in ("q_proj", "v_proj"):
            k = f"model.layers.0.self_attn.{t}"
            want, got = mg[k + ".weight"].double(), m.state_dict()[k + ".base_layer.weight"].double()
            assert float((want - w0[k + ".base_layer.weight"].double()).abs().max()) > 1e-3 * float(want.abs().max())
            assert float((got - want).abs().max()) <= 1e-6 * float(want.abs().max())
        m.unmerge_adapter()
        for k, v in w0.items():
            assert float((m.state_dict()[k].double() - v.double()).abs().max()) <= 1e-6 * max(float(v.abs().max()), 1e-30), k
        m.merge_and_unload()
    assert not any("lora_" in k or "base_layer" in k for k in m.state_dict())


def test_changed_adapter_weights_repack():
    from stllm_amd import runtime
    m = llm(1, 16, 0.05)
    emb = T("input.inputs_embeds", (1, 7, 4096), 0.05)
    with CB.installed(), runtime.use_dtype("fp32"):
        a = m(samples=None, inputs_embeds=emb).logits.clone()
        m.model.layers[0].self_attn.v_proj.B.mul_(-1.0)
        b = m(samples=None, inputs_embeds=emb).logits.clone()
    assert float((a - b).abs().max()) >= 10 * TOL * float(a.abs().max())


def test_checkpoint_layouts_round_trip(tmp_path):
    """peft's keys (prefix, base_layer, .default) through load_state_dict; HF base keys into a LoRA model; an adapter-only file on top"""
    from stllm_amd import runtime
    from stllm_amd.models import lora
    src = llm(1, 16, 0.05)
    emb = T("input.inputs_embeds", (1, 7, 4096), 0.05)
    with CB.installed(), runtime.use_dtype("fp32"):
        want = src(samples=None, inputs_embeds=emb).logits.clone()
    full = lora.peft_state_dict(src)
    assert all(k.startswith("base_model.model.") for k in full)
    assert "base_model.model.model.layers.0.self_attn.q_proj.base_layer.weight" in full
    assert "base_model.model.model.layers.0.self_attn.v_proj.lora_B.default.weight" in full
    torch.save(full, tmp_path / "full.pth")
    torch.save({"model": lora.peft_state_dict(src, adapter_only=True)}, tmp_path / "adapter.pth")
    hf_base = {k.replace(".base_layer.", "."): v for k, v in src.state_dict().items() if "lora_" not in k}
    assert "model.layers.0.self_attn.q_proj.weight" in hf_base

    def fresh():
        from stllm_amd.models.st_llm import STLLMForCausalLM, StllmConfig
        m = STLLMForCausalLM(StllmConfig(num_hidden_layers=1), device="cpu")
        for p in m.parameters():
            p.zero_()
        return m.add_lora(16)

    a = fresh()
    a.load_state_dict(torch.load(tmp_path / "full.pth"), strict=True)
    b = fresh()
    res = b.load_state_dict(hf_base, strict=False)                       # a plain HF directory's names into a LoRA model
    assert not res.unexpected_keys and all("lora_" in k for k in res.missing_keys)
    res = b.load_state_dict(torch.load(tmp_path / "adapter.pth")["model"], strict=False)
    assert not res.unexpected_keys and len(torch.load(tmp_path / "adapter.pth")["model"]) == 4
    with CB.installed(), runtime.use_dtype("fp32"):
        for m in (a, b):
            assert torch.equal(m(samples=None, inputs_embeds=emb).logits, want)
    with CB.installed():
        c = fresh().merge_and_unload()                                     # peft names into a model WITHOUT adapter modules: base_layer -> weight
    res = c.load_state_dict(full, strict=False)
    assert all("lora_" in k for k in res.unexpected_keys) and not res.missing_keys


def test_rejections():
    from stllm_amd import runtime
    from stllm_amd.models.st_llm import STLLMForCausalLM, StllmConfig
    for r in (12, 128, 0, 4):
        with pytest.raises(ValueError, match="lora_r"):
            STLLMForCausalLM(StllmConfig(num_hidden_layers=1), device="cpu").add_lora(r)
    m = llm(1, 16, 0.05)
    emb = T("input.inputs_embeds", (1, 40, 4096), 0.05)
    for mode in ("bf16x3", "mixed"):
        with CB.installed(), runtime.use_dtype(mode):
            with pytest.raises(NotImplementedError, match="merge"):
                m(samples=None, inputs_embeds=emb)
    with CB.installed(), runtime.use_dtype("fp32"):
        with pytest.raises(NotImplementedError, match="merge"):
            m.model.prefill_sp(emb, dict(index=0, size=1, ranks=[0], rank=0))
        m.merge_adapter()                                                   # merged: the unchanged base path, every mode
        m.model.prefill_sp(emb, dict(index=0, size=1, ranks=[0], rank=0))
    with runtime.use_dtype("bf16x3"):
        assert "lora_A" not in m.model.pack()[0]                           # (the split weights pack; the contract backend does not run them)


def test_abi_is_additive():
    from stllm_amd import hip
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "stllm_hip.h")).read()
    for name in ("stllm_lora_down", "stllm_lora_down_workspace_bytes", "stllm_llama_layers_lora", "stllm_llama_layers_lora_scratch_bytes"):
        assert name in hip.EXPORTS and name + "(" in header
    assert hip.lib().stllm_abi_version() == 7
    assert hip.lora_pad(8, "bf16") == 64 and hip.lora_pad(64, "bf16") == 128 and hip.lora_pad(8, "fp32") == 32 and hip.lora_pad(24, "fp32") == 64


def test_from_config_loads_peft_checkpoints(tmp_path):
    """from_config(ckpt=...): a full peft-keyed file (under {"model": ...}, with a vocabulary of its own) and an adapter-only file over a base directory"""
    import json
    from stllm_amd import runtime
    from stllm_amd.models import lora, st_llm
    from stllm_amd.models.blip2 import Blip2Base
    from stllm_amd.tokenizer import IdTokenizer
    src = llm(1, 16, 0.05)
    src.resize_token_embeddings(32003)                                     # a checkpoint whose vocabulary differs from the config's
    emb = T("input.inputs_embeds", (1, 7, 4096), 0.05)
    with CB.installed(), runtime.use_dtype("fp32"):
        want = src(samples=None, inputs_embeds=emb).logits.clone()
    torch.save({"model": lora.peft_state_dict(src)}, tmp_path / "full.pth")
    torch.save({"model": lora.peft_state_dict(src, adapter_only=True)}, tmp_path / "adapter.pth")
    base_dir = tmp_path / "vicuna"
    base_dir.mkdir()
    json.dump(dict(hidden_size=4096, intermediate_size=11008, num_hidden_layers=1, num_attention_heads=32, vocab_size=32003), open(base_dir / "config.json", "w"))
    hf = {k.replace(".base_layer.", "."): v for k, v in src.state_dict().items() if "lora_" not in k}
    torch.save(hf, base_dir / "pytorch_model-00001-of-00001.bin")
    old = (Blip2Base.vit_depth, Blip2Base.qformer_layers, Blip2Base.init_tokenizer)
    Blip2Base.vit_depth, Blip2Base.qformer_layers = 1, 2
    Blip2Base.init_tokenizer = classmethod(lambda cls, truncation_side="right": IdTokenizer(0, 1, 2, 32000))
    try:
        a = st_llm.STLLMForCausalLM.from_config(dict(CFG, llama_model=dict(num_hidden_layers=1), lora_r=16, ckpt=str(tmp_path / "full.pth")), device="cpu")
        b = st_llm.STLLMForCausalLM.from_config(dict(CFG, llama_model=str(base_dir), lora_r=16, ckpt=str(tmp_path / "adapter.pth")), device="cpu")
    finally:
        Blip2Base.vit_depth, Blip2Base.qformer_layers, Blip2Base.init_tokenizer = old
    assert a.config.vocab_size == 32003 and a.lm_head.weight.shape[0] == 32003
    with CB.installed(), runtime.use_dtype("fp32"):
        for m in (a, b):
            assert torch.equal(m(samples=None, inputs_embeds=emb).logits, want)

