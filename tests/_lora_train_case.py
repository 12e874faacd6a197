"""Shared by tests/test_lora_train_cpu.py and tests/test_lora_gpu.py: one training case with LoRA adapters and its autograd reference.

The reference is autograd through the pinned oracle (oracle/stllm_oracle.py) with q_proj / v_proj = W + s·B·(A·diag(m)) as a differentiable
expression of the leaves A and B.  m is the injected lora_dropout mask; the oracle can only express masks that are constant over the rows
(a per-feature mask folds into A), so that is the shape of mask the parity check injects (None = no dropout)."""
import torch

import shapes
import stllm_oracle as O
from _util import T, sd_from

R, ALPHA, LAYERS = 16, 32, 2
FROZEN = ("model.stllm_model.visual_encoder", "model.stllm_model.ln_vision", "model.stllm_model.Qformer", "model.stllm_model.query_tokens")


def build_model(device="cpu"):
    from test_host_orchestration_cpu import CFGS, make_inputs
    cfg = CFGS["mean_pooling"]
    if device == "cpu":
        from test_host_orchestration_cpu import build
        model = build(cfg, vit_depth=1, qf_layers=2, llm_layers=LAYERS)
    else:
        from test_model_gpu import build_stllm
        model = build_stllm(cfg, vit_depth=1, qf_layers=2, llm_layers=LAYERS)
    model.add_lora(R, ALPHA)
    with torch.no_grad():
        for i, mod in enumerate(model._lora_modules()):
            mod.B.copy_(T(f"lora.B{i}", tuple(mod.B.shape), 0.05).to(mod.B.device))      # non-zero B: the adapters matter
    samples, osamples = make_inputs(2, 4, False)
    if device != "cpu":
        samples["image"] = samples["image"].to(device)
    return cfg, model, samples, osamples


def feature_mask(n_layers, n_rows, keep=0.95, seed=11):
    """lora_dropout factors [n_layers, 2, n_rows, 4096]: 0 or 1 / keep per FEATURE, the same for every row (see the module docstring)"""
    g = torch.Generator().manual_seed(seed)
    m = (torch.rand((n_layers, 2, 1, 4096), generator=g) < keep).float() / keep
    return m.expand(n_layers, 2, n_rows, 4096).contiguous()


def oracle_grads(cfg, model, osamples, mask=None):
    """(loss, {product parameter name: gradient}) for the trainable set of a LoRA model: the adapters + the non-frozen stllm_model parameters"""
    sd = sd_from({**shapes.stllm_model_shapes(1, 2, False, "mean", False, qf_vocab=32000), **shapes.llama_shapes(LAYERS)})
    leaves = {}
    for n in sd:
        if n.startswith("model.stllm_model.") and not n.startswith(FROZEN):
            leaves[n] = sd[n].requires_grad_(True)
    mods = model._lora_modules()
    with torch.enable_grad():
        for li in range(LAYERS):
            for j, t in enumerate(("q_proj", "v_proj")):
                mod = mods[2 * li + j]
                p = f"model.layers.{li}.self_attn.{t}."
                A = leaves[p + "lora_A.default.weight"] = mod.A.detach().cpu().clone().requires_grad_(True)
                Bm = leaves[p + "lora_B.default.weight"] = mod.B.detach().cpu().clone().requires_grad_(True)
                Am = A if mask is None else A * mask[li, j, 0][None, :]
                sd[p + "weight"] = sd[p + "weight"] + mod.scaling * (Bm @ Am)
        out = O.stllm_forward(osamples, sd, dict(cfg, pad_id=0, bos_id=1))
        out["loss"].backward()
    return out["loss"].item(), {n: v.grad for n, v in leaves.items() if v.grad is not None}
