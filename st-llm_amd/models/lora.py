"""LoRA adapters on the Llama q_proj / v_proj (the reference's ``lora_r > 0`` branch, st_llm.py:165-177:
``LoraConfig(r, lora_alpha, target_modules=["q_proj", "v_proj"], lora_dropout=0.05, bias="none")``).

peft 0.8.1 ``Linear`` semantics, eval:  y = W x + (lora_alpha / r) · B (A x),  A [r, in], B [out, r], no bias; A is drawn
Kaiming-uniform(a = √5), B starts at zero, so a fresh model equals the base model.  ``LoraLinear`` holds the parameters under
peft's names (``base_layer.weight``, ``lora_A.default.weight``, ``lora_B.default.weight``); the arithmetic is not here: the
decoder layer packs the adapters into the K-extended QKV weight (``extend_qkv``) and the kernels do the rest (csrc/lora.hip,
stllm_llama_layers_lora).  Merging adds s·B·A to the fp32 master weights on the device with the library's own fp32 GEMM.

peft itself is not a dependency and its source was not available when this was written: the key layout below follows peft's
documented state-dict format (``base_model.model.`` prefix, ``base_layer``, adapter name ``default``).
"""
import math

import torch
import torch.nn as nn

from .. import hip, pack
from .layers import _dev

TARGETS = ("q_proj", "v_proj")
ADAPTER = "default"
# ---- the ONE table of checkpoint key rewrites (peft <-> HF <-> this package) -----------------------------------------------------
PEFT_PREFIX = "base_model.model."                       # get_peft_model wraps the whole causal LM
BASE_SUFFIX = {f".self_attn.{t}.weight": f".self_attn.{t}.base_layer.weight" for t in TARGETS}   # HF name -> peft name of an adapted Linear's weight


def check_rank(r):
    if not isinstance(r, int) or r % 8 != 0 or not 8 <= r <= 64:
        raise ValueError(f"lora_r = {r!r}: the adapter kernels take ranks that are multiples of 8 in [8, 64]")
    return r


class _Weight(nn.Module):
    """nn.Linear(bias=False)-named holder of one adapter matrix"""

    def __init__(self, out_features, in_features, device):
        super().__init__()
        # requires_grad stays False like every parameter of the package (the backward is explicit: stllm_amd.training); what the reference leaves
        # trainable — `'lora' in name`, st_llm.py:182-185 — is training.trainable_parameters' rule
        self.weight = nn.Parameter(torch.empty(out_features, in_features, device=_dev(device)), requires_grad=False)


class LoraLinear(nn.Module):
    """peft.tuners.lora.Linear's parameter layout around one of the package's Linear holders (one adapter, "default")."""

    def __init__(self, base, r, lora_alpha, seed=0):
        super().__init__()
        self.base_layer = base
        self.in_features, self.out_features = base.in_features, base.out_features
        self.r, self.lora_alpha, self.scaling = check_rank(r), lora_alpha, lora_alpha / r
        dev = base.weight.device
        self.lora_A = nn.ModuleDict({ADAPTER: _Weight(r, self.in_features, dev)})
        self.lora_B = nn.ModuleDict({ADAPTER: _Weight(self.out_features, r, dev)})
        self.merged = False
        # peft's reset_lora_parameters: kaiming_uniform_(A, a=sqrt(5)) = U(-1/sqrt(in), 1/sqrt(in)); B = 0
        g = torch.Generator().manual_seed(seed)
        bound = 1.0 / math.sqrt(self.in_features)
        with torch.no_grad():
            self.A.copy_(((torch.rand((r, self.in_features), generator=g) * 2 - 1) * bound).to(dev))
            self.B.zero_()

    @property
    def weight(self):          # the code that reads `q_proj.weight` (packers, training) sees the base weight
        return self.base_layer.weight

    @property
    def A(self):
        return self.lora_A[ADAPTER].weight

    @property
    def B(self):
        return self.lora_B[ADAPTER].weight

    @property
    def active(self):
        return not self.merged

    def merge(self, sign=1.0):
        """W <- W + sign · s · B · A on the fp32 master, on the device: one exact-fp32 GEMM of the library with the residual epilogue
        (K = r zero-padded to the fp32 GEMM's granularity)."""
        r, kp = self.r, (self.r + 31) // 32 * 32
        W = self.base_layer.weight
        a = torch.zeros((self.out_features, kp), device=W.device, dtype=torch.float32)
        a[:, :r] = self.B.detach().float() * (sign * self.scaling)
        w = torch.zeros((self.in_features, kp), device=W.device, dtype=torch.float32)
        w[:, :r] = self.A.detach().float().t()
        hip.gemm(a, w, dtype=torch.float32, epilogue=hip.EPI_RESID, resid=W.data)


def adapters_of(layer):
    """(q, v) LoraLinear of a decoder layer with ACTIVE adapters, else None"""
    q, v = layer.self_attn.q_proj, layer.self_attn.v_proj
    if isinstance(q, LoraLinear) and isinstance(v, LoraLinear) and q.active and v.active:
        return q, v
    return None


def extend_qkv(wqkv, q, v, dt, n_heads):
    """packed wqkv [3 D, D] -> (extended weight [3 D, D + P], A [2 r, D], r, P): P extra K columns  [s B_q | 0] on the q rows (in the RoPE head
    permutation of pack.llama_qkv), zeros on the k rows, [0 | s B_v | 0] on the v rows — so that [h | h A^T] · W'^T = h W^T + s B (A h) lands in one
    fp32 accumulator before the RoPE epilogue.  s·B is rounded to the compute dtype ONCE, here."""
    if q.r != v.r:
        raise NotImplementedError("q_proj and v_proj adapters of different rank")
    r, D = q.r, wqkv.shape[1]
    P = hip.lora_pad(r, dt)
    ext = torch.zeros((3 * D, P), device=wqkv.device, dtype=dt)
    perm = pack.rope_head_perm(n_heads, D // n_heads, wqkv.device)
    ext[:D, :r] = (q.B.detach().float() * q.scaling).to(dt)[perm]
    ext[2 * D:, r:2 * r] = (v.B.detach().float() * v.scaling).to(dt)
    A = torch.cat((q.A.detach(), v.A.detach()), dim=0).to(dt).contiguous()
    return torch.cat((wqkv, ext), dim=1).contiguous(), A, r, P


def refresh_qkv(pk, q, v, dt, n_heads):
    """extend_qkv's adapter parts written into an existing pack in place: the P extra columns of pk["wqkv"] and pk["lora_A"]"""
    r, D = q.r, pk["wqkv"].shape[1] - pk["lora_P"]
    perm = pack.rope_head_perm(n_heads, D // n_heads, pk["wqkv"].device)
    pk["wqkv"][:D, D:D + r] = (q.B.detach().float() * q.scaling).to(dt)[perm]
    pk["wqkv"][2 * D:, D + r:D + 2 * r] = (v.B.detach().float() * v.scaling).to(dt)
    pk["lora_A"][:r] = q.A.detach().to(dt)
    pk["lora_A"][r:] = v.A.detach().to(dt)


def any_nonzero_b(llama_model):
    """True when some active adapter has a non-zero B — ONE reduced flag, one device read"""
    flags = [m.B.detach().any() for l in llama_model.layers for m in (adapters_of(l) or ())]
    return bool(torch.stack(flags).any()) if flags else False


def add_adapters(llama_model, r, lora_alpha=32):
    """get_peft_model(..., target_modules=["q_proj", "v_proj"]) for the decoder layers of a LlamaModel"""
    check_rank(r)
    for i, layer in enumerate(llama_model.layers):
        for j, t in enumerate(TARGETS):
            base = getattr(layer.self_attn, t)
            if isinstance(base, LoraLinear):
                raise RuntimeError("the model already has adapters")
            setattr(layer.self_attn, t, LoraLinear(base, r, lora_alpha, seed=1000 * i + j))
    llama_model.repack()


def unload_adapters(llama_model):
    for layer in llama_model.layers:
        for t in TARGETS:
            m = getattr(layer.self_attn, t)
            if isinstance(m, LoraLinear):
                setattr(layer.self_attn, t, m.base_layer)
    llama_model.repack()


def has_adapters(llama_model):
    return any(isinstance(getattr(l.self_attn, t), LoraLinear) for l in llama_model.layers for t in TARGETS)


def remap_keys(sd, adapted):
    """state dict in peft's, HF's or this package's layout -> the names of a model with (adapted=True) or without LoraLinear modules"""
    out = {}
    for k, v in sd.items():
        if k.startswith(PEFT_PREFIX):
            k = k[len(PEFT_PREFIX):]
        for hf, pf in BASE_SUFFIX.items():
            if adapted and k.endswith(hf):
                k = k[: -len(hf)] + pf
            elif not adapted and k.endswith(pf):
                k = k[: -len(pf)] + hf
        out[k] = v
    return out


def peft_state_dict(model, adapter_only=False):
    """the model's state dict under peft's names (what the reference's trainer saves); adapter_only: the `lora_` tensors alone (train_hf.py:125-147)"""
    return {PEFT_PREFIX + k: v for k, v in model.state_dict().items() if not adapter_only or "lora_" in k}
