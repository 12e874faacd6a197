"""TEST-ONLY: tests/_cpu_backend.py (+ its LoRA extension) extended, by import, with the prefix-cache entry points of include/stllm_hip.h —
stllm_attention_offset (hip.attention(q_off=)) and stllm_llama_layers_extend as plain fp32 torch on the CPU, restating their contracts."""
import contextlib

import torch

import _cpu_backend as base
import _cpu_backend_lora as lora_base


def attention(q, k, v, *, B, H, Sq, Skv, D, scale, causal=False, kv_len=None, out=None, q_strides=None, k_strides=None,
              v_strides=None, q_off=0):
    """stllm_attention / stllm_attention_offset: query row i sits at position q_off + i; causal: key j visible iff j <= q_off + i"""
    if not q_off:
        return base.attention(q, k, v, B=B, H=H, Sq=Sq, Skv=Skv, D=D, scale=scale, causal=causal, kv_len=kv_len, out=out,
                              q_strides=q_strides, k_strides=k_strides, v_strides=v_strides)
    assert q_off > 0 and q_off + Sq <= Skv

    def heads(t, S, strides):
        bs, rs = strides if strides is not None else (S * t.stride(0), t.stride(0))
        return torch.as_strided(t, (B, S, H, D), (bs, rs, D, 1), t.storage_offset()).float().transpose(1, 2)
    qh, kh, vh = heads(q, Sq, q_strides), heads(k, Skv, k_strides), heads(v, Skv, v_strides)
    s = (qh @ kh.transpose(-1, -2)) * scale
    if causal:
        s = s.masked_fill(torch.arange(Skv)[None, :] > torch.arange(Sq)[:, None] + q_off, float("-inf"))
    if kv_len is not None:
        dead = torch.arange(Skv)[None, :] >= kv_len.long()[:, None]
        s = s.masked_fill(dead[:, None, None, :], float("-inf"))
    o = (s.softmax(-1) @ vh).transpose(1, 2).reshape(B * Sq, H * D).to(q.dtype)
    if out is not None:
        out.copy_(o)
        return out
    return o


def llama_layers_extend(x, layers, carr, *, B, S, pos0, n_heads, eps, rope, dtype, cache):
    """stllm_llama_layers_extend: the per-op body (what the C entry point issues)"""
    from stllm_amd.models.llama import LlamaModel
    lm = base._LM(x.shape[1], n_heads, eps)
    return LlamaModel.extend_layers_per_op(lm, x, layers, B, S, pos0, rope[0], rope[1], cache, dtype)


@contextlib.contextmanager
def installed():
    from stllm_amd import hip
    names = ["attention", "llama_layers_extend"]
    with lora_base.installed():
        saved = {n: getattr(hip, n) for n in names}
        try:
            for n in names:
                setattr(hip, n, globals()[n])
            yield
        finally:
            for n, f in saved.items():
                setattr(hip, n, f)
