"""TEST-ONLY: tests/_cpu_backend.py extended (by import, not by edit) with the LoRA entry points of include/stllm_hip.h —
stllm_lora_down and stllm_llama_layers_lora as plain fp32 torch on the CPU, restating their contracts."""
import contextlib

import torch

import _cpu_backend as base


def rmsnorm(x, gamma, eps, *, dtype, out_t=None, out_f32=None, want_t=True, want_f32=False):
    """stllm_rmsnorm writing into a caller's (strided) output rows — the K-extended QKV operand is one"""
    y_t, y_f = base.rmsnorm(x, gamma, eps, dtype=dtype, out_t=None, out_f32=out_f32, want_t=want_t or out_t is not None, want_f32=want_f32)
    if out_t is not None:
        out_t.copy_(y_t)
        y_t = out_t
    return y_t, y_f


def lora_down(x, A, *, dtype, out, M=None):
    """stllm_lora_down: out[:, :n] = x A^T (fp32 accumulation, rounded to the compute dtype), out[:, n:] = 0"""
    M = x.shape[0] if M is None else M
    n = A.shape[0]
    assert n <= out.shape[1] <= 128 and out.shape[1] % 32 == 0 and x.shape[1] == A.shape[1]
    out[:M, :n] = (x[:M].float() @ A.float().t()).to(out.dtype)
    out[:M, n:] = 0
    return out


def llama_lora_array(layers):
    return None


def llama_layers(x, layers, carr, *, B, S, n_heads, eps, rope, dtype, kv_len=None, cache=None, lora=None):
    """stllm_llama_layers / stllm_llama_layers_lora: the per-op body (the adapters travel inside the packed layer dicts)"""
    from stllm_amd.models.llama import LlamaModel
    lm = base._LM(x.shape[1], n_heads, eps)      # the stand-in the per-op body runs on, plus the adapted layers' operand builder
    lm.qkv_operand = lambda x_, pk, dt: LlamaModel.qkv_operand(lm, x_, pk, dt)
    return LlamaModel.prefill_layers_per_op(lm, x, layers, B, S, rope[0], rope[1], kv_len, cache, dtype)


@contextlib.contextmanager
def installed():
    from stllm_amd import hip
    names = ["rmsnorm", "lora_down", "llama_lora_array", "llama_layers"]
    with base.installed():
        saved = {n: getattr(hip, n) for n in names}
        try:
            for n in names:
                setattr(hip, n, globals()[n])
            yield
        finally:
            for n, f in saved.items():
                setattr(hip, n, f)
