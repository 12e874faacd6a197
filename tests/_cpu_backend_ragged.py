"""TEST-ONLY: tests/_cpu_backend_w8.py extended, by import, with the ragged-KV-cache entry points of include/stllm_hip.h — stllm_kv_append_rows
(hip.kv_append_rows) and stllm_attention_decode_ragged (hip.attention_decode_ragged, hip.attention(Sq=1, kv_len=...)) —
as plain torch on the CPU.  CALLS records the name of every compute entry point called while counting() is active."""
import contextlib

import torch

import _cpu_backend_w8 as w8_base

CALLS = []
COUNTED = ["gemm", "gemv_w8", "rmsnorm", "attention", "attention_decode_ragged", "kv_append_rows", "gather_rows", "lora_down"]


def kv_append_rows(src, cache, pos, *, with_q=False):
    """cache[b, pos[b], cols] = src[b, cols], cols = [k | v] (with_q: [q | k | v]); a position outside [0, max_len) is a free slot: nothing written"""
    B, max_len, D3 = cache.shape
    assert src.shape == (B, D3) and src.dtype == cache.dtype and pos.dtype == torch.int32 and pos.numel() == B
    c0 = 0 if with_q else D3 // 3
    for b, p in enumerate(pos.tolist()):
        if 0 <= p < max_len:
            cache[b, p, c0:] = src[b, c0:]
    return cache


def attention(q, k, v, *, B, H, Sq, Skv, D, scale, causal=False, kv_len=None, out=None, q_strides=None, k_strides=None, v_strides=None, q_off=0):
    """as the backend below; the one-token step over a ragged cache (Sq = 1 with kv_len) reads the LIVE keys of every row only, as the kernels do: the rows
    behind a row's length are uninitialised memory, and 0 * NaN in a dense masked softmax would leak it"""
    if Sq != 1 or kv_len is None:
        return w8_base.prefix_base.attention(q, k, v, B=B, H=H, Sq=Sq, Skv=Skv, D=D, scale=scale, causal=causal, kv_len=kv_len, out=out,
                                             q_strides=q_strides, k_strides=k_strides, v_strides=v_strides, q_off=q_off)
    ks = k_strides if k_strides is not None else (Skv * k.stride(0), k.stride(0))
    vs = v_strides if v_strides is not None else (Skv * v.stride(0), v.stride(0))
    n = kv_len.clamp(max=Skv).long()
    dead = torch.arange(Skv)[None, :] >= n[:, None]
    kc = torch.as_strided(k, (B, Skv, H * D), (ks[0], ks[1], 1), k.storage_offset()).clone()
    vc = torch.as_strided(v, (B, Skv, H * D), (vs[0], vs[1], 1), v.storage_offset()).clone()
    kc[dead] = 0
    vc[dead] = 0
    o = w8_base.prefix_base.attention(q, kc.view(B * Skv, H * D), vc.view(B * Skv, H * D), B=B, H=H, Sq=1, Skv=Skv, D=D, scale=scale, causal=False,
                                      kv_len=n.clamp(min=1), q_strides=q_strides)
    o[n <= 0] = 0
    if out is not None:
        out.copy_(o)
        return out
    return o


def attention_decode_ragged(q, k, v, kv_len, *, B, H, max_kv, D, scale, out=None, q_stride=None, k_strides=None, v_strides=None):
    """row b attends keys [0, min(kv_len[b], max_kv)); a row of length <= 0 gets zeros"""
    return attention(q, k, v, B=B, H=H, Sq=1, Skv=max_kv, D=D, scale=scale, kv_len=kv_len, out=out,
                     q_strides=(q.stride(0) if q_stride is None else q_stride,) * 2, k_strides=k_strides, v_strides=v_strides)


@contextlib.contextmanager
def installed():
    from stllm_amd import hip
    names = ["attention", "kv_append_rows", "attention_decode_ragged"]
    with w8_base.installed():
        saved = {n: getattr(hip, n) for n in names}
        try:
            for n in names:
                setattr(hip, n, globals()[n])
            yield
        finally:
            for n, f in saved.items():
                setattr(hip, n, f)


@contextlib.contextmanager
def counting():
    """inside installed(): append the name of every compute entry point that the host code calls to CALLS"""
    from stllm_amd import hip
    saved = {n: getattr(hip, n) for n in COUNTED}

    def wrap(name, f):
        def g(*a, **k):
            CALLS.append(name)
            return f(*a, **k)
        return g
    CALLS.clear()
    try:
        for n, f in saved.items():
            setattr(hip, n, wrap(n, f))
        yield CALLS
    finally:
        for n, f in saved.items():
            setattr(hip, n, f)
