"""TEST-ONLY: tests/_cpu_backend_ragged.py extended, by import, with the shared-prefix entry point of include/stllm_hip.h — stllm_attention_shared
(hip.attention_shared) — as plain torch on the CPU: fp64 softmax over the concatenated LIVE keys of every query row (the rows behind P and behind a
row's suffix length are uninitialised memory and are never read)."""
import contextlib

import torch

import _cpu_backend_ragged as ragged_base

CALLS = ragged_base.CALLS
COUNTED = ragged_base.COUNTED + ["attention_shared"]


def attention_shared(q, kp, vp, ks, vs, *, B, G, H, Sq, P, D, scale, max_sfx, sfx_len=None, sfx_q_off=0, causal=False, out=None,
                     q_strides=None, kp_strides=None, ks_strides=None):
    assert B % G == 0 and P > 0 and max_sfx > 0
    R = B // G
    qs = q_strides if q_strides is not None else (Sq * q.stride(0), q.stride(0))
    kps = kp_strides if kp_strides is not None else (P * kp.stride(0), kp.stride(0))
    kss = ks_strides if ks_strides is not None else (max_sfx * ks.stride(0), ks.stride(0))
    lens = [max_sfx] * B if sfx_len is None else [min(int(n), max_sfx) for n in sfx_len.tolist()]

    def rows(t, b, n, st):   # the first n rows of batch entry b: [n, H, D]
        return torch.as_strided(t, (n, H, D), (st[1], D, 1), t.storage_offset() + b * st[0]).double()
    o = torch.zeros((B * Sq, H * D), dtype=torch.float64)
    for b in range(B):
        g = b // R
        kpre, vpre = rows(kp, g, P, kps), rows(vp, g, P, kps)
        qb = rows(q, b, Sq, qs)
        for i in range(Sq):
            n = min(lens[b], sfx_q_off + i + 1) if causal else lens[b]
            k = torch.cat([kpre, rows(ks, b, n, kss)]).transpose(0, 1)      # [H, P + n, D]
            v = torch.cat([vpre, rows(vs, b, n, kss)]).transpose(0, 1)
            s = (qb[i].unsqueeze(1) @ k.transpose(-1, -2)) * scale
            o[b * Sq + i] = (s.softmax(-1) @ v).reshape(H * D)
    o = o.to(q.dtype)
    if out is not None:
        out.copy_(o)
        return out
    return o


@contextlib.contextmanager
def installed():
    from stllm_amd import hip
    with ragged_base.installed():
        saved = hip.attention_shared
        try:
            hip.attention_shared = attention_shared
            yield
        finally:
            hip.attention_shared = saved


@contextlib.contextmanager
def counting():
    """inside installed(): the name of every compute entry point the host code calls, attention_shared included"""
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
