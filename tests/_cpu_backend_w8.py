"""TEST-ONLY: tests/_cpu_backend_prefix.py extended, by import, with stllm_gemv_w8 (hip.gemv_w8) as plain fp32 torch on the CPU, restating its
contract (include/stllm_hip.h): epilogue(scale[n] * (A @ Wq^T) + bias), the scale applied to the finished sum.  CALLS records every call."""
import contextlib

import torch
import torch.nn.functional as F

import _cpu_backend as base
import _cpu_backend_prefix as prefix_base

CALLS = []   # (epilogue, M, N, K, fused_norm) of every gemv_w8 call since the last clear()


def gemv_w8(a, wq, scale, *, dtype, epilogue=base.EPI_STORE, bias=None, resid=None, rope=None, rope_seq=0, rope_cols=0, out=None, out_f32=False,
            a_norm=None, M=None, a_rows=None, o_rows=None):
    td = base.torch_dtype(dtype)
    assert td in (torch.bfloat16, torch.float16) and wq.dtype == torch.int8 and scale.dtype == torch.float32
    assert int(wq.abs().max()) <= 127 and epilogue in (base.EPI_STORE, base.EPI_RESID, base.EPI_SWIGLU, base.EPI_ROPE)
    if a_norm is not None:
        xn, gamma, eps = a_norm
        assert a is None and xn.shape[0] <= 2
        a = base.rmsnorm(xn, gamma, eps, dtype=dtype)[0]
    assert a.dtype == td and a_rows is None
    M = a.shape[0] if M is None else M
    N, K = wq.shape
    assert M <= 16 and N % 64 == 0 and K % 16 == 0 and a.shape[-1] == K
    CALLS.append((epilogue, M, N, K, a_norm is not None))
    acc = (a[:M].float() @ wq.float().t()) * scale[None, :]
    if bias is not None:
        acc = acc + bias
    if epilogue == base.EPI_RESID:
        dst = resid if out is None else out
        dst[base._rows(dst, M, o_rows)] = resid[:M].float() + acc
        return dst
    if epilogue == base.EPI_SWIGLU:
        g = acc.view(M, N // 64, 2, 32)
        val = (F.silu(g[:, :, 0]) * g[:, :, 1]).reshape(M, N // 2)
    elif epilogue == base.EPI_ROPE:
        cos, sin = rope
        x = acc.view(M, N // 64, 2, 32)
        grp = torch.arange(N // 64)
        pos = torch.arange(M) % rope_seq
        fi = (grp % 2)[:, None] * 32 + torch.arange(32)[None, :]
        c, s = cos[pos][:, fi], sin[pos][:, fi]
        live = (grp * 64 < rope_cols)[None, :, None]
        x1, x2 = x[:, :, 0], x[:, :, 1]
        val = torch.stack((torch.where(live, x1 * c - x2 * s, x1), torch.where(live, x2 * c + x1 * s, x2)), dim=2).reshape(M, N)
    else:
        val = acc
    odt = torch.float32 if (out_f32 and epilogue == base.EPI_STORE) else td
    if out is None:
        return val.to(odt)
    out[base._rows(out, M, o_rows)] = val.to(out.dtype)
    return out


@contextlib.contextmanager
def installed():
    from stllm_amd import hip
    with prefix_base.installed():
        saved = hip.gemv_w8
        hip.gemv_w8 = gemv_w8
        try:
            yield
        finally:
            hip.gemv_w8 = saved
