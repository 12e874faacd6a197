"""TEST-ONLY: the contract backends up to tests/_cpu_backend_shared.py (which stacks the prefix, int8, ragged and shared-prefix ones) extended, by import, with stllm_gemv_q4 (hip.gemv_q4) as plain fp32 torch on the CPU, restating its contract
(include/stllm_hip.h): epilogue(sum_g scale[n, g] * (A[:, g] @ q[n, g]^T) + bias), the scale applied per 128-element K group to the finished group sum;
q comes from pack.dequant4_groups (only pack.py and the kernel know the nibble placement).  CALLS records every call."""
import contextlib

import torch
import torch.nn.functional as F

import _cpu_backend as base
import _cpu_backend_shared as shared_base

CALLS = []   # (epilogue, M, N, K, fused_norm) of every gemv_q4 call since the last clear()


def gemv_q4(a, qp, scale, *, dtype, epilogue=base.EPI_STORE, bias=None, resid=None, rope=None, rope_seq=0, rope_cols=0, out=None, out_f32=False,
            a_norm=None, M=None, a_rows=None, o_rows=None):
    from stllm_amd import pack
    td = base.torch_dtype(dtype)
    assert td in (torch.bfloat16, torch.float16) and qp.dtype == torch.uint8 and scale.dtype == torch.float32
    assert epilogue in (base.EPI_STORE, base.EPI_RESID, base.EPI_SWIGLU, base.EPI_ROPE)
    if a_norm is not None:
        xn, gamma, eps = a_norm
        assert a is None and xn.shape[0] <= 2
        a = base.rmsnorm(xn, gamma, eps, dtype=dtype)[0]
    assert a.dtype == td and a_rows is None
    M = a.shape[0] if M is None else M
    N, K = qp.shape[0], qp.shape[1] * 2
    assert M <= 16 and N % 64 == 0 and K % 128 == 0 and a.shape[-1] == K and tuple(scale.shape) == (N, K // 128)
    q, _ = pack.dequant4_groups(qp, scale)
    assert int(q.min()) >= -7 and int(q.max()) <= 7
    CALLS.append((epilogue, M, N, K, a_norm is not None))
    G = K // 128
    # sum_g scale[n, g] * (A_g @ q_g^T) as ONE fp32 product with the weight the format stands for, w = q * scale (one fp32 rounding per weight): the
    # arithmetic of the 16-bit contract backend over that w, so the model tests compare routing and layouts, not two fp32 summation orders — whose
    # 1e-7 differences flip a bf16 rounding of a hidden element now and then (measured: 3e-4 .. 1.7e-3 x logits per flip, int8 backend alike).  The
    # order of the kernels' sums is the business of the emulator / GPU tests, against fp64.
    w = (q.float().view(N, G, 128) * scale[:, :, None]).reshape(N, K)
    acc = a[:M].float() @ w.t()
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
    with shared_base.installed():
        saved = hip.gemv_q4
        hip.gemv_q4 = gemv_q4
        try:
            yield
        finally:
            hip.gemv_q4 = saved
