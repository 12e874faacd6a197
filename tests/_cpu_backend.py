"""TEST-ONLY stand-in for ``stllm_amd.hip``: the whole compute call surface of include/stllm_hip.h as plain torch on the CPU,
every contract stated once.  It lets the product's *host code* (module graph, weight packers, index tables, KV caches, generate(),
the training step, ``bench.py --dry-cpu``) run without a GPU.  It is NOT a fallback: nothing in ``st-llm_amd/`` imports it.

Entry points, by the section of include/stllm_hip.h they restate:
  GEMM family      gemm (stllm_gemm, a_norm_*, the packed weight layouts), gemv_w8 (stllm_gemv_w8), gemv_q4 (stllm_gemv_q4),
                   lora_down (stllm_lora_down); one epilogue (_epilogue) and one fused-RMSNorm operand (_norm_operand) behind all of them
  norms            layernorm, rmsnorm (stllm_rmsnorm, into a caller's strided rows with out_t)
  attention        attention (stllm_attention, stllm_attention_offset with q_off; Sq = 1 with kv_len: the live keys only),
                   attention_decode_ragged, attention_shared, kv_append_rows
  rows / losses    gather_rows, mean_t, vit_cls_rows, cosine_rows, cross_entropy_rows, cast_rows, preprocess_frames
  backward / opt   transpose .. sumsq ("backward / optimizer")
  stacks           vit_blocks, llama_layers (stllm_llama_layers, stllm_llama_layers_lora), llama_layers_extend, qformer_layers: these
                   run the product's per-op bodies, which call back through ``hip``; every other function calls its helpers directly.
installed() patches all of them; counting() records the COUNTED names into CALLS; CALLS_W8 / CALLS_Q4 record the quantised GEMVs."""
import contextlib
import math

import torch
import torch.nn.functional as F

BF16, F16, F32 = 0, 1, 2
EPI_STORE, EPI_RESID, EPI_SWIGLU, EPI_ROPE, EPI_PATCH = 0, 1, 2, 3, 4
ACT_NONE, ACT_GELU, ACT_RELU = 0, 1, 2


def torch_dtype(d):
    return {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}.get(d, d) if isinstance(d, str) else d


def _rows(t, n, rows):
    """row indices of the logical rows 0..n-1 inside the 2-D buffer `t` under (rows_per_batch, batch_stride)"""
    if rows is None:
        return torch.arange(n)
    rpb, bs = rows
    m = torch.arange(n)
    return (m // rpb) * (bs // t.stride(-2)) + (m % rpb)


def _pairs(x, M, N):
    """[M, N] as [M, N/64, 2, 32]: every 64-column group holds gate | up (SwiGLU) or the rotary halves x1 | x2 of half a head"""
    return x.view(M, N // 64, 2, 32)


def _rope_tables(cos, sin, M, N, rope_seq, rope_cols):
    """(c, s, live) for the _pairs view: row m sits at position m % rope_seq; groups at columns >= rope_cols pass through"""
    grp = torch.arange(N // 64)
    pos = torch.arange(M) % rope_seq
    fi = (grp % 2)[:, None] * 32 + torch.arange(32)[None, :]             # [groups, 32]
    return cos[pos][:, fi], sin[pos][:, fi], (grp * 64 < rope_cols)[None, :, None]   # [M, groups, 32] x 2


def _norm_operand(a, a_norm, dtype, max_rows):
    """the fused RMSNorm operand of the decode regime (stllm_hip.h: a_norm_*): a = RMSNorm(xn) rounded to the compute dtype, for at most
    max_rows rows (8 for the GEMM, 2 for the GEMVs)"""
    if a_norm is None:
        return a
    xn, gamma, eps = a_norm
    assert a is None and xn.shape[0] <= max_rows and torch_dtype(dtype) != torch.float32
    return rmsnorm(xn, gamma, eps, dtype=dtype)[0]


def _epilogue(acc, M, N, *, epilogue, td, act=ACT_NONE, resid=None, rope=None, rope_seq=0, rope_cols=0, out=None, out_f32=False, o_rows=None):
    """what follows the fp32 accumulator (bias added) of gemm / gemv_w8 / gemv_q4: RESID | SWIGLU | ROPE | act + store"""
    if epilogue == EPI_RESID:
        res = resid[:M].float() + acc
        dst = resid if out is None else out
        dst[_rows(dst, M, o_rows)] = res
        return dst
    if epilogue == EPI_SWIGLU:
        g = _pairs(acc, M, N)
        val = (F.silu(g[:, :, 0]) * g[:, :, 1]).reshape(M, N // 2)
    elif epilogue == EPI_ROPE:
        x = _pairs(acc, M, N)
        c, s, live = _rope_tables(*rope, M, N, rope_seq, rope_cols)
        x1, x2 = x[:, :, 0], x[:, :, 1]
        val = torch.stack((torch.where(live, x1 * c - x2 * s, x1), torch.where(live, x2 * c + x1 * s, x2)), dim=2).reshape(M, N)
    else:
        val = acc
        if act == ACT_GELU:
            val = 0.5 * val * (1.0 + torch.erf(val / math.sqrt(2.0)))
        elif act == ACT_RELU:
            val = torch.relu(val)
    odt = torch.float32 if (out_f32 and epilogue == EPI_STORE) else td
    if out is None:
        return val.to(odt)
    out[_rows(out, M, o_rows)] = val.to(out.dtype)
    return out


def gemm(a, w, *, dtype, epilogue=EPI_STORE, bias=None, out=None, out_f32=False, act=ACT_NONE, resid=None,
         rope=None, rope_seq=0, rope_cols=0, frames=None, pos_embed=None, n_frames=0, M=None, a_rows=None, o_rows=None, a_norm=None):
    td = torch_dtype(dtype)
    a = _norm_operand(a, a_norm, dtype, 8)
    wf = w.float()
    N = w.shape[0]
    if epilogue == EPI_PATCH:
        n = n_frames
        cols = frames.float().reshape(n, 3, 16, 14, 16, 14).permute(0, 2, 4, 1, 3, 5).reshape(n * 256, 588)
        acc = cols.to(td).float() @ wf[:, :588].t()
        acc = acc + (bias if bias is not None else 0)
        o = out.view(n, 257, -1)
        o[:, 1:] = acc.view(n, 256, N) + pos_embed[1:].view(1, 256, N)
        return out
    if M is None:
        M = a.shape[0]
    if a_rows is None:
        A = a[:M].float()
    else:   # (rows_per_batch, batch_stride in elements): the stride need not be a whole number of rows (the no-Q-Former projector reads 64 rows of
        # 5632 behind the CLS row of every 257 x 1408 frame block) -> a strided view of the storage, as the kernel's byte addressing sees it
        rpb, bs = a_rows
        nb = (M + rpb - 1) // rpb
        A = torch.as_strided(a, (nb, rpb, a.shape[-1]), (bs, a.stride(-2), 1), a.storage_offset()).reshape(nb * rpb, a.shape[-1])[:M].float()
    acc = A @ wf.t()
    if bias is not None:
        acc = acc + bias
    return _epilogue(acc, M, N, epilogue=epilogue, td=td, act=act, resid=resid, rope=rope, rope_seq=rope_seq, rope_cols=rope_cols,
                     out=out, out_f32=out_f32, o_rows=o_rows)


CALLS_W8, CALLS_Q4 = [], []   # (epilogue, M, N, K, fused_norm) of every gemv_w8 / gemv_q4 call since the last clear()


def gemv_w8(a, wq, scale, *, dtype, epilogue=EPI_STORE, bias=None, resid=None, rope=None, rope_seq=0, rope_cols=0, out=None, out_f32=False,
            a_norm=None, M=None, a_rows=None, o_rows=None):
    """stllm_gemv_w8: epilogue(scale[n] * (A @ Wq^T) + bias), the scale applied to the finished sum"""
    td = torch_dtype(dtype)
    assert td in (torch.bfloat16, torch.float16) and wq.dtype == torch.int8 and scale.dtype == torch.float32
    assert int(wq.abs().max()) <= 127 and epilogue in (EPI_STORE, EPI_RESID, EPI_SWIGLU, EPI_ROPE)
    a = _norm_operand(a, a_norm, dtype, 2)
    assert a.dtype == td and a_rows is None
    M = a.shape[0] if M is None else M
    N, K = wq.shape
    assert M <= 16 and N % 64 == 0 and K % 16 == 0 and a.shape[-1] == K
    CALLS_W8.append((epilogue, M, N, K, a_norm is not None))
    acc = (a[:M].float() @ wq.float().t()) * scale[None, :]
    if bias is not None:
        acc = acc + bias
    return _epilogue(acc, M, N, epilogue=epilogue, td=td, resid=resid, rope=rope, rope_seq=rope_seq, rope_cols=rope_cols,
                     out=out, out_f32=out_f32, o_rows=o_rows)


def gemv_q4(a, qp, scale, *, dtype, epilogue=EPI_STORE, bias=None, resid=None, rope=None, rope_seq=0, rope_cols=0, out=None, out_f32=False,
            a_norm=None, M=None, a_rows=None, o_rows=None):
    """stllm_gemv_q4: epilogue(sum_g scale[n, g] * (A[:, g] @ q[n, g]^T) + bias), the scale applied per 128-element K group; q comes from
    pack.dequant4_groups (only pack.py and the kernel know the nibble placement)"""
    from stllm_amd import pack
    td = torch_dtype(dtype)
    assert td in (torch.bfloat16, torch.float16) and qp.dtype == torch.uint8 and scale.dtype == torch.float32
    assert epilogue in (EPI_STORE, EPI_RESID, EPI_SWIGLU, EPI_ROPE)
    a = _norm_operand(a, a_norm, dtype, 2)
    assert a.dtype == td and a_rows is None
    M = a.shape[0] if M is None else M
    N, K = qp.shape[0], qp.shape[1] * 2
    assert M <= 16 and N % 64 == 0 and K % 128 == 0 and a.shape[-1] == K and tuple(scale.shape) == (N, K // 128)
    q, _ = pack.dequant4_groups(qp, scale)
    assert int(q.min()) >= -7 and int(q.max()) <= 7
    CALLS_Q4.append((epilogue, M, N, K, a_norm is not None))
    # sum_g scale[n, g] * (A_g @ q_g^T) as ONE fp32 product with the weight the format stands for, w = q * scale (one fp32 rounding per weight): the
    # arithmetic of the 16-bit gemm above over that w, so the model tests compare routing and layouts, not two fp32 summation orders — whose
    # 1e-7 differences flip a bf16 rounding of a hidden element now and then (measured: 3e-4 .. 1.7e-3 x logits per flip, int8 backend alike).  The
    # order of the kernels' sums is the business of the emulator / GPU tests, against fp64.
    w = (q.float().view(N, K // 128, 128) * scale[:, :, None]).reshape(N, K)
    acc = a[:M].float() @ w.t()
    if bias is not None:
        acc = acc + bias
    return _epilogue(acc, M, N, epilogue=epilogue, td=td, resid=resid, rope=rope, rope_seq=rope_seq, rope_cols=rope_cols,
                     out=out, out_f32=out_f32, o_rows=o_rows)


def lora_down(x, A, *, dtype, out, M=None):
    """stllm_lora_down: out[:, :n] = x A^T (fp32 accumulation, rounded to the compute dtype), out[:, n:] = 0"""
    M = x.shape[0] if M is None else M
    n = A.shape[0]
    assert n <= out.shape[1] <= 128 and out.shape[1] % 32 == 0 and x.shape[1] == A.shape[1]
    out[:M, :n] = (x[:M].float() @ A.float().t()).to(out.dtype)
    out[:M, n:] = 0
    return out


def layernorm(x, gamma, beta, eps, *, dtype, out_t=None, out_f32=None, want_t=True, want_f32=False):
    y = F.layer_norm(x.float(), (x.shape[-1],), gamma.float(), beta.float(), eps)
    return (y.to(torch_dtype(dtype)) if want_t or out_t is not None else None), (y if want_f32 or out_f32 is not None else None)


def rmsnorm(x, gamma, eps, *, dtype, out_t=None, out_f32=None, want_t=True, want_f32=False):
    """stllm_rmsnorm; out_t: a caller's (strided) output rows — the K-extended QKV operand is one"""
    xf = x.float()
    y = gamma.float() * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps))
    y_t = y.to(torch_dtype(dtype)) if want_t or out_t is not None else None
    if out_t is not None:
        out_t.copy_(y_t)
        y_t = out_t
    return y_t, (y if want_f32 else None)


def _heads(t, B, S, H, D, strides):
    """[B, S, H, D] view: element (b, s, h, d) lives at t.flat[b * batch_stride + s * row_stride + h * D + d] (include/stllm_hip.h)"""
    bs, rs = strides if strides is not None else (S * t.stride(0), t.stride(0))
    return torch.as_strided(t, (B, S, H, D), (bs, rs, D, 1), t.storage_offset())


def _dead_keys(s, Skv, kv_len):
    """scores with the keys at [kv_len[b], Skv) of batch row b at -inf: read, weightless, must be finite"""
    if kv_len is None:
        return s
    dead = torch.arange(Skv)[None, :] >= kv_len.long()[:, None]
    return s.masked_fill(dead[:, None, None, :], float("-inf"))


def _causal_mask(Sq, Skv, q_off=0):
    """True where key j is hidden from query row i, which sits at position q_off + i: j > q_off + i"""
    return torch.arange(Skv)[None, :] > torch.arange(Sq)[:, None] + q_off


def _attention_dense(q, k, v, *, B, H, Sq, Skv, D, scale, causal, kv_len, q_strides, k_strides, v_strides, q_off):
    """the dense masked softmax: rows in [kv_len, Skv) are read, weightless, and must be finite (a NaN there reaches the output)"""
    assert q_off >= 0 and (not q_off or q_off + Sq <= Skv)
    qh, kh, vh = (_heads(t, B, S, H, D, st).float().transpose(1, 2) for t, S, st in ((q, Sq, q_strides), (k, Skv, k_strides), (v, Skv, v_strides)))
    s = (qh @ kh.transpose(-1, -2)) * scale
    if causal:
        s = s.masked_fill(_causal_mask(Sq, Skv, q_off), float("-inf"))
    return (_dead_keys(s, Skv, kv_len).softmax(-1) @ vh).transpose(1, 2).reshape(B * Sq, H * D).to(q.dtype)


def attention(q, k, v, *, B, H, Sq, Skv, D, scale, causal=False, kv_len=None, out=None, q_strides=None, k_strides=None,
              v_strides=None, q_off=0):
    """stllm_attention / stllm_attention_offset: query row i sits at position q_off + i; causal: key j visible iff j <= q_off + i.  The one-token
    step over a ragged cache (Sq = 1 with kv_len) reads the LIVE keys of every row only, as the kernels do: the rows behind a row's length are
    uninitialised memory, and 0 * NaN in a dense masked softmax would leak it.  Every other case is that dense masked softmax."""
    if Sq == 1 and kv_len is not None:   # dead rows zeroed in a copy; a row of length <= 0 gets zeros
        n = kv_len.clamp(max=Skv).long()
        dead = torch.arange(Skv)[None, :] >= n[:, None]
        kc, vc = (_heads(t, B, Skv, 1, H * D, st).squeeze(2).clone() for t, st in ((k, k_strides), (v, v_strides)))
        kc[dead] = 0
        vc[dead] = 0
        o = _attention_dense(q, kc.view(B * Skv, H * D), vc.view(B * Skv, H * D), B=B, H=H, Sq=1, Skv=Skv, D=D, scale=scale, causal=False,
                             kv_len=n.clamp(min=1), q_strides=q_strides, k_strides=None, v_strides=None, q_off=0)
        o[n <= 0] = 0
    else:
        o = _attention_dense(q, k, v, B=B, H=H, Sq=Sq, Skv=Skv, D=D, scale=scale, causal=causal, kv_len=kv_len, q_strides=q_strides,
                             k_strides=k_strides, v_strides=v_strides, q_off=q_off)
    if out is not None:
        out.copy_(o)
        return out
    return o


def attention_decode_ragged(q, k, v, kv_len, *, B, H, max_kv, D, scale, out=None, q_stride=None, k_strides=None, v_strides=None):
    """stllm_attention_decode_ragged: row b attends keys [0, min(kv_len[b], max_kv)); a row of length <= 0 gets zeros"""
    return attention(q, k, v, B=B, H=H, Sq=1, Skv=max_kv, D=D, scale=scale, kv_len=kv_len, out=out,
                     q_strides=(q.stride(0) if q_stride is None else q_stride,) * 2, k_strides=k_strides, v_strides=v_strides)


def kv_append_rows(src, cache, pos, *, with_q=False):
    """cache[b, pos[b], cols] = src[b, cols], cols = [k | v] (with_q: [q | k | v]); a position outside [0, max_len) is a free slot: nothing written"""
    B, max_len, D3 = cache.shape
    assert src.shape == (B, D3) and src.dtype == cache.dtype and pos.dtype == torch.int32 and pos.numel() == B
    c0 = 0 if with_q else D3 // 3
    for b, p in enumerate(pos.tolist()):
        if 0 <= p < max_len:
            cache[b, p, c0:] = src[b, c0:]
    return cache


def attention_shared(q, kp, vp, ks, vs, *, B, G, H, Sq, P, D, scale, max_sfx, sfx_len=None, sfx_q_off=0, causal=False, out=None,
                     q_strides=None, kp_strides=None, ks_strides=None):
    """stllm_attention_shared: fp64 softmax over the concatenated LIVE keys of every query row (the rows behind P and behind a row's suffix length
    are uninitialised memory and are never read)"""
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


def gather_rows(src_a, idx_a, *, src_b=None, add=None, idx_add=None, out=None, scale=1.0):
    idx = idx_a.long()
    res = torch.empty((idx.numel(), src_a.shape[-1]))
    pos = idx >= 0
    res[pos] = src_a[idx[pos]].float()
    if (~pos).any():
        res[~pos] = src_b[-idx[~pos] - 1].float()
    if add is not None:
        res = res + add[idx_add.long()].float()
    if scale != 1.0:
        res = res * scale
    if out is not None:
        out[: res.shape[0]] = res
        return out
    return res


def mean_t(x):
    assert x.shape[0] > 0 and x.shape[1] > 0, "stllm_mean_t: empty batch (the device binding indexes x[0, 0])"
    return x.float().mean(dim=1)


def vit_cls_rows(cls, pos, x, n_frames):
    x.view(n_frames, 257, -1)[:, 0] = cls + pos[0]


def cosine_rows(a, b, idx_a=None, idx_b=None, n_rows=None):
    aa = a if idx_a is None else a[idx_a.long()]
    bb = b if idx_b is None else b[idx_b.long()]
    n = n_rows if n_rows is not None else aa.shape[0]
    aa, bb = aa[:n].float(), bb[:n].float()
    return 2 - 2 * (F.normalize(aa, dim=-1) * F.normalize(bb, dim=-1)).sum(-1)


def cross_entropy_rows(logits, labels):
    return F.cross_entropy(logits.float(), labels.long(), ignore_index=-100, reduction="none")


def cast_rows(x, dtype, out=None):
    return x.to(torch_dtype(dtype))


def set_profiler(p):
    pass


def preprocess_frames(frames_u8, out=None):
    """stllm_preprocess_frames via the oracle (tests only): uint8 [T,H,W,3] -> f32 [T,3,224,224]"""
    import preprocess_oracle as P
    r = torch.from_numpy(P.video_transform(frames_u8.cpu().numpy())).view(-1, 3, 224, 224)
    if out is not None:
        out.copy_(r)
        return out
    return r


# ---- training entry points (contracts: include/stllm_hip.h "backward / optimizer") -----------------------------------
def transpose(x, *, pad=64, out=None):
    R, C = x.shape
    Rp = (R + pad - 1) // pad * pad
    o = torch.zeros((C, Rp), dtype=x.dtype)
    o[:, :R] = x.t()
    return o


def rmsnorm_bwd(x, gamma, eps, dy, dx, *, accumulate=True):
    xf, g = x.float(), gamma.float() * dy.float()
    r = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    xh = xf * r
    d = r * (g - xh * (g * xh).mean(-1, keepdim=True))
    if accumulate:
        dx += d
    else:
        dx.copy_(d)
    return (dy.float() * xh).sum(0)


def layernorm_bwd(x, gamma, eps, dy, dx=None, *, accumulate=False):
    xf = x.float()
    mu = xf.mean(-1, keepdim=True)
    r = torch.rsqrt(xf.var(-1, unbiased=False, keepdim=True) + eps)
    xh = (xf - mu) * r
    g = gamma.float() * dy.float()
    d = r * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    if dx is None:
        dx = d
    elif accumulate:
        dx += d
    else:
        dx.copy_(d)
    return dx, (dy.float() * xh).sum(0), dy.float().sum(0)


def swiglu(gu, out=None):
    M, N2 = gu.shape
    g = _pairs(gu.float(), M, N2)
    return (F.silu(g[:, :, 0]) * g[:, :, 1]).reshape(M, N2 // 2).to(gu.dtype)


def swiglu_bwd(gu, dg, out=None):
    M, N2 = gu.shape
    g = _pairs(gu.float(), M, N2)
    gate, up = g[:, :, 0], g[:, :, 1]
    d = dg.float().view(M, N2 // 64, 32)
    sg = torch.sigmoid(gate)
    dgate = d * up * sg * (1 + gate * (1 - sg))
    dup = d * gate * sg
    return torch.stack((dgate, dup), dim=2).reshape(M, N2).to(gu.dtype)


def rope_bwd(dqkv, cos, sin, *, rope_seq, rope_cols):
    M, N = dqkv.shape
    x = _pairs(dqkv.float(), M, N)
    c, s, live = _rope_tables(cos, sin, M, N, rope_seq, rope_cols)
    d1, d2 = x[:, :, 0], x[:, :, 1]
    x1 = torch.where(live, d1 * c + d2 * s, d1)
    x2 = torch.where(live, d2 * c - d1 * s, d2)
    dqkv.copy_(torch.stack((x1, x2), dim=2).reshape(M, N).to(dqkv.dtype))
    return dqkv


def attention_bwd(q, k, v, o, do, dq, dk, dv, *, B, H, S=None, D, scale, causal=True, kv_len=None, Sq=None, Skv=None, strides=None,
                  kv_strides=None, do_strides=None, d_strides=None, dkv_strides=None):
    Sq = S if Sq is None else Sq
    Skv = S if Skv is None else Skv

    def heads(t, n, given):
        return _heads(t, B, n, H, D, given)
    same = Sq == Skv
    ks = kv_strides if kv_strides is not None else (strides if same else None)
    dks = dkv_strides if dkv_strides is not None else (d_strides if same else None)
    qh = heads(q, Sq, strides).float().transpose(1, 2)
    kh, vh = (heads(t, Skv, ks).float().transpose(1, 2) for t in (k, v))
    doh = heads(do, Sq, do_strides).float().transpose(1, 2)
    s = (qh @ kh.transpose(-1, -2)) * scale
    if causal:
        s = s.masked_fill(_causal_mask(Sq, Skv), float("-inf"))
    p = _dead_keys(s, Skv, kv_len).softmax(-1)
    gv = p.transpose(-1, -2) @ doh
    dp = doh @ vh.transpose(-1, -2)
    ds = p * (dp - (dp * p).sum(-1, keepdim=True))
    gq = (ds @ kh) * scale
    gk = (ds.transpose(-1, -2) @ qh) * scale
    heads(dq, Sq, d_strides).copy_(gq.transpose(1, 2).to(dq.dtype))
    heads(dk, Skv, dks).copy_(gk.transpose(1, 2).to(dk.dtype))
    heads(dv, Skv, dks).copy_(gv.transpose(1, 2).to(dv.dtype))
    return dq, dk, dv


def cross_entropy_bwd(logits, labels, scale, *, dtype, vocab=None):
    n, Vp = logits.shape
    V = Vp if vocab is None else vocab
    lab = labels.long()
    pr = logits[:, :V].float().softmax(-1)
    ok = lab >= 0
    pr[ok, lab[ok]] -= 1.0
    pr[~ok] = 0.0
    out = torch.zeros((n, Vp), dtype=torch_dtype(dtype))
    out[:, :V] = (pr * scale).to(out.dtype)
    return out


def scatter_add_rows(src, idx, dst_a, dst_b=None, scale=1.0):
    i = idx.long()
    pos = i >= 0
    dst_a.index_add_(0, i[pos], src[: i.numel()][pos].float() * scale)
    if (~pos).any():
        dst_b.index_add_(0, -i[~pos] - 1, src[: i.numel()][~pos].float() * scale)


def cosine_rows_bwd(a, b, idx_a=None, idx_b=None, n_rows=None, scale=1.0):
    aa = a if idx_a is None else a[idx_a.long()]
    bb = b if idx_b is None else b[idx_b.long()]
    n = n_rows if n_rows is not None else aa.shape[0]
    aa, bb = aa[:n].float(), bb[:n].float()
    na = aa.norm(dim=-1, keepdim=True)
    ah, bh = aa / na, F.normalize(bb, dim=-1)
    return -2.0 * scale * (bh - (ah * bh).sum(-1, keepdim=True) * ah) / na


def colsum(x):
    return x.float().sum(0)


def relu_bwd(dy, y):
    return dy * (y > 0).to(dy.dtype)


def gelu(x):
    xf = x.float()
    return (0.5 * xf * (1.0 + torch.erf(xf / math.sqrt(2.0)))).to(x.dtype)


def gelu_bwd(x, dy):
    xf = x.float()
    cdf = 0.5 * (1.0 + torch.erf(xf / math.sqrt(2.0)))
    return (dy.float() * (cdf + xf * torch.exp(-0.5 * xf * xf) / math.sqrt(2.0 * math.pi))).to(x.dtype)


def scale_rows(x, scale, *, rows_per_group=0, idx=None):
    g = idx.long() if idx is not None else torch.arange(x.shape[0]) // rows_per_group
    x.copy_((x.float() * scale.float()[g][:, None]).to(x.dtype))
    return x


def bcast_add_t(dst, src, scale):
    dst += scale * src.unsqueeze(1)


def adamw(p, g, m, v, *, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, p16=None):
    gg = g * grad_scale
    p.mul_(1 - lr * weight_decay)
    m.mul_(beta1).add_(gg, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(gg, gg, value=1 - beta2)
    denom = (v.sqrt() / math.sqrt(1 - beta2 ** step)).add_(eps)
    p.addcdiv_(m, denom, value=-lr / (1 - beta1 ** step))
    if p16 is not None:
        p16.copy_(p)


def sumsq(x, out=None):
    if out is None:
        out = torch.zeros(1)
    out += x.float().pow(2).sum()
    return out


def vit_block_array(blocks):
    return None


def vit_blocks(x, blocks, carr, *, n_seq, seq_len, num_heads, dtype):
    """stllm_vit_blocks: the block loop, one contract call per op (what the C entry point issues)"""
    from stllm_amd.models.eva_vit import block_forward
    for bp in blocks:
        block_forward(x, bp, n_seq, seq_len, num_heads, dtype)
    return x


def llama_layer_array(layers, cache=None):
    return None


def llama_lora_array(layers):
    return None


class _LM:
    """the bits of LlamaModel that the per-op bodies read: config, and the adapted layers' operand builder"""
    def __init__(self, hidden, n_heads, eps):
        import types
        self.config = types.SimpleNamespace(hidden_size=hidden, num_attention_heads=n_heads, rms_norm_eps=eps)

    def qkv_operand(self, x, pk, dt):
        from stllm_amd.models.llama import LlamaModel
        return LlamaModel.qkv_operand(self, x, pk, dt)


def llama_layers(x, layers, carr, *, B, S, n_heads, eps, rope, dtype, kv_len=None, cache=None, lora=None):
    """stllm_llama_layers / stllm_llama_layers_lora: the per-op body (the adapters travel inside the packed layer dicts)"""
    from stllm_amd.models.llama import LlamaModel
    return LlamaModel.prefill_layers_per_op(_LM(x.shape[1], n_heads, eps), x, layers, B, S, rope[0], rope[1], kv_len, cache, dtype)


def llama_layers_extend(x, layers, carr, *, B, S, pos0, n_heads, eps, rope, dtype, cache):
    """stllm_llama_layers_extend: the per-op body (what the C entry point issues)"""
    from stllm_amd.models.llama import LlamaModel
    return LlamaModel.extend_layers_per_op(_LM(x.shape[1], n_heads, eps), x, layers, B, S, pos0, rope[0], rope[1], cache, dtype)


def qformer_layer_array(layers):
    return None


def qformer_layers(hq32, hq16, ht32, ht16, enc16, layers, carr, *, n_seq, n_query, n_text, n_heads, dtype, kv_len=None):
    """stllm_qformer_layers: the BertLayer loop, one contract call per op (what the C entry point issues)"""
    import types
    from stllm_amd.models.Qformer import BertModel
    shim = types.SimpleNamespace(config=types.SimpleNamespace(hidden_size=hq32.shape[1], num_attention_heads=n_heads))
    return BertModel.encode_layers_per_op(shim, layers, hq32, hq16, ht32, ht16, enc16, n_seq, n_query, n_text, kv_len, dtype)


NAMES = ["gemm", "gemv_w8", "gemv_q4", "lora_down", "layernorm", "rmsnorm", "attention", "attention_decode_ragged", "attention_shared",
         "kv_append_rows", "gather_rows", "mean_t", "vit_cls_rows", "cosine_rows", "cross_entropy_rows", "cast_rows", "preprocess_frames",
         "transpose", "rmsnorm_bwd", "layernorm_bwd", "swiglu", "swiglu_bwd", "rope_bwd", "attention_bwd", "cross_entropy_bwd",
         "scatter_add_rows", "cosine_rows_bwd", "colsum", "relu_bwd", "gelu", "gelu_bwd", "scale_rows", "bcast_add_t", "adamw", "sumsq",
         "vit_block_array", "vit_blocks", "llama_layer_array", "llama_lora_array", "llama_layers", "llama_layers_extend",
         "qformer_layer_array", "qformer_layers"]
CALLS = []   # the name of every COUNTED entry point called while counting() is active
COUNTED = ["gemm", "gemv_w8", "rmsnorm", "attention", "attention_decode_ragged", "kv_append_rows", "gather_rows", "lora_down", "attention_shared"]


@contextlib.contextmanager
def _patched(fns):
    """stllm_amd.hip with the entry points {name: function} swapped in; whatever was there before comes back on exit, so nesting is harmless"""
    from stllm_amd import hip
    saved = {n: getattr(hip, n) for n in fns}
    try:
        for n, f in fns.items():
            setattr(hip, n, f)
        yield
    finally:
        for n, f in saved.items():
            setattr(hip, n, f)


def installed():
    """Monkey-patch stllm_amd.hip's compute entry points with the functions above (tests only)."""
    return _patched({n: globals()[n] for n in NAMES})


@contextlib.contextmanager
def counting():
    """inside installed(): append the name of every COUNTED entry point that the host code calls to CALLS"""
    from stllm_amd import hip

    def wrap(name, f):
        def g(*a, **k):
            CALLS.append(name)
            return f(*a, **k)
        return g
    CALLS.clear()
    with _patched({n: wrap(n, getattr(hip, n)) for n in COUNTED}):
        yield CALLS
