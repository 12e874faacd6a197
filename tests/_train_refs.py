"""TEST-ONLY: plain fp64 references of the backward / optimizer entry points of include/stllm_hip.h ("Backward / optimizer entry points"), one
function per entry point, torch float64 on the CPU, written from the formulas of the header.  Where the op is the transpose of a differentiable
forward, the forward is here too (`*_fwd`), so that tests/test_train_refs_cpu.py can check every closed form against torch.autograd; the same
file checks them against the fp32 restatements of tests/_cpu_backend.py, so the two statements of each contract cannot drift apart.

Operands are LOGICAL tensors (no strides, no padding): attention takes [B, S, H, D]; the packed column layouts ([32 gate | 32 up] groups,
[32 x1 | 32 x2] rotary halves) are the header's.  Everything a caller passes is converted with .double() first.

Also here, because both the CPU and the GPU file need them:
  * ATTN_CASES — the attention-backward case table of tests/test_train_kernels_gpu.py and attn_inputs(), its inputs;
  * attention_bwd_model16 — the DESIGNED rounding of the 16-bit MFMA kernels (P and dS rounded to 16 bit before the second product, each
    output rounded once), which shows without running a kernel that the 16-bit bounds are reachable by a correct one."""
import math

import torch

F64 = torch.float64
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
# tests/test_kernels_emulated_cpu.py::test_attention_bwd: fp32 2e-5 of abs-max; 16 bit 2 * TOL with TOL = 2^-7 (bf16), 2^-10 (fp16)
ATTN_TOL = {"fp32": 2e-5, "bf16": 2.0 ** -6, "fp16": 2.0 ** -9}


def _d(t):
    return t.detach().double().cpu()


# ---- layout -----------------------------------------------------------------------------------------------------------------------------------
def transpose(x, pad=64):
    """dst[c, r] = src[r, c] for r < rows, 0 for rows <= r < rows_padded (rows rounded up to `pad`); exact, in x's own dtype"""
    R, C = x.shape
    Rp = (R + pad - 1) // pad * pad
    out = torch.zeros((C, Rp), dtype=x.dtype)
    out[:, :R] = x.cpu().t()
    return out


# ---- norms ------------------------------------------------------------------------------------------------------------------------------------
def rmsnorm_fwd(x, gamma, eps):
    return gamma * x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)


def rmsnorm_bwd(x, gamma, eps, dy):
    """r = rsqrt(mean(x^2) + eps), xh = x r, g = gamma dy:  dx = r (g - xh mean(g xh)),  dgamma = sum_rows dy xh"""
    x, gamma, dy = _d(x), _d(gamma), _d(dy)
    r = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    xh, g = x * r, gamma * dy
    return r * (g - xh * (g * xh).mean(-1, keepdim=True)), (dy * xh).sum(0)


def layernorm_fwd(x, gamma, beta, eps):
    mu = x.mean(-1, keepdim=True)
    return gamma * (x - mu) * torch.rsqrt((x - mu).pow(2).mean(-1, keepdim=True) + eps) + beta


def layernorm_bwd(x, gamma, eps, dy):
    """xh = (x - mu) r:  dx = r (g - mean(g) - xh mean(g xh)),  dgamma = sum dy xh,  dbeta = sum dy"""
    x, gamma, dy = _d(x), _d(gamma), _d(dy)
    mu = x.mean(-1, keepdim=True)
    r = torch.rsqrt((x - mu).pow(2).mean(-1, keepdim=True) + eps)
    xh, g = (x - mu) * r, gamma * dy
    return r * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True)), (dy * xh).sum(0), dy.sum(0)


def norm_terms(x, eps, dy, rms):
    """(sum_rows |dy xh|, sum_rows |dy|): the sums of absolute terms behind dgamma / dbeta, for the derived reduction bounds"""
    x, dy = _d(x), _d(dy)
    mu = torch.zeros_like(x[:, :1]) if rms else x.mean(-1, keepdim=True)
    xh = (x - mu) * torch.rsqrt((x - mu).pow(2).mean(-1, keepdim=True) + eps)
    return (dy * xh).abs().sum(0), dy.abs().sum(0)


# ---- SwiGLU on the packed [32 gate | 32 up] column groups ---------------------------------------------------------------------------------------
def _groups(x):
    M, N = x.shape
    return x.reshape(M, N // 64, 2, 32)


def swiglu_fwd(gu):
    """silu(gate) * up: gu [M, 2 I] -> [M, I]"""
    g = _groups(gu)
    gate, up = g[:, :, 0], g[:, :, 1]
    return (gate * torch.sigmoid(gate) * up).reshape(gu.shape[0], -1)


def swiglu(gu):
    return swiglu_fwd(_d(gu))


def swiglu_bwd(gu, dg):
    """d gate = dg up s (1 + gate (1 - s)),  d up = dg gate s,  s = sigmoid(gate); in the packed layout of gu"""
    g = _groups(_d(gu))
    gate, up = g[:, :, 0], g[:, :, 1]
    d = _d(dg).reshape(gate.shape)
    s = torch.sigmoid(gate)
    return torch.stack((d * up * s * (1 + gate * (1 - s)), d * gate * s), dim=2).reshape(gu.shape)


# ---- RoPE on the packed head layout: every 64-column group is (x1 | x2) of half a head, frequencies (group % 2) * 32 + j ----------------------
def _rope_cs(cos, sin, M, groups, rope_seq):
    pos = torch.arange(M) % rope_seq
    fi = (torch.arange(groups) % 2)[:, None] * 32 + torch.arange(32)[None, :]
    return _d(cos).reshape(-1, 64)[pos][:, fi], _d(sin).reshape(-1, 64)[pos][:, fi]       # [M, groups, 32]


def rope_fwd(x, cos, sin, rope_seq, rope_cols):
    """the ROPE epilogue's rotation: y1 = x1 c - x2 s,  y2 = x2 c + x1 s on the first rope_cols columns; the rest passes through"""
    M, N = x.shape
    ng = rope_cols // 64
    c, s = _rope_cs(cos, sin, M, ng, rope_seq)
    g = _groups(x[:, :rope_cols])
    x1, x2 = g[:, :, 0], g[:, :, 1]
    rot = torch.stack((x1 * c - x2 * s, x2 * c + x1 * s), dim=2).reshape(M, rope_cols)
    return torch.cat((rot, x[:, rope_cols:]), dim=1)


def rope_bwd(d, cos, sin, rope_seq, rope_cols):
    """its transpose: dx1 = dy1 c + dy2 s,  dx2 = dy2 c - dy1 s"""
    d = _d(d)
    M, N = d.shape
    ng = rope_cols // 64
    c, s = _rope_cs(cos, sin, M, ng, rope_seq)
    g = _groups(d[:, :rope_cols])
    y1, y2 = g[:, :, 0], g[:, :, 1]
    rot = torch.stack((y1 * c + y2 * s, y2 * c - y1 * s), dim=2).reshape(M, rope_cols)
    return torch.cat((rot, d[:, rope_cols:]), dim=1)


# ---- attention --------------------------------------------------------------------------------------------------------------------------------
def _visible(B, Sq, Skv, causal, kv_len):
    """[B, 1, Sq, Skv] bool: key j visible to query i of batch row b"""
    vis = torch.ones(B, 1, Sq, Skv, dtype=torch.bool)
    if causal:
        vis &= (torch.arange(Skv)[None, :] <= torch.arange(Sq)[:, None])[None, None]
    if kv_len is not None:
        vis &= (torch.arange(Skv)[None, :] < torch.as_tensor(kv_len).long().clamp(max=Skv)[:, None])[:, None, None, :]
    return vis


def attention_probs(q, k, scale, causal, kv_len):
    """P [B, H, Sq, Skv] = softmax(scale q k^T + masks); a row with no visible key (kv_len[b] <= 0) is all zeros, never NaN"""
    qh, kh = q.transpose(1, 2), k.transpose(1, 2)
    B, _, Sq, _ = qh.shape
    vis = _visible(B, Sq, kh.shape[2], causal, kv_len)
    s = ((qh @ kh.transpose(-1, -2)) * scale).masked_fill(~vis, float("-inf"))
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    return e / torch.where(l > 0, l, torch.ones_like(l))


def attention_fwd(q, k, v, scale, causal=False, kv_len=None):
    """o [B, Sq, H, D] of q [B, Sq, H, D], k, v [B, Skv, H, D]"""
    return (attention_probs(q, k, scale, causal, kv_len) @ v.transpose(1, 2)).transpose(1, 2)


def attention_bwd(q, k, v, o, do, scale, causal=False, kv_len=None):
    """the closed form, P and dS in fp64:  delta = dO . o (the o the kernel receives),  dS = P (dO V^T - delta),
    dQ = scale dS K,  dK = scale dS^T Q,  dV = P^T dO.  A batch row with kv_len[b] <= 0 has P = 0: zero dq, dk and dv."""
    q, k, v, o, do = (_d(t) for t in (q, k, v, o, do))
    p = attention_probs(q, k, scale, causal, kv_len)
    qh, kh, vh, oh, doh = (t.transpose(1, 2) for t in (q, k, v, o, do))
    delta = (doh * oh).sum(-1, keepdim=True)
    ds = p * (doh @ vh.transpose(-1, -2) - delta)
    dq = (ds @ kh) * scale
    dk = (ds.transpose(-1, -2) @ qh) * scale
    dv = p.transpose(-1, -2) @ doh
    return dq.transpose(1, 2), dk.transpose(1, 2), dv.transpose(1, 2)


def attention_bwd_model16(q, k, v, o, do, scale, causal, kv_len, dtype):
    """what the 16-bit MFMA kernels compute BY DESIGN, everything else exact: P and dS are rounded to `dtype` before the second matrix product
    (they are its 16-bit B operand), each output is rounded once."""
    q, k, v, o, do = (_d(t) for t in (q, k, v, o, do))
    r = lambda t: t.to(dtype).double()
    p = attention_probs(q, k, scale, causal, kv_len)
    qh, kh, vh, oh, doh = (t.transpose(1, 2) for t in (q, k, v, o, do))
    delta = (doh * oh).sum(-1, keepdim=True)
    ds = r(p * (doh @ vh.transpose(-1, -2) - delta))
    p = r(p)
    dq = r((ds @ kh) * scale)
    dk = r((ds.transpose(-1, -2) @ qh) * scale)
    dv = r(p.transpose(-1, -2) @ doh)
    return dq.transpose(1, 2), dk.transpose(1, 2), dv.transpose(1, 2)


# name, B, H, Sq, Skv, D, causal, kv_len, kind ("plain" | "peaked"); every case runs in bf16, fp16 (MFMA) and fp32 (VALU) unless `only`
ATTN_CASES = [
    ("llama_127", 2, 3, 127, 127, 128, True, None, "plain"),            # one workgroup, last wave one query short
    ("llama_128", 2, 3, 128, 128, 128, True, None, "plain"),            # exactly one 128-row workgroup
    ("llama_129", 2, 3, 129, 129, 128, True, None, "plain"),            # a second workgroup that owns one row
    ("llama_129_len", 2, 3, 129, 129, 128, True, [129, 32], "plain"),   # kv_len on a tile edge
    ("llama_160_len1", 2, 3, 160, 160, 128, True, [1, 97], "plain"),    # one visible key: P = 1, dS = 0
    ("llama_300_len", 2, 3, 300, 300, 128, True, [300, 131], "plain"),
    ("llama_160_len0", 2, 3, 160, 160, 128, True, [0, 160], "plain"),   # no visible key: zero gradients for that batch row
    ("eva_257", 2, 2, 257, 257, 88, False, None, "plain"),              # D = 88 padded to 96 in LDS
    ("qf_self", 2, 3, 64, 64, 64, False, [64, 33], "plain"),
    ("qf_cross", 2, 3, 32, 257, 64, False, None, "plain"),              # Sq != Skv
    ("d40", 2, 3, 70, 70, 40, False, None, "plain"),                    # head dims the ABI accepts and the model does not use
    ("d72", 2, 3, 70, 70, 72, False, None, "plain"),
    ("d104", 2, 3, 70, 70, 104, False, None, "plain"),
    ("peaked_causal", 2, 3, 257, 257, 128, True, None, "peaked"),
    ("peaked_full", 2, 3, 257, 257, 128, False, None, "peaked"),
]
ATTN_BF16_ONLY = ("d40", "d72", "d104")
ATTN_IDS = [c[0] for c in ATTN_CASES]
DEAD_KV = 1.0e3      # magnitude of the K / V rows in [kv_len[b], Skv): read, weightless, must be finite


def attn_inputs(case, dtype):
    """(q, k, v, o, do) of a case as fp64 [B, S, H, D] tensors whose values are exactly representable in `dtype` (rounded first, so that a kernel
    and the reference see the same numbers).  o is the fp64 forward of the rounded q, k, v, rounded to `dtype` — the o a kernel receives.
    plain: q, k ~ N(0, 0.7^2), v, dO ~ N(0, 1) + a small offset (asymmetric).  peaked: q, k ~ N(0, 3^2), key row j scaled by 0.2 + 0.8 j / S, so
    that one weight dominates each row and the running max rises through the key sweep.  K / V rows behind kv_len[b] hold +-DEAD_KV."""
    name, B, H, Sq, Skv, D, causal, kv_len, kind = case
    td = DTYPES[dtype] if isinstance(dtype, str) else dtype
    g = torch.Generator().manual_seed(1000 + ATTN_IDS.index(name))
    n = lambda S, std: torch.randn(B, S, H, D, generator=g, dtype=F64) * std
    if kind == "peaked":
        q, k = n(Sq, 3.0), n(Skv, 3.0) * (0.2 + 0.8 * torch.arange(Skv, dtype=F64) / Skv)[None, :, None, None]
    else:
        q, k = n(Sq, 0.7), n(Skv, 0.7) + 0.05
    v, do = n(Skv, 1.0) + 0.1, n(Sq, 1.0) - 0.05
    if kv_len is not None:
        sign = torch.where(torch.arange(D) % 2 == 0, 1.0, -1.0).double()
        for b, L in enumerate(kv_len):
            k[b, max(L, 0):] = DEAD_KV * sign
            v[b, max(L, 0):] = -DEAD_KV * sign
    q, k, v, do = (t.to(td).double() for t in (q, k, v, do))
    o = attention_fwd(q, k, v, D ** -0.5, causal, kv_len).to(td).double()
    return q, k, v, o, do


# ---- losses / rows ------------------------------------------------------------------------------------------------------------------------------
def cross_entropy_fwd(logits, labels, scale, vocab):
    """scale * sum over the rows with labels >= 0 of  logsumexp(logits[i, :vocab]) - logits[i, labels[i]]"""
    lab = labels.long()
    ok = lab >= 0
    x = logits[:, :vocab]
    return scale * (torch.logsumexp(x[ok], -1) - x[ok].gather(1, lab[ok][:, None])[:, 0]).sum()


def cross_entropy_bwd(logits, labels, scale, vocab):
    """dlogits[i, c] = scale (softmax(logits[i, :vocab])[c] - [c == labels[i]]) for labels[i] >= 0, else 0; columns >= vocab are 0"""
    x = _d(logits)
    lab = labels.long().cpu()
    out = torch.zeros_like(x)
    out[:, :vocab] = torch.softmax(x[:, :vocab], -1)
    ok = lab >= 0
    out[ok, lab[ok]] -= 1.0
    out[~ok] = 0.0
    return out * scale


def gather_fwd(dst_a, dst_b, idx):
    """stllm_gather_rows with scale 1: row i is dst_a[idx[i]] (idx >= 0) or dst_b[-idx[i] - 1]"""
    return torch.stack([dst_a[i] if i >= 0 else dst_b[-i - 1] for i in idx.tolist()])


def scatter_add_rows(src, idx, dst_a, dst_b, scale):
    """(idx[i] >= 0 ? dst_a[idx[i]] : dst_b[-idx[i] - 1]) += scale src[i]; returns the new (dst_a, dst_b)"""
    src, a = _d(src), _d(dst_a).clone()
    b = _d(dst_b).clone() if dst_b is not None else None
    for i, j in enumerate(idx.tolist()):
        if j >= 0:
            a[j] += scale * src[i]
        else:
            b[-j - 1] += scale * src[i]
    return a, b


def cosine_rows_fwd(a, b, idx_a, idx_b):
    """out[i] = 2 - 2 <a_i / |a_i|, b_i / |b_i|>, rows gathered by index"""
    aa = a if idx_a is None else a[idx_a.long()]
    bb = b if idx_b is None else b[idx_b.long()]
    return 2 - 2 * (aa * bb).sum(-1) / (aa.norm(dim=-1) * bb.norm(dim=-1))


def cosine_rows_bwd(a, b, idx_a, idx_b, scale):
    """da[i] = -2 scale / |a_i| (b_i / |b_i| - cos_i a_i / |a_i|)  w.r.t. the GATHERED a rows"""
    a, b = _d(a), _d(b)
    aa = a if idx_a is None else a[idx_a.long().cpu()]
    bb = b if idx_b is None else b[idx_b.long().cpu()]
    na, nb = aa.norm(dim=-1, keepdim=True), bb.norm(dim=-1, keepdim=True)
    cs = (aa * bb).sum(-1, keepdim=True) / (na * nb)
    return -2 * scale / na * (bb / nb - cs * aa / na)


def colsum(x):
    return _d(x).sum(0)


def relu_fwd(x):
    return x.clamp(min=0)


def relu_bwd(dy, y):
    """dx = dy (y > 0)"""
    return _d(dy) * (_d(y) > 0)


def gelu_fwd(x):
    """exact-erf GELU: x Phi(x)"""
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2.0)))


def gelu(x):
    return gelu_fwd(_d(x))


def gelu_bwd(x, dy):
    """dy (Phi(x) + x phi(x))"""
    x = _d(x)
    return _d(dy) * (0.5 * (1 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi))


def scale_rows_fwd(x, scale, idx):
    return x * scale[idx.long()][:, None]


def scale_rows(x, scale, rows_per_group=0, idx=None):
    """x[r, :] *= scale[idx ? idx[r] : r / rows_per_group] — linear and diagonal: its own backward"""
    g = idx.long().cpu() if idx is not None else torch.arange(x.shape[0]) // rows_per_group
    return _d(x) * _d(scale)[g][:, None]


def mean_t_fwd(x):
    return x.mean(1)


def bcast_add_t(dst, src, scale):
    """dst[b, t, j] += scale src[b, j]; stays on the device of its operands (fp64 there: a host copy of the large case would dominate the test)"""
    return dst.double() + scale * src.double().unsqueeze(1)


def adamw(p, g, m, v, *, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
    """g' = grad_scale g;  p *= 1 - lr wd;  m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2;
    p -= lr / (1 - b1^step) m / (sqrt(v) / sqrt(1 - b2^step) + eps); returns the new (p, m, v)"""
    p, g, m, v = (_d(t) for t in (p, g, m, v))
    g = g * grad_scale
    p = p * (1 - lr * weight_decay)
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    p = p - lr / (1 - beta1 ** step) * m / (v.sqrt() / math.sqrt(1 - beta2 ** step) + eps)
    return p, m, v


def sumsq(x):
    return _d(x).pow(2).sum()


# ---- comparison -----------------------------------------------------------------------------------------------------------------------------------
def rel_err(got, ref):
    """max |got - ref| over abs-max of ref, in fp64"""
    got, ref = _d(got), _d(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return ((got - ref).abs().max() / max(ref.abs().max().item(), 1e-30)).item()
