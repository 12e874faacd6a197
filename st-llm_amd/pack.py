"""Weight packers: reference-named fp32 parameters -> the layouts the HIP kernels consume.

All packers are pure index permutations / concatenations / casts (done once, on the device the
parameter lives on); none changes the mathematical function:

* ``vit_qkv_bias``   — eva_vit.py:120-124: bias = cat(q_bias, zeros, v_bias).
* ``patch_weight``   — Conv2d weight [1408,3,14,14] -> GEMM weight [1408, 588] zero-padded in K to a
                       whole number of 128-byte LDS panels (640 for 16-bit, 608 for fp32).
* ``llama_qkv``      — q/k/v_proj fused to one [3*4096, 4096] weight.  Inside every 128-wide q/k head
                       the rows are re-ordered to [0:32 | 64:96 | 32:64 | 96:128] so that the rotate-half
                       partners (i, i+64) land in the two 32-column halves of one 64-column wave tile
                       and RoPE is an in-lane epilogue.  q and k get the SAME permutation, so q.k is
                       unchanged (spec of the rotation: modeling_llama_mem.py:113-127).
* ``llama_gate_up``  — gate/up_proj interleaved in groups of 32 rows ([32 gate | 32 up] per 64-column
                       wave tile) for the fused SiLU(gate)*up epilogue (modeling_llama_mem.py:143-144).
* ``bert_qkv`` / ``bert_kv`` — Q-Former query/key/value fused (Qformer.py:127-133).
* ``quant8_rows``    — the one packer that is NOT exact: a packed 16-bit weight -> int8 rows + one fp32 scale per row, the
                       weight format of the W8A16 decode kernels (hip.gemv_w8).
* ``quant4_groups``  — its 4-bit sibling: two weights per byte + one fp32 scale per row and 128-element K group, the weight
                       format of the W4A16 decode kernels (hip.gemv_q4); ``dequant4_groups`` undoes the nibble placement.
"""
import os

import torch

from . import runtime
from .hip import torch_dtype


def split3_weight(w):
    """fp32 [N, K] -> bf16 [N, 3 K] = (hi | lo | hi) along K, hi = bf16(w), lo = bf16(w - hi): the weight operand of the "bf16x3" GEMMs
    (stllm_hip.h STLLM_BF16X3; the same rounding as stllm_split3_rows side 1)."""
    wf = w.detach().float()
    hi = wf.to(torch.bfloat16)
    lo = (wf - hi.float()).to(torch.bfloat16)
    return torch.cat((hi, lo, hi), dim=1).contiguous()


def _cast(w, dtype):
    td = torch_dtype(dtype)
    if td == torch.float32 and runtime.gemm_split() and w.dim() == 2 and w.shape[1] % 64 == 0:
        return split3_weight(w)
    return w.detach().to(td).contiguous()


def linear(w, dtype):
    return _cast(w, dtype)


def f32(b):
    return None if b is None else b.detach().float().contiguous()


def vit_qkv_bias(q_bias, v_bias):
    return torch.cat((q_bias.detach().float(), torch.zeros_like(v_bias, dtype=torch.float32), v_bias.detach().float())).contiguous()


def patch_k_padded(dtype):
    eb = 4 if torch_dtype(dtype) == torch.float32 else 2
    panel = 128 // eb
    return ((588 + panel - 1) // panel) * panel


def patch_weight(w, dtype):
    n = w.shape[0]
    out = torch.zeros((n, patch_k_padded(dtype)), device=w.device, dtype=torch_dtype(dtype))
    out[:, :588] = w.detach().reshape(n, 588).to(out.dtype)
    return out


def rope_head_perm(n_heads, head_dim=128, device="cpu"):
    assert head_dim == 128
    base = torch.cat([torch.arange(0, 32), torch.arange(64, 96), torch.arange(32, 64), torch.arange(96, 128)])
    return (torch.arange(n_heads)[:, None] * head_dim + base[None, :]).reshape(-1).to(device)


def llama_qkv(wq, wk, wv, dtype, n_heads=32):
    perm = rope_head_perm(n_heads, wq.shape[0] // n_heads, wq.device)
    return torch.cat((_cast(wq, dtype)[perm], _cast(wk, dtype)[perm], _cast(wv, dtype)), dim=0).contiguous()


def llama_gate_up(wg, wu, dtype):
    n, k = wg.shape
    assert n % 32 == 0
    g = _cast(wg, dtype)
    u = _cast(wu, dtype)
    k = g.shape[1]   # 3 K in the split mode
    return torch.stack((g.view(n // 32, 32, k), u.view(n // 32, 32, k)), dim=1).reshape(2 * n, k).contiguous()


def quant8_rows(w16):
    """packed weight [N, K] -> (q int8 [N, K] contiguous, scale f32 [N]) for hip.gemv_w8: symmetric, one scale per output row.
    amax = max |w| over the row (fp32); scale = amax / 127, an fp32 division (1 for an all-zero row); q = clamp(rint(w / scale), -127, 127),
    round-half-even (-128 never occurs).  The quotient w / scale is taken in fp64, where w and scale are exact: an fp32 quotient can be rounded
    ONTO a tie k + 1/2 from below and then away from w (measured: |w - q scale| = (1 + 3.5e-6) scale / 2), the fp64 one keeps
    |w - q scale| <= scale / 2 (1 + 2^-20).  Every step is one correctly rounded IEEE operation, so the CPU and the device agree bit for bit.
    Works on the PACKED weight: the RoPE head permutation of llama_qkv and
    the [32 gate | 32 up] interleave of llama_gate_up are row permutations, and a per-row scale commutes with those."""
    assert w16.dim() == 2
    wf = w16.detach().float()
    amax = wf.abs().amax(dim=1)
    scale = torch.where(amax > 0, amax / 127.0, torch.ones_like(amax))
    q = torch.clamp(torch.round(wf.double() / scale.double()[:, None]), -127.0, 127.0).to(torch.int8)
    return q.contiguous(), scale.contiguous()


Q4_GROUP = 128
_Q4_LO, _Q4_HI = (0, 4, 1, 5), (2, 6, 3, 7)   # elements of an 8-element piece in the low / high nibbles of its 4 bytes


def quant4_groups(w16, group=Q4_GROUP):
    """packed weight [N, K] (K % 128 == 0) -> (qp uint8 [N, K / 2] contiguous, scale f32 [N, K / 128] contiguous) for hip.gemv_q4: symmetric, one
    scale per output row and group of 128 consecutive K elements.  amax = max |w| over the group (fp32); scale = amax / 7, an fp32 division (1 for an
    all-zero group); q = clamp(rint(w / scale), -7, 7), round-half-even, the quotient taken in fp64 for the reason given in quant8_rows (so
    |w - q scale| <= scale / 2 (1 + 2^-20)); -8 never occurs.  Stored nibble u = q + 8 in [1, 15].
    Nibble placement, a fixed permutation inside every 8-element piece (so every 8-, 32- or 128-aligned slice of K is self-contained): read as a
    little-endian dword, the 4 bytes of piece j hold element 8 j + 2 t at bits [4 t, 4 t + 4) and element 8 j + 2 t + 1 at bits [16 + 4 t, 16 + 4 t + 4),
    t = 0..3 — byte b carries the elements (0, 2), (4, 6), (1, 3), (5, 7)[b] in its (low, high) nibble.  In a register `(w >> 4 t) & 0x000f000f` is then
    the K-adjacent pair t with one nibble at the bottom of each 16-bit half, ready to have a float exponent or-ed onto it (csrc/gemv.hip, Q4).
    Only this function, dequant4_groups and the kernel know the placement.  Like quant8_rows it works on the PACKED weight: a per-(row, group)
    scale commutes with the row permutations of llama_qkv / llama_gate_up."""
    assert w16.dim() == 2 and group == Q4_GROUP, "the kernels of hip.gemv_q4 serve groups of 128"
    n, k = w16.shape
    assert k % group == 0, f"quant4_groups: K = {k} is no multiple of {group}"
    wf = w16.detach().float().view(n, k // group, group)
    amax = wf.abs().amax(dim=2)
    scale = torch.where(amax > 0, amax / 7.0, torch.ones_like(amax))
    u = (torch.clamp(torch.round(wf.double() / scale.double()[:, :, None]), -7.0, 7.0) + 8.0).to(torch.uint8).view(n, k // 8, 8)
    qp = u[:, :, _Q4_LO] | (u[:, :, _Q4_HI] << 4)
    return qp.reshape(n, k // 2).contiguous(), scale.contiguous()


def dequant4_groups(qp, scale):
    """the inverse of quant4_groups' nibble placement: (qp uint8 [N, K / 2], scale) -> (q int8 [N, K] in logical K order, |q| <= 7, scale unchanged);
    the weight the format stands for is q.view(N, K / 128, 128) * scale[:, :, None]"""
    n, kb = qp.shape
    b = qp.view(n, kb // 4, 4)
    u = torch.empty((n, kb // 4, 8), dtype=torch.uint8, device=qp.device)
    u[:, :, _Q4_LO] = b & 15
    u[:, :, _Q4_HI] = b >> 4
    return (u.view(n, 2 * kb).to(torch.int16) - 8).to(torch.int8), scale


def frag32(w):
    """fragment-major copy of a packed 16-bit weight [N, K] (N % 32 == 0, K % 16 == 0) for the W-direct GEMM (csrc/gemm_wd.inc, stllm_gemm_args.w_frag):
    [N / 32][K / 16][64 lanes][8 elements], lane l of fragment (nb, ks) = w[32 nb + (l & 31), 16 ks + 8 (l >> 5) : + 8] — the operand of one
    v_mfma_f32_32x32x16 as one contiguous KiB."""
    n, k = w.shape
    assert n % 32 == 0 and k % 16 == 0 and w.element_size() == 2
    #            nb      row      ks     half   e            nb ks half row e  -> lane = half * 32 + row
    return w.reshape(n // 32, 32, k // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous().reshape(-1)


def frag32_or_none(w):
    """frag32(w) where the W-direct kernel can use it: a 16-bit weight on the GPU with N % 256 == 0 and K % 256 == 0 (un-padded, contiguous rows);
    STLLM_WD_FRAG=0 in the environment: never (the prefill runs on the other kernels, no second copy of the weights)."""
    if os.environ.get("STLLM_WD_FRAG", "1") == "0" or not w.is_cuda or w.dim() != 2 or w.element_size() != 2 or not w.is_contiguous():
        return None
    n, k = w.shape
    if n % 256 or k % 256 or n * k * 2 >= (1 << 32):
        return None
    return frag32(w)


def bert_qkv(q, k, v, dtype):
    w = torch.cat((_cast(q.weight, dtype), _cast(k.weight, dtype), _cast(v.weight, dtype)), dim=0).contiguous()
    b = torch.cat((f32(q.bias), f32(k.bias), f32(v.bias))).contiguous()
    return w, b


def bert_kv(k, v, dtype):
    w = torch.cat((_cast(k.weight, dtype), _cast(v.weight, dtype)), dim=0).contiguous()
    b = torch.cat((f32(k.bias), f32(v.bias))).contiguous()
    return w, b


def pad_rows(w, mult=128):
    """zero-pad the out_features dim to a multiple of `mult` (lm_head with a 32001-token vocab)."""
    n = w.shape[0]
    n_pad = ((n + mult - 1) // mult) * mult
    if n_pad == n:
        return w
    out = torch.zeros((n_pad,) + tuple(w.shape[1:]), device=w.device, dtype=w.dtype)
    out[:n] = w
    return out


def rope_tables(S, head_dim=128, base=10000.0, device="cpu"):
    """cos/sin [S, head_dim/2] fp32 — LlamaRotaryEmbedding (modeling_llama_mem.py:81-110); computed on the
    host in fp32 exactly as the reference does, then copied to the device."""
    inv = 1.0 / (base ** (torch.arange(0, head_dim, 2, dtype=torch.float32) / head_dim))
    f = torch.outer(torch.arange(S, dtype=torch.float32), inv)
    return f.cos().contiguous().to(device), f.sin().contiguous().to(device)
