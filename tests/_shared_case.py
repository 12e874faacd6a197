"""TEST-ONLY: inputs and the fp64 reference of stllm_attention_shared, shared by tests/test_shared_prefix_cpu.py (host emulation) and
tests/test_shared_prefix_gpu.py.  Everything at or behind P in the prefix buffers and at or behind sfx_len[b] in the suffix buffers is NaN: an output
that is finite proves that nothing behind the bounds was read."""
import numpy as np
import torch

D = 128


def make(td, G, R, H, P, sfx, Sq=1, seed=0, pre_pad=3, sfx_pad=6, device="cpu"):
    """fused [q | k | v] prefix buffer [G, P + pre_pad, 3HD] and suffix buffer [B, max(sfx) + sfx_pad, 3HD] (different max_len = different strides),
    queries [B * Sq, 3HD] (the q columns of a dense fused buffer)"""
    g = torch.Generator().manual_seed(1000 + seed)
    B, W = G * R, 3 * H * D
    MLp, MLs = P + pre_pad, max(sfx) + sfx_pad
    pre = torch.randn((G, MLp, W), generator=g).to(td)
    suf = torch.randn((B, MLs, W), generator=g).to(td)
    q = torch.randn((B * Sq, W), generator=g).to(td)
    pre[:, P:] = float("nan")
    for b, n in enumerate(sfx):
        suf[b, n:] = float("nan")
    return pre.to(device), suf.to(device), q.to(device)


def reference(pre, suf, q, G, R, H, P, sfx, Sq=1, causal=False, q_off=0):
    """fp64 softmax over the concatenated live keys; returns [B * Sq, HD] and the mask [B, Sq] of query rows whose output is defined
    (Sq > 1: rows at or behind a row's own length are don't-care)"""
    B = G * R
    out = torch.zeros((B * Sq, H * D), dtype=torch.float64)
    live = torch.ones((B, Sq), dtype=torch.bool)
    pre, suf, q = pre.double().cpu(), suf.double().cpu(), q.double().cpu()
    for b in range(B):
        g = b // R
        kp = pre[g, :P].view(P, 3, H, D)
        ksf = suf[b, :sfx[b]].view(sfx[b], 3, H, D)
        for i in range(Sq):
            n = min(sfx[b], q_off + i + 1) if causal else sfx[b]
            if Sq > 1 and causal and q_off + i >= sfx[b]:
                live[b, i] = False
            k = torch.cat([kp[:, 1], ksf[:n, 1]]).transpose(0, 1)     # [H, P + n, D]
            v = torch.cat([kp[:, 2], ksf[:n, 2]]).transpose(0, 1)
            qq = q[b * Sq + i].view(3, H, D)[0]
            s = (qq.unsqueeze(1) @ k.transpose(-1, -2)) * D ** -0.5
            out[b * Sq + i] = (torch.softmax(s, dim=-1) @ v).reshape(H * D)
    return out, live


def call(hip, pre, suf, q, G, R, H, P, sfx, Sq=1, causal=False, q_off=0, ragged=True):
    B, W, HD = G * R, 3 * H * D, H * D
    MLp, MLs = pre.shape[1], suf.shape[1]
    sl = torch.tensor(sfx, dtype=torch.int32).to(q.device) if ragged else None
    pf, sf = pre.view(G * MLp, W), suf.view(B * MLs, W)
    return hip.attention_shared(q[:, :HD], pf[:, HD:2 * HD], pf[:, 2 * HD:], sf[:, HD:2 * HD], sf[:, 2 * HD:], B=B, G=G, H=H, Sq=Sq, P=P, D=D,
                                scale=D ** -0.5, max_sfx=max(sfx), sfx_len=sl, sfx_q_off=q_off, causal=causal,
                                q_strides=(Sq * W, W), kp_strides=(MLp * W, W), ks_strides=(MLs * W, W))


def draw_lens(B, seed, hi=300):
    """B - 1 suffix lengths from a fixed seed in [1, hi] plus one row of length 1 (B = 1: the drawn length)"""
    rs = np.random.RandomState(4321 + seed)
    lens = [int(x) for x in rs.randint(1, hi + 1, size=max(B - 1, 1))]
    return lens + [1] if B > 1 else lens
