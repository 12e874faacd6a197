"""TEST-ONLY: the cases of stllm_attention's dispatch tests (tests/test_attention_dispatch_gpu.py on the device, tests/test_attention_dispatch_cpu.py through the
host emulation of the same sources): the inputs, the fp64 reference, the kernel names the dispatcher must report, and the run-and-compare routine they share.

Layout, as the model calls it: q / k / v are column slices of one fused buffer [B, rows, 3 H D] (Sq == Skv) or of a q buffer and a fused [k | v] buffer;
every buffer has three rows more per batch entry than the call uses and those rows are NaN (never read: include/stllm_hip.h, memory regions).  The K / V rows
in [kv_len[b], Skv) stay finite (read, weightless).  The output sits in a _poison.Guarded buffer.

Two input sets per shape.  RANDOM: N(0, 1) rounded to the compute dtype.  PLANTED: the same, plus keys that make every mask boundary the case is about
decide the output.  At the bf16 tolerance random inputs do not: one key more or less moves a row by about 1 / (keys it sees).
  * kv_len boundary L < Skv of batch row b: a common direction u (+-1 per dim) is added to every Q row of b, K[L - 1] = K[L] = 2 u, V[L - 1] = +4, V[L] = -4;
  * the end of Skv inside a 32-key tile (no causal mask, kv_len = Skv): the same with the key Skv - 1 alone — the key behind it is the NaN row;
  * causal boundary (batch rows without a kv_len boundary): for the query rows r in {0, 31, 32, last, one per 32-row tile}: K[r] = K[r + 1] = 2 Q[r],
    V[r] = +4, V[r + 1] = -4, two neighbouring r never in the same head.
All planted values are exact in bf16.  Inputs.__init__ asserts in fp64, before any kernel runs, that moving each planted boundary by one key in either direction
displaces the reference of the rows that see it by at least 4 x the tolerance of the comparison (`sensitivity`, relative to max |ref| like the tolerance).
A boundary that does not exist is listed in `exempt` with its reason (kv_len = Skv under the causal mask is the causal boundary; Skv on a tile edge)."""
import functools
from typing import NamedTuple, Optional, Tuple

import torch

import _poison

OUT_TOL = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -10}   # tests/test_kernels_gpu.py: attention vs fp64 of the same inputs is 2 x this x abs-max
EMU_TOL = {torch.bfloat16: 4 * 2.0 ** -7, torch.float16: 4 * 2.0 ** -10, torch.float32: 2e-5}   # test_emulated_forward_attention_matches_contract: 4 * TOL
TNAME = {torch.bfloat16: "bf16_t", torch.float16: "f16_t"}
DEFAULTS = {"attn_dma": 1, "attn_q_lds": 1, "attn_f32_mfma": 1}
PAD_ROWS = 3


def tol_of(dtype):
    return 2e-5 if dtype == torch.float32 else 2 * OUT_TOL[dtype]


class Shape(NamedTuple):
    B: int
    H: int
    Sq: int
    Skv: int
    D: int
    causal: bool
    kv_len: Optional[Tuple[int, ...]] = None

    @property
    def id(self):
        s = f"B{self.B}H{self.H}D{self.D}-{self.Sq}x{self.Skv}{'c' if self.causal else ''}"
        return s if self.kv_len is None else s + "-kv" + "_".join(map(str, self.kv_len))


def attn_ref(q, k, v, scale, vis):
    """plain masked softmax in fp64: q [B, H, Sq, D], k / v [B, H, Skv, D], vis bool [B, Sq, Skv]"""
    s = (q @ k.transpose(-1, -2)) * scale
    return s.masked_fill(~vis[:, None], float("-inf")).softmax(-1) @ v


def visible(shape):
    B, Sq, Skv = shape.B, shape.Sq, shape.Skv
    vis = torch.ones(B, Sq, Skv, dtype=torch.bool)
    if shape.causal:
        vis &= ~torch.ones(Sq, Skv).triu(1).bool()
    if shape.kv_len is not None:
        vis &= (torch.arange(Skv)[None, :] < torch.tensor(shape.kv_len)[:, None])[:, None, :]
    return vis


def causal_rows(S):
    """the query rows whose causal boundary is planted: tile edges, the last row, one row per 32-row query tile"""
    return sorted({r for r in [0, 31, 32, S - 1] + [min(32 * t + 13, S - 1) for t in range((S + 31) // 32)] if 0 <= r < S})


class Inputs:
    """inputs of one (shape, dtype, planted) on the host, their fp64 reference (computed once, never changed) and, lazily, the copies on a device"""

    def __init__(self, shape, dtype, planted):
        self.shape, self.dtype, self.planted = shape, dtype, planted
        B, H, Sq, Skv, D = shape.B, shape.H, shape.Sq, shape.Skv, shape.D
        HD = H * D
        g = torch.Generator().manual_seed(1000 * D + 7 * Sq + Skv)
        self.fused = Sq == Skv
        if self.fused:
            big = torch.randn(B, Skv + PAD_ROWS, 3 * HD, generator=g)
            Q, K, V = (big[:, :, i * HD:(i + 1) * HD].unflatten(-1, (H, D)) for i in range(3))
            bufs = [big]
        else:
            qb, kvb = torch.randn(B, Sq + PAD_ROWS, HD, generator=g), torch.randn(B, Skv + PAD_ROWS, 2 * HD, generator=g)
            Q, K, V = qb.unflatten(-1, (H, D)), kvb[:, :, :HD].unflatten(-1, (H, D)), kvb[:, :, HD:].unflatten(-1, (H, D))
            bufs = [qb, kvb]
        for t in bufs:   # rounded to the compute dtype first: the planted rows below copy ROUNDED query rows
            t.copy_(t.to(dtype).float())
        self.boundaries, self.exempt = [], []
        if planted:
            self._plant(Q, K, V, torch.Generator().manual_seed(77))
        bufs[0][:, Sq:] = float("nan")
        bufs[-1][:, Skv:] = float("nan")
        self.host = [t.to(dtype) for t in bufs]
        self.kv_len = None if shape.kv_len is None else torch.tensor(shape.kv_len, dtype=torch.int32)
        h64 = [t.double() for t in self.host]
        if self.fused:
            q64, k64, v64 = (h64[0][:, :Sq, i * HD:(i + 1) * HD].unflatten(-1, (H, D)).transpose(1, 2) for i in range(3))
        else:
            q64 = h64[0][:, :Sq].unflatten(-1, (H, D)).transpose(1, 2)
            k64, v64 = (h64[1][:, :Skv, i * HD:(i + 1) * HD].unflatten(-1, (H, D)).transpose(1, 2) for i in range(2))
        self.scale = D ** -0.5
        vis = visible(shape)
        self.ref = attn_ref(q64, k64, v64, self.scale, vis).transpose(1, 2).reshape(B * Sq, HD)
        self.ref_max = max(float(self.ref.abs().max()), 1e-6)
        self.sensitivity = self._sensitivity(q64, k64, v64, vis) if planted else None
        if planted:   # the fixture's own precondition (reference only)
            assert self.boundaries, (shape.id, "a planted input set without a boundary", self.exempt)
            assert self.sensitivity >= 4 * tol_of(dtype), (shape.id, dtype, self.sensitivity, 4 * tol_of(dtype))
        self._dev = {}

    def _plant(self, Q, K, V, g):
        s = self.shape
        u = (torch.randint(0, 2, (s.H, s.D), generator=g) * 2 - 1).float()
        for b in range(s.B):
            L = s.Skv if s.kv_len is None else s.kv_len[b]
            if L < s.Skv:
                Q[b, :s.Sq] = (Q[b, :s.Sq] + u).to(self.dtype).float()
                K[b, L - 1], K[b, L], V[b, L - 1], V[b, L] = 2 * u, 2 * u, 4.0, -4.0
                self.boundaries.append(dict(kind="kv_len", b=b, h=None, rows=None, key_in=L - 1, key_out=L))
            elif s.causal:
                if s.kv_len is not None:
                    self.exempt.append((b, "kv_len = Skv under the causal mask: the boundary of row b is the causal one, planted below"))
                used = [set() for _ in range(s.H)]
                for i, r in enumerate(causal_rows(s.Sq)):
                    for h in [(i + d) % s.H for d in range(s.H)]:
                        if not ({r, r + 1} & used[h]):
                            break
                    else:
                        self.exempt.append((b, f"causal row {r}: its keys are a neighbouring planted row's in every head (H = {s.H})"))
                        continue
                    used[h] |= {r, r + 1}
                    K[b, r, h], V[b, r, h] = 2 * Q[b, r, h], 4.0
                    if r + 1 < s.Skv:
                        K[b, r + 1, h], V[b, r + 1, h] = 2 * Q[b, r, h], -4.0
                    self.boundaries.append(dict(kind="causal", b=b, h=h, rows=[r], key_in=r, key_out=r + 1 if r + 1 < s.Skv else None))
            elif s.Skv % 32 != 0:
                Q[b, :s.Sq] = (Q[b, :s.Sq] + u).to(self.dtype).float()
                K[b, s.Skv - 1], V[b, s.Skv - 1] = 2 * u, 4.0
                self.boundaries.append(dict(kind="Skv", b=b, h=None, rows=None, key_in=s.Skv - 1, key_out=None))
            else:
                self.exempt.append((b, f"no mask boundary: no causal mask, kv_len = Skv = {s.Skv} on a 32-key tile edge"))

    def _sensitivity(self, q64, k64, v64, vis):
        """min over the planted boundaries, both directions and the rows that see them of max_d |ref moved - ref|, relative to max |ref|.  The key behind
        Skv is a NaN row (any read of it fails the finiteness check), and a row left without a key has no defined output: neither direction is evaluated."""
        s, worst = self.shape, float("inf")
        ref = self.ref.view(s.B, s.Sq, s.H, s.D).transpose(1, 2)
        for bd in self.boundaries:
            b = bd["b"]
            hs = slice(None) if bd["h"] is None else slice(bd["h"], bd["h"] + 1)
            for key, on in ((bd["key_in"], False), (bd["key_out"], True)):
                if key is None:
                    continue
                rows = torch.arange(s.Sq) if bd["rows"] is None else torch.tensor(bd["rows"])
                v2 = vis[b].clone()
                if bd["kind"] == "causal":
                    v2[rows, key] = on
                else:   # the length moves for every row; the causal mask stays
                    v2[:, key] = vis[b][:, key - 1] if on else False
                    if on and s.causal:
                        v2[:, key] &= torch.arange(s.Sq) >= key
                rows = rows[(v2[rows] != vis[b][rows]).any(-1) & v2[rows].any(-1)]
                if rows.numel() == 0:
                    continue
                moved = attn_ref(q64[b:b + 1, hs][:, :, rows], k64[b:b + 1, hs], v64[b:b + 1, hs], self.scale, v2[rows][None])
                d = (moved - ref[b:b + 1, hs][:, :, rows]).abs().amax(-1)
                worst = min(worst, float(d.min()) / self.ref_max)
                bd.setdefault("moved", []).append((key, on, int(rows.numel()), float(d.min())))
            if "moved" not in bd:
                self.exempt.append((b, f"{bd['kind']} boundary at key {bd['key_in']}: the only key of its rows, and the key behind it is the NaN row"))
        return worst

    def on(self, device):
        if device not in self._dev:
            self._dev[device] = ([t.to(device) for t in self.host], None if self.kv_len is None else self.kv_len.to(device))
        return self._dev[device]


@functools.lru_cache(maxsize=None)
def inputs(shape, dtype, planted=False):
    return Inputs(shape, dtype, planted)


def has_boundary(shape):
    """does the planted set of this shape plant anything? (else the case declares itself boundary-free and runs the random set alone)"""
    if shape.causal or shape.Skv % 32 != 0:
        return True
    return shape.kv_len is not None and any(L < shape.Skv for L in shape.kv_len)


# ---- the names stllm_last_kernel() must report, restated from dispatch<T>() / launch_dma / launch_dma_nt of st-llm_amd/csrc/attention.hip -----------------------
DMA_CONFIGS = {24: (4, 2), 121: (1, 12), 42: (2, 4), 34: (4, 3)}   # attn_dma = 10 x tiles + waves -> (key-split waves per query tile, query tiles per workgroup)


def dma_name(dtype, ks2, tiles_req, Sq, q_lds_opt):
    """attn_dma_kernel<T, KS2, 128, NT> nw q_lds merge_par at head_dim 128: nw is clipped to the query tiles; 512 threads' worth of waves run the 512-thread
    instantiation unless attn_q_lds = 0; the query image needs nw x 8 KiB behind the 128 KiB of windows within 160 KiB; the parallel merge needs
    (KS2 - 1) x nw states of 66 x 256 bytes within the launch's LDS"""
    nw = min(tiles_req, (Sq + 31) // 32)
    nt = 512 if 64 * nw * ks2 <= 512 and q_lds_opt else 768
    q_lds = int(bool(q_lds_opt) and 131072 + nw * 8192 <= 163840)
    lds = 131072 + (nw * 8192 if q_lds else 0)
    merge_par = int(ks2 > 1 and bool(q_lds_opt) and (ks2 - 1) * nw * 66 * 256 <= lds)
    return f"attn_dma_kernel<{TNAME[dtype]},{ks2},128,{nt}> nw={nw} q_lds={q_lds} merge_par={merge_par}"


# ---- run and compare -----------------------------------------------------------------------------------------------------------------------------------------------
def last_kernel(hip):
    return hip.lib().stllm_last_kernel().decode()


def launch(hip, inp, device):
    """one stllm_attention call on inp's buffers; returns the guarded output"""
    s = inp.shape
    HD = s.H * s.D
    bufs, kl = inp.on(device)
    if inp.fused:
        ML, C = s.Skv + PAD_ROWS, 3 * HD
        f = bufs[0].view(s.B * ML, C)
        q, k, v = f[:, :HD], f[:, HD:2 * HD], f[:, 2 * HD:]
        st = dict(q_strides=(ML * C, C), k_strides=(ML * C, C), v_strides=(ML * C, C))
    else:
        q = bufs[0].view(s.B * (s.Sq + PAD_ROWS), HD)
        f = bufs[1].view(s.B * (s.Skv + PAD_ROWS), 2 * HD)
        k, v = f[:, :HD], f[:, HD:]
        st = dict(q_strides=((s.Sq + PAD_ROWS) * HD, HD), k_strides=((s.Skv + PAD_ROWS) * 2 * HD, 2 * HD), v_strides=((s.Skv + PAD_ROWS) * 2 * HD, 2 * HD))
    g = _poison.Guarded(s.B * s.Sq, HD, inp.dtype, device=device)
    saved = hip._decode_attn
    hip._decode_attn = False   # Sq = 1 is stllm_attention's here, not the decode entry's
    try:
        hip.attention(q, k, v, B=s.B, H=s.H, Sq=s.Sq, Skv=s.Skv, D=s.D, scale=inp.scale, causal=s.causal, kv_len=kl, out=g.out, **st)
    finally:
        hip._decode_attn = saved
    return g


def run_case(hip, shape, dtype, opts, want_name, device="cuda", tol=None, planted=True, random=True):
    """the dispatch options `opts`, then per input set (random; planted where the shape has a mask boundary): launch; 1. the kernel's name, 2. the guards,
    3. finiteness, 4. |got - ref| <= tol x max |ref|.  Options are restored whatever happens.  random / planted = False leaves that set out.  Returns the sets it ran."""
    tol = tol_of(dtype) if tol is None else tol
    ran = []
    try:
        for key, val in opts.items():
            hip.set_option(key, val)
        for pl in ([False] if random else []) + ([True] if planted and has_boundary(shape) else []):
            inp = inputs(shape, dtype, pl)
            if pl:
                assert inp.sensitivity >= 4 * tol, (shape.id, "planted boundary too weak for this tolerance", inp.sensitivity, tol)
            what = f"attention {shape.id} {dtype} {opts} {'planted' if pl else 'random'}"
            g = launch(hip, inp, device)
            name = last_kernel(hip)
            got = g.out.detach().cpu().double()
            err = float((got - inp.ref).abs().nan_to_num(float("inf")).max())
            print(f"{what}: [{name}] err {err:.3e} / abs-max {inp.ref_max:.3e} (bound {tol * inp.ref_max:.3e})")
            assert name == want_name, (what, name, want_name)
            assert g.intact(), (what, "a byte outside the B * Sq x H D output was written")
            assert bool(torch.isfinite(got).all()), (what, "non-finite output")
            assert err <= tol * inp.ref_max, (what, err, tol * inp.ref_max)
            ran.append(inp)
    finally:
        for key in opts:
            hip.set_option(key, DEFAULTS[key])
    return ran


# ---- the tables ----------------------------------------------------------------------------------------------------------------------------------------------------
def _with_kv(B, H, Sq, Skv, D, causal, ks):
    return [Shape(B, H, Sq, Skv, D, causal)] + [Shape(B, H, Sq, Skv, D, causal, (Skv, k)) for k in ks if k < Skv]


# A. head_dim 128, 16-bit, forced configuration: S = 96 leaves a KS2 = 4 partner without a key tile, 70 / 160 make a workgroup's last query wave dead at
# nw = 2, 3, 4, 257 comes back to window buffer 0; kv_len on and next to tile and window edges
A_SHAPES = [s for S in (1, 32, 33, 70, 96, 128, 129, 160, 257, 300) for s in _with_kv(2, 2, S, S, 128, True, (1, 32, 33, 128, 129) if S >= 129 else ())]
A_SHAPES += [s for sq, skv in ((40, 129), (129, 40), (33, 257)) for s in _with_kv(2, 2, sq, skv, 128, False, (33,))]

# C. head_dim 88: dma88 / resident (no causal mask, Skv <= 288, Sq > 32) on the 96-key window edges; the temporal kernel; the fall-through
C_WINDOW = [s for sq, skv in ((33, 33), (96, 96), (97, 97), (193, 192), (257, 257), (288, 288)) for s in _with_kv(2, 2, sq, skv, 88, False, (1, 96, 97))]
C_TEMPORAL = [Shape(2, 2, sq, skv, 88, False) for sq, skv in ((1, 1), (16, 16), (32, 32), (32, 257), (8, 300))]
C_FALL = [Shape(2, 2, 40, 289, 88, False), Shape(2, 2, 33, 33, 88, True), Shape(2, 2, 100, 100, 88, True)]

# D. head_dim 64: one wave up to 32 query rows, two above
D_SHAPES = [s for sq, skv in ((1, 1), (32, 31), (32, 33), (33, 32), (44, 44), (65, 257)) for s in _with_kv(2, 2, sq, skv, 64, False, (1, 32))]


def planted_shapes():
    """every shape of A, C and D that has a mask boundary: the planted sets the device file runs"""
    return [s for s in A_SHAPES + C_WINDOW + C_TEMPORAL + C_FALL + D_SHAPES if has_boundary(s)]
