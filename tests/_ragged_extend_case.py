"""TEST-ONLY: the two contracts of the ragged extend — stllm_attention_offset_ragged and stllm_kv_append_spans (include/stllm_hip.h) — stated once for the
contract backend (tests/_cpu_backend.py; installed() below layers them on top of it), the kernel case that the emulated and the device test share, and
the helpers of the model-level comparisons."""
import contextlib

import torch

import _cpu_backend as CB


# ---- the contracts ---------------------------------------------------------------------------------------------------------------------------------
def attention_offset_ragged(q, k, v, q_off, kv_len, *, B, H, Sq, max_kv, D, scale, out=None, q_strides=None, k_strides=None, v_strides=None):
    """fp64 softmax over every row's LIVE keys: batch row b holds q_off[b] cached positions and n_b = kv_len[b] - q_off[b] new ones (clamped as the header
    says); query row i < n_b sees the keys j <= q_off[b] + i, rows i >= n_b are zeros.  Keys at or behind kv_len[b] are never touched."""
    assert q_off.dtype == torch.int32 and kv_len.dtype == torch.int32 and q_off.numel() == B and kv_len.numel() == B
    qs = q_strides if q_strides is not None else (Sq * q.stride(0), q.stride(0))
    ks = k_strides if k_strides is not None else (max_kv * k.stride(0), k.stride(0))
    vs = v_strides if v_strides is not None else (max_kv * v.stride(0), v.stride(0))

    def rows(t, b, n, st):   # the first n rows of batch entry b: [n, H, D]
        return torch.as_strided(t, (n, H, D), (st[1], D, 1), t.storage_offset() + b * st[0]).double()
    o = torch.zeros((B * Sq, H * D), dtype=torch.float64)
    for b in range(B):
        L = max(min(int(kv_len[b]), max_kv), 0)
        P = max(min(int(q_off[b]), L), 0)
        n = min(L - P, Sq)
        if n <= 0:
            continue
        qb = rows(q, b, n, qs)
        kb, vb = rows(k, b, P + n, ks).transpose(0, 1), rows(v, b, P + n, vs).transpose(0, 1)   # [H, P + n, D]
        for i in range(n):
            s = (qb[i].unsqueeze(1) @ kb[:, :P + i + 1].transpose(-1, -2)) * scale
            o[b * Sq + i] = (s.softmax(-1) @ vb[:, :P + i + 1]).reshape(H * D)
    o = o.to(q.dtype)
    if out is not None:
        out.copy_(o)
        return out
    return o


def kv_append_spans(src, cache, pos0, n, *, S):
    """cache[b, pos0[b] + i, [k | v]] = src[b * S + i, [k | v]] for i < min(n[b], S) and 0 <= pos0[b] + i < max_len; nothing else is written"""
    B, max_len, D3 = cache.shape
    assert src.shape == (B * S, D3) and src.dtype == cache.dtype and pos0.dtype == torch.int32 and n.dtype == torch.int32
    c0 = D3 // 3
    for b, (p, m) in enumerate(zip(pos0.tolist(), n.tolist())):
        for i in range(min(m, S)):
            if 0 <= p + i < max_len:
                cache[b, p + i, c0:] = src[b * S + i, c0:]
    return cache


CONTRACTS = {"attention_offset_ragged": attention_offset_ragged, "kv_append_spans": kv_append_spans}


@contextlib.contextmanager
def installed():
    """the contract backend plus the two contracts above (and the answer that they are there: hip.ragged_extend_available)"""
    with CB.installed(), CB._patched(dict(CONTRACTS, ragged_extend_available=lambda device: True)):
        yield


@contextlib.contextmanager
def counting():
    """CB.counting() that also records the two new entry points (inside installed())"""
    from stllm_amd import hip

    def wrap(name, f):
        def g(*a, **k):
            CB.CALLS.append(name)
            return f(*a, **k)
        return g
    with CB.counting() as calls, CB._patched({n: wrap(n, getattr(hip, n)) for n in CONTRACTS}):
        yield calls


# ---- the kernel case -------------------------------------------------------------------------------------------------------------------------------
OUT_TOL = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -10}   # tests/test_prefix_cache_gpu.py: attention vs fp64 of the same 16-bit inputs is 2 x this x abs-max
Q_OFF, N_NEW = [0, 33, 200, 170], [40, 7, 40, 0]
# row 0: an empty cache (admission); row 1: keys end inside a 32-key tile, pad query rows; row 2: a long row with several key ranges; row 3: untouched


def rnd(*shape, seed=0, dtype=torch.float32, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def tol_of(dtype):
    return 2e-5 if dtype == torch.float32 else 2 * OUT_TOL[dtype]


class KernelCase:
    """B = 4, H = 2, D = 128, Sq = 40 (two query tiles, the second with 8 live rows at most), max_kv = 240 inside a cache of 256 rows per batch entry.
    q lives in a dense [B * Sq, 3 H D] scratch, K / V in the cache's own rows; every cache row at or behind kv_len[b] — and all of the n_b = 0 row — is NaN,
    and so are the pad rows of the scratch.  A late dominating key sits at position 230 of the long row: it is 6 x the q of query row (2, 35), which sits at position 235 and sees it, and
    carries more than 0.9 of that row's fp64 softmax (asserted here) — the running max jumps late in the key walk and the merge has to rescale."""

    def __init__(self, dtype, q_off=Q_OFF, n_new=N_NEW, Sq=40, H=2, ML=256, poison=True):
        self.dtype, self.B, self.H, self.D, self.Sq, self.ML = dtype, len(q_off), H, 128, Sq, ML
        B, HD = self.B, H * 128
        self.HD = HD
        self.q_off_h, self.n_h = list(q_off), list(n_new)
        self.kv_h = [p + n for p, n in zip(q_off, n_new)]
        self.max_kv = max(self.kv_h)
        self.cache = rnd(B, ML, 3 * HD, seed=500 + B, dtype=dtype, scale=0.6)
        self.dense = rnd(B * Sq, 3 * HD, seed=501, dtype=dtype, scale=0.6)
        self.dominated = None
        if B > 2 and self.q_off_h[2] + 35 >= 230 and self.n_h[2] > 35:
            # head 0 of query row (2, 35) — position q_off[2] + 35 >= 230, so it sees key 230 — finds that key dominating (asserted below, in fp64)
            self.cache[2, 230, HD:HD + 128] = (self.dense[2 * Sq + 35, :128].float() * 6).to(dtype)
            self.dominated = (2, 35, 230)
        if poison:
            for b in range(B):
                self.cache[b, self.kv_h[b]:] = float("nan")
                if self.n_h[b] == 0:
                    self.cache[b] = float("nan")
                self.dense[b * Sq + self.n_h[b]:(b + 1) * Sq] = float("nan")
        self.q_off = torch.tensor(self.q_off_h, dtype=torch.int32)
        self.kv_len = torch.tensor(self.kv_h, dtype=torch.int32)
        self.before = self.cache.clone()
        d64, c64 = self.dense.double(), self.flat(self.cache).double()   # fp64 of the same inputs, same strides
        self.want = attention_offset_ragged(d64[:, :HD], c64[:, HD:2 * HD], c64[:, 2 * HD:], self.q_off, self.kv_len, B=B, H=H, Sq=Sq, max_kv=self.max_kv, D=128, scale=128 ** -0.5,
                                            q_strides=(Sq * 3 * HD, 3 * HD), k_strides=(ML * 3 * HD, 3 * HD), v_strides=(ML * 3 * HD, 3 * HD))
        if self.dominated is not None:   # the fixture's own precondition: the planted key carries the row's softmax, so running max and merge rescale
            b, i, j = self.dominated
            vis = self.q_off_h[b] + i + 1
            w = ((self.cache[b, :vis, HD:HD + 128].double() @ d64[b * Sq + i, :128]) * 128 ** -0.5).softmax(0)
            self.dominating_weight = float(w[j])
            assert j < vis and self.dominating_weight > 0.9, (j, vis, self.dominating_weight)

    def flat(self, cache):
        return cache.view(self.B * self.ML, 3 * self.HD)

    def to(self, device):
        for n in ("cache", "dense", "q_off", "kv_len", "before"):
            setattr(self, n, getattr(self, n).to(device))
        return self

    def run(self, hip, out=None):
        HD, f = self.HD, self.flat(self.cache)
        st = (self.ML * 3 * HD, 3 * HD)
        return hip.attention_offset_ragged(self.dense[:, :HD], f[:, HD:2 * HD], f[:, 2 * HD:], self.q_off, self.kv_len, B=self.B, H=self.H, Sq=self.Sq,
                                           max_kv=self.max_kv, D=128, scale=128 ** -0.5, out=out, q_strides=(self.Sq * 3 * HD, 3 * HD), k_strides=st, v_strides=st)

    def check(self, got, what=""):
        """live rows against fp64, pad rows exactly zero (and not NaN); prints the figure before it asserts"""
        got = got.detach().cpu()
        scale = float(self.want.abs().max())
        live = torch.zeros(self.B * self.Sq, dtype=torch.bool)
        for b, n in enumerate(self.n_h):
            live[b * self.Sq: b * self.Sq + n] = True
        err = float((got[live].double() - self.want[live]).abs().max())
        print(f"attention_offset_ragged {self.dtype} {what}: err {err:.3e} / abs-max {scale:.3e} (bound {tol_of(self.dtype) * scale:.3e})")
        assert not torch.isnan(got.float()).any(), what
        assert bool((got[~live].float() == 0).all()), (what, "pad rows are exact zeros")
        assert err <= tol_of(self.dtype) * scale, (what, err, scale)


def append_case(dtype):
    """stllm_kv_append_spans: B = 4, S = 5, hidden = 136 (a partial last workgroup), batch stride > max_len x row stride, a span that would cross max_len"""
    B, S, ML, hidden = 4, 5, 7, 136
    cache = rnd(B, ML + 1, 3 * hidden, seed=510, dtype=dtype)[:, :ML]
    src = rnd(B * S, 3 * hidden, seed=511, dtype=dtype)
    pos0, n = [0, 5, 3, 5], [5, 2, 0, 3]          # row 3: positions 5, 6, 7 — the last one is max_len: not written
    want = cache.clone()
    for b in range(B):
        for i in range(min(n[b], S)):
            if 0 <= pos0[b] + i < ML:
                want[b, pos0[b] + i, hidden:] = src[b * S + i, hidden:]
    return cache, src, torch.tensor(pos0, dtype=torch.int32), torch.tensor(n, dtype=torch.int32), S, want


# ---- model level -----------------------------------------------------------------------------------------------------------------------------------
SMALL = dict(num_hidden_layers=2, hidden_size=256, intermediate_size=704, num_attention_heads=2, vocab_size=512)
MODEL_TOL = {"fp32": 2e-4, "bf16": 5e-2, "fp16": 5e-2}   # x the reference's abs-max (test_extend_matches_prefill_and_per_token_loop)


# ids / seeds of the id-equality cases: drawn at random and kept where, on the CPU contract backend in fp32, the from-scratch margin of every generated step
# is >= 1.8e-2 (the tests assert >= 1e-2 x max |score| themselves, on the CPU and on the device's own reference run)
CHAT_QUESTIONS = [[29174, 13784, 1329], [28526, 2066, 6263, 30051, 18599], [26327]]
CHAT_TURNS = [[8487, 31639, 16756, 15925], [7267], [31707, 4672]]
WIDE_PREFIXES, WIDE_QUESTIONS, WIDE_SEEDS = [40, 17, 33], [9, 3, 5], [5, 0, 3]   # full width (4096), two layers, lm_head x 6: T("rex.gvideo{b}.{seed}") / T("rex.gq{b}.{seed}")
MARGIN = 1e-2


def ragged_prefix(lm, emb, prefixes, max_len, device):
    """a cache of len(prefixes) rows, row b prefilled with emb[b, :prefixes[b]] (one right-padded prefill: KVCache.lens = prefixes)"""
    B, Pm = len(prefixes), max(prefixes)
    c = lm.new_cache(B, max_len, device)
    mask = (torch.arange(Pm)[None, :] < torch.tensor(prefixes)[:, None]).long()
    lm.prefill(emb[:, :Pm].clone() * mask[..., None].to(emb.device), mask, cache=c)
    return c


def margins(logit_rows):
    """(top-1 - top-2) / max|logit| of every generated step's logits row"""
    out = []
    for lg in logit_rows:
        top = lg.double().topk(2).values
        out.append(float((top[0] - top[1]) / lg.double().abs().max()))
    return out


@contextlib.contextmanager
def scored_runs():
    """records, for every token selected inside the context, (top-1 - top-2) / max |finite score| of the processed scores the selection saw
    (generation._process_logits: greedy search, one row per call or more)"""
    from stllm_amd import generation
    seen, orig = [], generation._process_logits

    def spy(scores, *a, **k):
        out = orig(scores, *a, **k)
        for row in out.double():
            top = row.topk(2).values
            seen.append(float((top[0] - top[1]) / row[torch.isfinite(row)].abs().max()))
        return out
    generation._process_logits = spy
    try:
        yield seen
    finally:
        generation._process_logits = orig
