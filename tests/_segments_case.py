"""TEST-ONLY: the two contracts of the packed segment step — stllm_attention_segments and stllm_kv_append_segments (include/stllm_hip.h) — stated once for the
contract backend (installed() layers them over tests/_ragged_extend_case.py, which layers its own over tests/_cpu_backend.py), the kernel case and the
append case that the emulated and the device tests share, and the helpers of the model- and engine-level comparisons."""
import contextlib

import torch

import _cpu_backend as CB
import _ragged_extend_case as RC


# ---- the contracts ---------------------------------------------------------------------------------------------------------------------------------
def _tables(p, R):
    assert all(t.dtype == torch.int32 and t.numel() == R for t in p)
    return [t.tolist() for t in p]


def attention_segments(q, k, v, slot, row0, q_off, kv_len, *, H, D, T, n_slots, max_n, max_kv, scale, out=None, k_strides=None, v_strides=None):
    """fp64 softmax over every segment's LIVE keys: segment r reads cache row slot[r], holds q_off[r] cached positions and n_r = kv_len[r] - q_off[r] new
    ones (clamped as the header says); its query row i < n_r is packed row row0[r] + i and sees the keys j <= q_off[r] + i.  A segment whose tables point
    outside the buffers does nothing.  Only the segments' packed rows of `out` are written; nothing else of q, K or V is touched."""
    R = slot.numel()
    slot, row0, q_off, kv_len = _tables((slot, row0, q_off, kv_len), R)
    ks = k_strides if k_strides is not None else (max_kv * k.stride(0), k.stride(0))
    vs = v_strides if v_strides is not None else (max_kv * v.stride(0), v.stride(0))

    def rows(t, base, n, rs):   # n rows of H x D from element offset `base`: [n, H, D]
        return torch.as_strided(t, (n, H, D), (rs, D, 1), t.storage_offset() + base).double()
    if out is None:
        out = torch.zeros((T, H * D), dtype=q.dtype)
    for r in range(R):
        L = max(min(kv_len[r], max_kv), 0)
        P = max(min(q_off[r], L), 0)
        n = min(L - P, max_n)
        if n <= 0 or not 0 <= slot[r] < n_slots or row0[r] < 0 or row0[r] + n > T:
            continue
        qb = rows(q, row0[r] * q.stride(0), n, q.stride(0))
        kb = rows(k, slot[r] * ks[0], P + n, ks[1]).transpose(0, 1)   # [H, P + n, D]
        vb = rows(v, slot[r] * vs[0], P + n, vs[1]).transpose(0, 1)
        for i in range(n):
            s = (qb[i].unsqueeze(1) @ kb[:, :P + i + 1].transpose(-1, -2)) * scale
            out[row0[r] + i, :H * D] = (s.softmax(-1) @ vb[:, :P + i + 1]).reshape(H * D).to(out.dtype)
    return out


def kv_append_segments(src, cache, slot, row0, pos0, n, *, T, max_n):
    """cache[slot[r], pos0[r] + i, [k | v]] = src[row0[r] + i, [k | v]] for i < n[r] and 0 <= pos0[r] + i < max_len; a segment whose tables point outside
    the buffers, and everything else, is left alone"""
    n_slots, max_len, D3 = cache.shape
    R = slot.numel()
    assert src.shape[0] >= T and src.shape[1] == D3 and src.dtype == cache.dtype
    slot, row0, pos0, n = _tables((slot, row0, pos0, n), R)
    c0 = D3 // 3
    for r in range(R):
        assert n[r] <= max_n
        if not 0 <= slot[r] < n_slots or row0[r] < 0 or row0[r] + n[r] > T:
            continue
        for i in range(n[r]):
            if 0 <= pos0[r] + i < max_len:
                cache[slot[r], pos0[r] + i, c0:] = src[row0[r] + i, c0:]
    return cache


CONTRACTS = {"attention_segments": attention_segments, "kv_append_segments": kv_append_segments}


@contextlib.contextmanager
def installed():
    """the contract backend, the ragged-extend contracts and the two contracts above (and the answer that they are there: hip.segments_available)"""
    with RC.installed(), CB._patched(dict(CONTRACTS, segments_available=lambda device: True)):
        yield


@contextlib.contextmanager
def counting():
    """RC.counting() that also records the two new entry points (inside installed())"""
    from stllm_amd import hip

    def wrap(name, f):
        def g(*a, **k):
            CB.CALLS.append(name)
            return f(*a, **k)
        return g
    with RC.counting() as calls, CB._patched({n: wrap(n, getattr(hip, n)) for n in CONTRACTS}):
        yield calls


# ---- the kernel case -------------------------------------------------------------------------------------------------------------------------------
rnd, tol_of = RC.rnd, RC.tol_of
SEGMENTS = [(4, 0, 40), (0, 33, 1), (2, 200, 40), (5, 170, 1), (1, 63, 7)]   # (slot, q_off, n) in packed order
# an admission into an empty slot (two query tiles); a decode token whose keys end inside a 32-key tile; a long row with several key ranges and the planted
# dominating key; another decode token; a short block.  Slot 3 is named by no segment.
GUARD = 8        # sentinel rows behind T in the q scratch (NaN) and in the out buffer (a fixed pattern)


class SegmentCase:
    """H = 2, D = 128, a cache of 6 slots x 256 rows, max_kv = 240, max_n = 40, R = 5 segments, T = 89 packed rows.  q lives in a packed [T + 8, 3 H D] scratch
    whose last 8 rows are NaN, K / V in the cache's own rows; every cache row at or behind its segment's kv_len — and all of slot 3 — is NaN.  The planted key
    sits at position 230 of slot 2: it is 6 x the q (head 0) of that segment's query row 35, which sits at position 235, sees it and gives it more than 0.9 of
    its fp64 softmax (asserted here).  The one-token segments share the query-tile grid with the 40-row ones: their second tile, and lanes 1 .. 31 of their
    first, are rows of OTHER segments (or behind T) that the kernel must neither read nor write."""

    def __init__(self, dtype, segments=SEGMENTS, n_slots=6, H=2, ML=256, max_kv=240, poison=True):
        self.dtype, self.H, self.D, self.ML, self.n_slots, self.max_kv = dtype, H, 128, ML, n_slots, max_kv
        HD = self.HD = H * 128
        self.slot_h, self.q_off_h, self.n_h = [s for s, _, _ in segments], [p for _, p, _ in segments], [n for _, _, n in segments]
        self.R, self.max_n, self.T = len(segments), max(self.n_h), sum(self.n_h)
        self.row0_h = [sum(self.n_h[:r]) for r in range(self.R)]
        self.kv_h = [p + n for p, n in zip(self.q_off_h, self.n_h)]
        self.cache = rnd(n_slots, ML, 3 * HD, seed=520, dtype=dtype, scale=0.6)
        self.dense = rnd(self.T + GUARD, 3 * HD, seed=521, dtype=dtype, scale=0.6)
        self.dominated = None
        for r, (s, p, n) in enumerate(segments):
            if s == 2 and p + 35 >= 230 and n > 35:
                self.cache[2, 230, HD:HD + 128] = (self.dense[self.row0_h[r] + 35, :128].float() * 6).to(dtype)
                self.dominated = (r, 35, 230)
        if poison:
            self.dense[self.T:] = float("nan")
            named = dict(zip(self.slot_h, self.kv_h))
            for s in range(n_slots):
                self.cache[s, named.get(s, 0):] = float("nan")
        i32 = lambda x: torch.tensor(x, dtype=torch.int32)
        self.slot, self.row0, self.q_off, self.kv_len = i32(self.slot_h), i32(self.row0_h), i32(self.q_off_h), i32(self.kv_h)
        self.before = self.cache.clone()
        d64, c64 = self.dense.double(), self.flat(self.cache).double()   # fp64 of the same inputs, same strides
        st = (ML * 3 * HD, 3 * HD)
        self.want = attention_segments(d64[:, :HD], c64[:, HD:2 * HD], c64[:, 2 * HD:], self.slot, self.row0, self.q_off, self.kv_len, H=H, D=128, T=self.T,
                                       n_slots=n_slots, max_n=self.max_n, max_kv=max_kv, scale=128 ** -0.5, k_strides=st, v_strides=st)
        assert not torch.isnan(self.want).any()
        if self.dominated is not None:   # the fixture's own precondition: the planted key carries the row's softmax, so running max and merge rescale
            r, i, j = self.dominated
            vis = self.q_off_h[r] + i + 1
            w = ((self.cache[2, :vis, HD:HD + 128].double() @ d64[self.row0_h[r] + i, :128]) * 128 ** -0.5).softmax(0)
            self.dominating_weight = float(w[j])
            assert j < vis and self.dominating_weight > 0.9, (j, vis, self.dominating_weight)

    def flat(self, cache):
        return cache.view(self.n_slots * self.ML, 3 * self.HD)

    def to(self, device):
        for n in ("cache", "dense", "slot", "row0", "q_off", "kv_len", "before"):
            setattr(self, n, getattr(self, n).to(device))
        return self

    def out_buffer(self):
        """[T + 8, H D]: a fixed finite pattern everywhere — the kernel overwrites the T packed rows and must leave the 8 behind them as they are"""
        rows = self.T + GUARD
        pat = ((torch.arange(rows * self.HD) % 251).float() / 16 - 7).view(rows, self.HD).to(self.dtype)
        return pat.to(self.dense.device)

    def run(self, hip, out=None):
        HD, f = self.HD, self.flat(self.cache)
        st = (self.ML * 3 * HD, 3 * HD)
        return hip.attention_segments(self.dense[:, :HD], f[:, HD:2 * HD], f[:, 2 * HD:], self.slot, self.row0, self.q_off, self.kv_len, H=self.H, D=128,
                                      T=self.T, n_slots=self.n_slots, max_n=self.max_n, max_kv=self.max_kv, scale=128 ** -0.5, out=out, k_strides=st, v_strides=st)

    def check(self, got, what=""):
        """every packed row against fp64, no NaN, the sentinel rows behind T as they were; prints the figure before it asserts"""
        from _poison import bits_equal
        got = got.detach().cpu()
        scale = float(self.want.abs().max())
        err = float((got[:self.T].double() - self.want).abs().max())
        print(f"attention_segments {self.dtype} {what}: err {err:.3e} / abs-max {scale:.3e} (bound {tol_of(self.dtype) * scale:.3e})")
        assert not torch.isnan(got.float()).any(), what
        assert got.shape[0] == self.T + GUARD and bits_equal(got[self.T:], self.out_buffer().cpu()[self.T:]), (what, "the rows behind T are not written")
        assert err <= tol_of(self.dtype) * scale, (what, err, scale)


def append_case(dtype):
    """stllm_kv_append_segments: hidden = 136 (a partial last workgroup), 5 slots of 7 positions (cache row stride > max_len x row stride), T = 12 packed rows;
    slots out of order, a segment that would cross max_len, one with n = 0, one with a slot out of range, one whose rows would end behind T; slot 1 unnamed"""
    n_slots, ML, hidden, T = 5, 7, 136, 12
    cache = rnd(n_slots, ML + 1, 3 * hidden, seed=530, dtype=dtype)[:, :ML]
    src = rnd(T + 2, 3 * hidden, seed=531, dtype=dtype)
    #        slot  row0 pos0 n
    segs = [(3, 0, 0, 4), (0, 4, 5, 3), (2, 7, 3, 0), (7, 7, 0, 2), (4, 9, 2, 3), (-1, 0, 0, 1), (2, 11, 0, 2)]
    # (0, 4, 5, 3): positions 5, 6, 7 — the last one is max_len: not written; (7, ..) and (-1, ..): no such slot; (2, 11, 0, 2): rows 11, 12 end behind T
    want = cache.clone()
    for s, r0, p, n in segs:
        if not 0 <= s < n_slots or r0 + n > T:
            continue
        for i in range(n):
            if 0 <= p + i < ML:
                want[s, p + i, hidden:] = src[r0 + i, hidden:]
    tabs = [torch.tensor(c, dtype=torch.int32) for c in zip(*segs)]
    return cache, src, tabs, T, 4, want


# ---- model level -------------------------------------------------------------------------------------------------------------------------------------
SMALL, MODEL_TOL, MARGIN = RC.SMALL, RC.MODEL_TOL, RC.MARGIN
margins, scored_runs = RC.margins, RC.scored_runs

# one packed step over slots that hold 17, 0 and 33 positions: 1, 9 and 1 new tokens; a fourth slot (5 positions) is named by no segment
STEP_HAVE, STEP_NEW, STEP_IDLE = [17, 0, 33], [1, 9, 1], 5


def segment_step(model, emb, max_len, device):
    """emb f32 [4, >= 34, D] on `device`.  Slots 0 .. 2 are loaded through KVCache.load_row from one-row prefills of emb[b, :STEP_HAVE[b]] (slot 1 stays
    empty), slot 3 holds STEP_IDLE positions of emb[3]; then ONE step_segments call.  Returns (h32 [3, D], h16, cache, the slot buffers before the step)."""
    lm = model.model
    cache = lm.new_cache(4, max_len, device)
    cache.set_lens([0] * 4)
    for b, P in list(enumerate(STEP_HAVE)) + [(3, STEP_IDLE)]:
        if P:
            one = lm.new_cache(1, P, device)
            lm.prefill(emb[b:b + 1, :P], None, cache=one)
            before = [x.clone() for x in one.qkv]
            cache.load_row(b, one)
            assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(one.qkv, before)), "load_row only reads its source"
    assert cache.row_lens() == STEP_HAVE + [STEP_IDLE]
    before = [x.clone() for x in cache.qkv]
    packed = torch.cat([emb[b, P:P + n] for b, (P, n) in enumerate(zip(STEP_HAVE, STEP_NEW))])
    h32, h16 = lm.step_segments(packed, cache, [(b, n) for b, n in enumerate(STEP_NEW)])
    assert cache.row_lens() == [P + n for P, n in zip(STEP_HAVE, STEP_NEW)] + [STEP_IDLE]
    return h32, h16, cache, before


def from_scratch(model, emb, b, device):
    """row b's full sequence prefilled alone: (the last token's final-norm hidden row f32 [D], its one-row cache)"""
    lm = model.model
    L = STEP_HAVE[b] + STEP_NEW[b]
    c = lm.new_cache(1, L, device)
    h32, _ = lm.prefill(emb[b:b + 1, :L], None, cache=c)
    return h32[0, -1], c


# ---- the engine case: 5 requests of different prompt lengths and max_new_tokens over 2 slots ----------------------------------------------------------
REQ_PROMPTS, REQ_MAX_NEW = [5, 9, 3, 7, 4], [6, 3, 8, 4, 5]


def alone(model, prompts, video=None, **k):
    """generate() of every request alone, from scratch ([video,] prompt prefilled in one call): the ids the Engine has to give"""
    out = []
    for p, n in zip(prompts, REQ_MAX_NEW):
        whole = p if video is None else torch.cat([video, p])
        out.append(model.generate(inputs_embeds=whole[None], max_new_tokens=n, **k)[0])
    return out


def serve(model, prompts, slots, max_len, prefix=None, **k):
    """the same requests through serving.Engine: (ids per request in submission order, the engine)"""
    from stllm_amd import serving
    eng = serving.Engine(model, slots, max_len, **k)
    handles = [eng.submit(p, prefix=prefix, max_new_tokens=n) for p, n in zip(prompts, REQ_MAX_NEW)]
    got = dict(eng.run())
    assert sorted(got) == sorted(handles) and eng.idle() and eng.cache.row_lens() == [0] * slots
    return [got[h] for h in handles], eng
