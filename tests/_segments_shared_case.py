"""TEST-ONLY: the contract of the packed segment step on a shared base — stllm_attention_segments_shared (include/stllm_hip.h) — stated once in
fp64 for the contract backend (installed() layers it over tests/_segments_case.py), the kernel case and the bit-contract case that the emulated and the device
tests share, and the helpers of the model- and engine-level comparisons."""
import contextlib

import torch

import _cpu_backend as CB
import _ragged_extend_case as RC
import _segments_case as SC


# ---- the contract ----------------------------------------------------------------------------------------------------------------------------------
def attention_segments_shared(q, kp, vp, ks, vs, slot, row0, sfx_off, sfx_len, *, H, D, T, P, n_slots, max_n, max_sfx, scale, out=None, kp_strides=None,
                              ks_strides=None):
    """fp64 softmax over the P prefix keys (ONE base row, only read) and every segment's LIVE suffix keys: segment r reads slot row slot[r], holds sfx_off[r]
    suffix positions and n_r = sfx_len[r] - sfx_off[r] new ones (clamped as the header says); its query row i < n_r is packed row row0[r] + i and sees all
    P prefix keys and the suffix keys j <= sfx_off[r] + i.  A segment whose tables point outside the buffers does nothing.  Only the segments' packed rows of
    `out` are written; base rows at or behind P and suffix rows at or behind sfx_len[r] are never read."""
    R = slot.numel()
    slot, row0, sfx_off, sfx_len = SC._tables((slot, row0, sfx_off, sfx_len), R)
    assert P > 0 and max_sfx > 0 and max_n > 0
    kps = kp_strides if kp_strides is not None else (P * kp.stride(0), kp.stride(0))
    kss = ks_strides if ks_strides is not None else (max_sfx * ks.stride(0), ks.stride(0))

    def rows(t, base, n, rs):   # n rows of H x D from element offset `base`: [n, H, D]
        return torch.as_strided(t, (n, H, D), (rs, D, 1), t.storage_offset() + base).double()
    if out is None:
        out = torch.zeros((T, H * D), dtype=q.dtype)
    kpre, vpre = rows(kp, 0, P, kps[1]), rows(vp, 0, P, kps[1])
    for r in range(R):
        L = max(min(sfx_len[r], max_sfx), 0)
        off = max(min(sfx_off[r], L), 0)
        n = min(L - off, max_n)
        if n <= 0 or not 0 <= slot[r] < n_slots or row0[r] < 0 or row0[r] + n > T:
            continue
        qb = rows(q, row0[r] * q.stride(0), n, q.stride(0))
        kb, vb = rows(ks, slot[r] * kss[0], off + n, kss[1]), rows(vs, slot[r] * kss[0], off + n, kss[1])
        for i in range(n):
            k = torch.cat([kpre, kb[:off + i + 1]]).transpose(0, 1)   # [H, P + off + i + 1, D]
            v = torch.cat([vpre, vb[:off + i + 1]]).transpose(0, 1)
            s = (qb[i].unsqueeze(1) @ k.transpose(-1, -2)) * scale
            out[row0[r] + i, :H * D] = (s.softmax(-1) @ v).reshape(H * D).to(out.dtype)
    return out


CONTRACTS = {"attention_segments_shared": attention_segments_shared}


@contextlib.contextmanager
def installed():
    """SC.installed() plus the contract above (and the answer that it is there: hip.segments_shared_available)"""
    with SC.installed(), CB._patched(dict(CONTRACTS, segments_shared_available=lambda device: True)):
        yield


@contextlib.contextmanager
def counting():
    """SC.counting() that also records the new entry point (inside installed())"""
    from stllm_amd import hip

    def wrap(name, f):
        def g(*a, **k):
            CB.CALLS.append(name)
            return f(*a, **k)
        return g
    with SC.counting() as calls, CB._patched({n: wrap(n, getattr(hip, n)) for n in CONTRACTS}):
        yield calls


# ---- the kernel case -------------------------------------------------------------------------------------------------------------------------------
rnd, tol_of, GUARD = RC.rnd, RC.tol_of, SC.GUARD
SEGMENTS = [(4, 0, 40), (0, 33, 1), (2, 20, 40), (5, 0, 1), (1, 31, 7)]   # (slot, sfx_off, n) in packed order
# an admission into an empty suffix (two query tiles); one token whose keys end just inside a second tile; a suffix of 60 keys (two key tiles); a one-token
# prompt; a block that crosses the 32-key edge.  Slot 3 is named by no segment.
PLANT_PREFIX = (2, 35, 0, 150)    # (segment index, query row, head, base position): the key is 6 x that row's q
PLANT_SUFFIX = (0, 30, 1, 10)     # (segment index, query row, head, local position in that segment's slot)


class SharedSegmentCase:
    """H = 2, D = 128.  Base: one row, P = 200 (ksplit_plan(1, 2, 89, 200): 3 key ranges, the last tile holds 8 live keys) in a buffer of 208 rows whose 8
    behind P are NaN.  Slots: 6 x 64 local rows, every row at or behind its segment's sfx_len — and all of slot 3 — NaN.  R = 5 segments, T = 89 packed rows
    (three query tiles, the last one partial) in a [T + 8, 3 H D] scratch whose last 8 rows are NaN.  Two planted keys make the merge rescale in both
    directions: one in the PREFIX that carries a row of the slot-2 segment, one in a SUFFIX that carries a row of the slot-4 segment (asserted here, fp64)."""

    def __init__(self, dtype, segments=SEGMENTS, n_slots=6, H=2, P=200, PB=208, ML=64, poison=True, plant=True):
        self.dtype, self.H, self.D, self.P, self.PB, self.ML, self.n_slots = dtype, H, 128, P, PB, ML, n_slots
        HD = self.HD = H * 128
        self.slot_h, self.off_h, self.n_h = [s for s, _, _ in segments], [p for _, p, _ in segments], [n for _, _, n in segments]
        self.R, self.max_n, self.T = len(segments), max(self.n_h), sum(self.n_h)
        self.row0_h = [sum(self.n_h[:r]) for r in range(self.R)]
        self.len_h = [p + n for p, n in zip(self.off_h, self.n_h)]
        self.max_sfx = max(self.len_h)
        self.base = rnd(PB, 3 * HD, seed=540, dtype=dtype, scale=0.6)
        self.cache = rnd(n_slots, ML, 3 * HD, seed=541, dtype=dtype, scale=0.6)
        self.dense = rnd(self.T + GUARD, 3 * HD, seed=542, dtype=dtype, scale=0.6)
        if plant:
            r, i, h, j = PLANT_PREFIX
            self.base[j, HD + h * 128:HD + (h + 1) * 128] = (self.dense[self.row0_h[r] + i, h * 128:(h + 1) * 128].float() * 6).to(dtype)
            r, i, h, j = PLANT_SUFFIX
            self.cache[self.slot_h[r], j, HD + h * 128:HD + (h + 1) * 128] = (self.dense[self.row0_h[r] + i, h * 128:(h + 1) * 128].float() * 6).to(dtype)
        if poison:
            self.dense[self.T:] = float("nan")
            self.base[P:] = float("nan")
            named = dict(zip(self.slot_h, self.len_h))
            for s in range(n_slots):
                self.cache[s, named.get(s, 0):] = float("nan")
        i32 = lambda x: torch.tensor(x, dtype=torch.int32)
        self.slot, self.row0, self.sfx_off, self.sfx_len = i32(self.slot_h), i32(self.row0_h), i32(self.off_h), i32(self.len_h)
        self.before = (self.base.clone(), self.cache.clone())
        self.want = self.call(attention_segments_shared, self.dense.double(), self.base.double(), self.cache.double())
        assert not torch.isnan(self.want).any()
        self.planted_weights = []
        if plant:   # the fixture's own precondition: each planted key carries its row's softmax
            d64, b64, c64 = self.dense.double(), self.base.double(), self.cache.double()
            for (r, i, h, j), in_prefix in ((PLANT_PREFIX, True), (PLANT_SUFFIX, False)):
                vis = self.off_h[r] + i + 1
                keys = torch.cat([b64[:P, HD + h * 128:HD + (h + 1) * 128], c64[self.slot_h[r], :vis, HD + h * 128:HD + (h + 1) * 128]])
                w = ((keys @ d64[self.row0_h[r] + i, h * 128:(h + 1) * 128]) * 128 ** -0.5).softmax(0)
                assert in_prefix or j < vis
                self.planted_weights.append(float(w[j if in_prefix else P + j]))
            assert min(self.planted_weights) > 0.9, self.planted_weights

    def flat(self, cache):
        return cache.view(self.n_slots * self.ML, 3 * self.HD)

    def to(self, device):
        for n in ("base", "cache", "dense", "slot", "row0", "sfx_off", "sfx_len"):
            setattr(self, n, getattr(self, n).to(device))
        return self

    def out_buffer(self):
        """[T + 8, H D]: a fixed finite pattern everywhere — the kernel overwrites the T packed rows and must leave the 8 behind them as they are"""
        rows = self.T + GUARD
        pat = ((torch.arange(rows * self.HD) % 251).float() / 16 - 7).view(rows, self.HD).to(self.dtype)
        return pat.to(self.dense.device)

    def call(self, f, dense, base, cache, out=None, **over):
        HD, c = self.HD, cache.view(self.n_slots * self.ML, 3 * self.HD)
        k = dict(H=self.H, D=128, T=self.T, P=self.P, n_slots=self.n_slots, max_n=self.max_n, max_sfx=self.max_sfx, scale=128 ** -0.5, out=out,
                 kp_strides=(self.PB * 3 * HD, 3 * HD), ks_strides=(self.ML * 3 * HD, 3 * HD))
        k.update(over)
        return f(dense[:, :HD], base[:, HD:2 * HD], base[:, 2 * HD:], c[:, HD:2 * HD], c[:, 2 * HD:], self.slot, self.row0, self.sfx_off, self.sfx_len, **k)

    def run(self, hip, out=None, **over):
        return self.call(hip.attention_segments_shared, self.dense, self.base, self.cache, out=out, **over)

    def unchanged(self):
        from _poison import bits_equal
        return bits_equal(self.base.cpu(), self.before[0]) and bits_equal(self.cache.cpu(), self.before[1])

    def check(self, got, what=""):
        """every packed row against fp64, no NaN, the sentinel rows behind T as they were; prints the figure before it asserts"""
        from _poison import bits_equal
        got = got.detach().cpu()
        scale = float(self.want.abs().max())
        err = float((got[:self.T].double() - self.want).abs().max())
        print(f"attention_segments_shared {self.dtype} {what}: err {err:.3e} / abs-max {scale:.3e} (bound {tol_of(self.dtype) * scale:.3e})")
        assert not torch.isnan(got.float()).any(), what
        assert got.shape[0] == self.T + GUARD and bits_equal(got[self.T:], self.out_buffer().cpu()[self.T:]), (what, "the rows behind T are not written")
        assert err <= tol_of(self.dtype) * scale, (what, err, scale)


BIT_SEGMENTS = [(0, 20, 9), (1, 20, 9), (2, 20, 9)]   # the bit contract: 3 segments of n = 9 behind sfx_off = 20, slots 0 .. 2 in slot order


def bit_contract(hip, dtype, device="cpu"):
    """(the new entry's output, stllm_attention_shared(B = 3, G = 1, Sq = 9, causal, sfx_q_off = 20)'s on the same buffers): equal bit for bit by contract"""
    case = SharedSegmentCase(dtype, segments=BIT_SEGMENTS, n_slots=3, plant=False).to(device)
    HD, c = case.HD, case.flat(case.cache)
    got = case.run(hip)
    want = hip.attention_shared(case.dense[:, :HD], case.base[:, HD:2 * HD], case.base[:, 2 * HD:], c[:, HD:2 * HD], c[:, 2 * HD:], B=3, G=1, H=case.H, Sq=9,
                                P=case.P, D=128, scale=128 ** -0.5, max_sfx=29, sfx_len=case.sfx_len, sfx_q_off=20, causal=True,
                                q_strides=(9 * 3 * HD, 3 * HD), kp_strides=(case.PB * 3 * HD, 3 * HD), ks_strides=(case.ML * 3 * HD, 3 * HD))
    assert case.T == 27 and case.max_sfx == 29 and not torch.isnan(got[:27].float()).any()
    return got[:27], want[:27]


# ---- model level -------------------------------------------------------------------------------------------------------------------------------------
SMALL, MODEL_TOL, MARGIN = SC.SMALL, SC.MODEL_TOL, SC.MARGIN
scored_runs, alone, REQ_PROMPTS, REQ_MAX_NEW = SC.scored_runs, SC.alone, SC.REQ_PROMPTS, SC.REQ_MAX_NEW
VIDEO_LEN, SLOTS, MAX_NEW = 11, 4, 37
FIRST = [(0, 17), (2, 33), (3, 5)]     # the first call admits 17, 33 and 5 tokens into slots 0, 2 and 3
SECOND = [(0, 1), (1, 9), (2, 1)]      # the second appends 1, 9 and 1 to slots 0, 1 and 2; slot 1 was empty, slot 3 is not named


def two_calls(model, video, emb, device):
    """video f32 [11, D], emb f32 [4, >= 34, D] on `device`.  The video is prefilled into a one-row cache, share(rows=4, max_new=37) makes the slot cache, then
    TWO step_segments calls (FIRST, SECOND).  Returns (h1 f32 [3, D], h2 f32 [3, D], the slot cache, the base, the slot buffers between the calls, the
    base's buffers before the first call)."""
    lm = model.model
    base = lm.new_cache(1, VIDEO_LEN, device)
    lm.prefill(video[None], None, cache=base)
    base_before = [x.clone() for x in base.qkv]
    cache = base.share(rows=SLOTS, max_new=MAX_NEW)
    assert cache.row_lens() == [VIDEO_LEN] * SLOTS and cache.base is base and cache.qkv[0].shape[1] == MAX_NEW
    h1, _ = lm.step_segments(torch.cat([emb[s, :n] for s, n in FIRST]), cache, FIRST)
    held = [VIDEO_LEN + n for n in (17, 0, 33, 5)]
    assert cache.row_lens() == held
    between = [x.clone() for x in cache.qkv]
    h2, _ = lm.step_segments(torch.cat([emb[s, held[s] - VIDEO_LEN:held[s] - VIDEO_LEN + n] for s, n in SECOND]), cache, SECOND)
    assert cache.row_lens() == [VIDEO_LEN + n for n in (18, 9, 34, 5)]
    return h1, h2, cache, base, between, base_before


def from_scratch(model, video, emb, b, L, device):
    """[video, emb[b, :L]] prefilled alone: (the last token's final-norm hidden row f32 [D], its one-row cache)"""
    lm = model.model
    c = lm.new_cache(1, VIDEO_LEN + L, device)
    h32, _ = lm.prefill(torch.cat([video, emb[b, :L]])[None], None, cache=c)
    return h32[0, -1], c


def check_two_calls(model, video, emb, device, tol, what=""):
    """the comparisons of the model-level case: every row's last hidden state (of both calls) against a from-scratch prefill of [video, row], the suffix
    K / V rows against that cache's rows [P, P + L), slot 3 bit-unchanged by the second call, the base bit-unchanged"""
    from _poison import bits_equal
    h1, h2, cache, base, between, base_before = two_calls(model, video, emb, device)
    P, D = VIDEO_LEN, emb.shape[-1]
    assert bool(torch.isfinite(h1).all()) and bool(torch.isfinite(h2).all())
    assert all(bits_equal(x, y) for x, y in zip(base.qkv, base_before)) and base.len == P, "the base is only read"
    for x, y in zip(cache.qkv, between):
        assert bits_equal(x[3], y[3]), "the slot that the second call does not name is untouched"
    for h, segs, L_of in ((h1, FIRST, {0: 17, 2: 33, 3: 5}), (h2, SECOND, {0: 18, 1: 9, 2: 34})):
        for r, (b, _) in enumerate(segs):
            L = L_of[b]
            want, one = from_scratch(model, video, emb, b, L, device)
            err, scale = float((h[r] - want).abs().max()), float(want.abs().max())
            print(f"[{what}] step_segments on a base, slot {b} at {L} suffix positions: hidden err {err:.3e} (bound {tol:.0e} x {scale:.3f})")
            assert err <= tol * scale, (what, b, L, err, scale)
            if L == {0: 18, 1: 9, 2: 34, 3: 5}[b]:   # what the slot holds in the end
                for x, y in zip(cache.qkv, one.qkv):
                    kv, ref = x[b, :L, D:].float(), y[0, P:P + L, D:].float()
                    assert float((kv - ref).abs().max()) <= tol * float(ref.abs().max()), ("suffix rows", what, b)
    return cache


# ---- the engine case ---------------------------------------------------------------------------------------------------------------------------------
def serve(model, prompts, slots, max_len, base, submit_prefix=None, **k):
    """SC.REQ_PROMPTS' requests through serving.Engine(base=): (ids per request in submission order, the engine); idle slots sit at the base's length"""
    from stllm_amd import serving
    eng = serving.Engine(model, slots, max_len, base=base, **k)
    assert eng.cache.base is base and eng.cache.row_lens() == [base.len] * slots
    handles = [eng.submit(p, prefix=submit_prefix, max_new_tokens=n) for p, n in zip(prompts, REQ_MAX_NEW)]
    got = dict(eng.run())
    assert sorted(got) == sorted(handles) and eng.idle() and eng.cache.row_lens() == [base.len] * slots
    return [got[h] for h in handles], eng
