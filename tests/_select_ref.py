"""TEST-ONLY: the contracts of stllm_select_tokens / stllm_beam_candidates (include/stllm_hip.h) stated once, on the CPU, with the signatures of
hip.select_tokens / hip.beam_candidates — so that `_cpu_backend._patched({"select_tokens": select_tokens, "beam_candidates": beam_candidates})` runs
generate(selection="device") without a GPU, and the kernel tests compare against `row_stats` / `beam_scores64`.

What is exact and what is fp64: the repetition penalty and the temperature are single IEEE fp32 operations in the contract, so they are done in fp32 here
too (bit-equal to the kernel and to generation._process_logits); everything behind them — exp, sums, masses, CDFs, log-softmax — is fp64.
No torch.sort / torch.topk / Tensor.log_softmax / torch.multinomial: one test runs device mode with those patched to raise."""
import torch


def processed(logits, prev=None, n_prev=0, penalty=1.0, suppress_eos=False, eos_id=None):
    """steps 1 and 2 of the contract on a copy of `logits` [rows, V] (its own dtype: fp32 for token selection, fp64 log-probabilities for beams)"""
    s = logits.detach().clone()
    V = s.shape[1]
    if penalty != 1.0 and n_prev > 0:
        ids = prev[:, :n_prev].long()
        ok = (ids >= 0) & (ids < V)
        idc = ids.clamp(0, V - 1)
        g = torch.gather(s, 1, idc)
        g2 = torch.where(g < 0, g * penalty, g / penalty)          # from the ORIGINAL score: a repeated id scatters the same value again
        assert bool(ok.all()), "the reference takes ids inside [0, V) only (the kernels skip the others)"
        s.scatter_(1, idc, g2)
    if suppress_eos and eos_id is not None and 0 <= eos_id < V:
        s[:, eos_id] = -float("inf")
    return s


class RowStats:
    """fp64 view of one sampling step: s (fp32 scores after penalty / EOS / temperature), e = exp(s - max), Z, mass[i] = sum_{e_j <= e_i} e_j / Z,
    kept (the contract's rule), amax"""

    def __init__(self, s32, top_p):
        self.s = s32
        s = s32.double()
        self.max = s.max(dim=1).values
        self.amax = s32.argmax(dim=1)                              # lowest index of the maximum (checked in test_select_cpu against a tie)
        for r in range(s.shape[0]):
            self.amax[r] = int((s32[r] == s32[r].max()).nonzero()[0])
        self.e = torch.exp(s - self.max[:, None])
        self.Z = self.e.sum(dim=1)
        order = torch.argsort(self.e, dim=1, stable=True)
        se = torch.gather(self.e, 1, order)
        cum = se.cumsum(dim=1)
        pos = torch.searchsorted(se, self.e.contiguous(), right=True) - 1      # the last sorted entry <= e_i: ties take the whole group's mass
        self.mass = torch.gather(cum, 1, pos) / self.Z[:, None]
        if top_p >= 1.0:
            self.kept = self.e > 0
        else:
            self.kept = self.mass > (1.0 - top_p)
        self.kept[torch.arange(s.shape[0]), self.amax] = True
        self.ek = torch.where(self.kept, self.e, torch.zeros_like(self.e))
        self.Zk = self.ek.sum(dim=1)
        self.cdf = self.ek.cumsum(dim=1)                           # inclusive prefix over the kept ids, in id order


def row_stats(logits, *, prev=None, n_prev=0, penalty=1.0, suppress_eos=False, eos_id=None, temperature=1.0, top_p=1.0):
    s = processed(logits.float(), prev, n_prev, penalty, suppress_eos, eos_id)
    if temperature != 1.0:
        s = s / temperature
    return RowStats(s, top_p)


def select_tokens(logits, out, *, prev=None, n_prev=0, penalty=1.0, suppress_eos=False, eos_id=None, pad_id=0, sample=False, temperature=1.0, top_p=1.0,
                  u=None, unfinished=None, aux=None):
    rows = logits.shape[0]
    if not sample:
        s = processed(logits.float(), prev, n_prev, penalty, suppress_eos, eos_id)
        tok = torch.stack([(s[r] == s[r].max()).nonzero()[0, 0] for r in range(rows)])
        mx = s.max(dim=1).values
        ax = torch.stack([mx.double(), torch.logsumexp(s.double() - mx.double()[:, None], dim=1), torch.zeros(rows, dtype=torch.float64),
                          torch.ones(rows, dtype=torch.float64)], dim=1)
    else:
        st = row_stats(logits, prev=prev, n_prev=n_prev, penalty=penalty, suppress_eos=suppress_eos, eos_id=eos_id, temperature=temperature, top_p=top_p)
        target = u.double() * st.Zk
        hit = st.kept & (st.cdf > target[:, None])
        tok = torch.empty(rows, dtype=torch.long)
        for r in range(rows):
            nz = hit[r].nonzero()
            tok[r] = int(nz[0]) if nz.numel() else int(st.kept[r].nonzero()[-1])
        thr = torch.where(st.kept, st.e, torch.full_like(st.e, float("inf"))).min(dim=1).values
        ax = torch.stack([st.max, st.Z.log(), thr, st.Zk / st.Z], dim=1)
    live = torch.ones(rows, dtype=torch.bool) if unfinished is None else unfinished != 0
    res = torch.where(live, tok, torch.full_like(tok, pad_id))
    out.copy_(res.to(out.dtype))
    if unfinished is not None and eos_id is not None:
        unfinished.mul_((~(live & (tok == eos_id))).to(unfinished.dtype))
    if aux is not None:
        aux[live] = ax.float()[live]
    return out


def beam_scores64(logits, beam_score, *, prev=None, n_prev=0, penalty=1.0, suppress_eos=False, eos_id=None):
    """fp64 candidate scores [rows, V]: log_softmax, then the penalty and the EOS suppression ON the log-probabilities, plus the beam's running score"""
    s = logits.double()
    lp = s - s.max(dim=1, keepdim=True).values
    lp = lp - torch.logsumexp(lp, dim=1, keepdim=True)
    return processed(lp, prev, n_prev, penalty, suppress_eos, eos_id) + beam_score.double()[:, None]


def beam_candidates(logits, beam_score, k, *, prev=None, n_prev=0, penalty=1.0, suppress_eos=False, eos_id=None, cand_score=None, cand_token=None):
    sc = beam_scores64(logits, beam_score, prev=prev, n_prev=n_prev, penalty=penalty, suppress_eos=suppress_eos, eos_id=eos_id).float()
    order = torch.argsort(-sc, dim=1, stable=True)[:, :k]          # fp32 scores descending; stable: token ascending inside a tie
    cs, ct = torch.gather(sc, 1, order), order.to(torch.int32)
    if cand_score is None:
        return cs, ct
    cand_score.copy_(cs)
    cand_token.copy_(ct)
    return cand_score, cand_token


# ---- kernel cases, shared by tests/test_select_cpu.py (host-emulated kernels) and tests/test_select_gpu.py (the device) -------------------------------------
# Bands (derived, not tuned): a row sum is at most ~130 ordered fp32 adds (125 per thread, then the butterfly) of terms carrying a 2-ulp exp: < 1e-5 relative;
# every band below is 2x that.  An e-value compared with the kernel's threshold carries the rounding of exp's argument s - max (half an ulp of |ln e|) and the
# 2 ulp of exp itself: relative (2 + |ln e|) * 2^-24, again doubled.
BAND = 2e-5
U_SPECIAL = [0.0, 0.5, 1.0 - 2.0 ** -24]


def u_values(n_seeded=64, seed=1234):
    g = torch.Generator().manual_seed(seed)
    return torch.cat([torch.tensor(U_SPECIAL, dtype=torch.float32), torch.rand(n_seeded, generator=g)])


def padded_logits(x):
    """x [rows, V] as a view of rows padded to a multiple of 128, the padding filled with NaN and +inf: columns >= V must not matter"""
    rows, V = x.shape
    ldl = (V + 127) // 128 * 128
    buf = torch.full((rows, ldl), float("nan"), dtype=torch.float32)
    buf[:, V + 1::2] = float("inf")
    buf[:, :V] = x
    return buf[:, :V]


def on_device(view, dev):
    """the padded rows behind a padded_logits view moved to `dev`, the same view of them (a plain .to() of the view would drop the padding)"""
    if dev == "cpu":
        return view
    base = view._base if view._base is not None else view
    return base.to(dev)[:, :view.shape[1]]


def make_case(rows, V, *, scale=1.0, n_prev=0, seed=0, max_at=None, tie=False):
    """(logits view [rows, V] fp32 in padded rows, prev int32 [rows, max(n_prev, 1)]).  n_prev = 300 holds duplicates and, in every row, that row's best and
    worst token (a positive and a negative penalised score).  max_at: the row maximum is planted there.  tie: rows get an exact tie of the maximum at two ids."""
    g = torch.Generator().manual_seed(1000 * seed + V)
    x = torch.randn(rows, V, generator=g) * scale
    if max_at is not None:
        x[:, max_at] = x.max(dim=1).values + 1.0
    if tie and V >= 2:
        i, j = V // 3, V - 1
        top = x.max(dim=1).values + 0.5
        x[:, i], x[:, j] = top, top
    prev = torch.randint(0, V, (rows, max(n_prev, 1)), generator=g).to(torch.int32)
    if n_prev >= 4:
        prev[:, n_prev // 2:n_prev] = prev[:, :n_prev - n_prev // 2]            # duplicates
        prev[:, 0], prev[:, 1] = x.argmax(dim=1).to(torch.int32), x.argmin(dim=1).to(torch.int32)
    elif n_prev == 1:
        prev[:, 0] = x.argmax(dim=1).to(torch.int32)
    return padded_logits(x), prev


def check_greedy(hip, dev, logits, prev, *, n_prev=0, penalty=1.0, suppress_eos=False, eos_id=None, pad_id=0, finished=(), min_gap=1e-3):
    """greedy: the token equals the reference exactly (top-2 gap of the reference >= min_gap, or an exact tie: lowest index)"""
    rows, V = logits.shape
    for _ in range(4):   # choose the input: a row whose REFERENCE top-2 gap is under min_gap (and not an exact tie) gets its winner raised by 1, in place
        s = processed(logits.float(), prev, n_prev, penalty, suppress_eos, eos_id)
        want = torch.stack([(s[r] == s[r].max()).nonzero()[0, 0] for r in range(rows)])
        if V == 1 or not min_gap:
            break
        top2 = torch.stack([s[r][torch.argsort(-s[r], stable=True)[:2]] for r in range(rows)])
        gap = top2[:, 0] - top2[:, 1]
        small = (gap < min_gap) & (gap != 0)
        if not bool(small.any()):
            break
        logits[small, want[small]] += 1.0
    else:
        raise AssertionError(f"test input: reference top-2 gap {gap.min().item():.2e} < {min_gap}")
    unf = torch.ones(rows, dtype=torch.int32)
    for r in finished:
        unf[r] = 0
    unf_d, out = unf.to(dev), torch.full((rows, 3), -7, dtype=torch.int32, device=dev)
    aux = torch.full((rows, 4), -5.0, device=dev)
    hip.select_tokens(on_device(logits, dev), out[:, 1], prev=prev.to(dev), n_prev=n_prev, penalty=penalty, suppress_eos=suppress_eos, eos_id=eos_id,
                      pad_id=pad_id, unfinished=unf_d, aux=aux)
    out, unf_d, aux = out.cpu(), unf_d.cpu(), aux.cpu()
    assert bool((out[:, 0] == -7).all()) and bool((out[:, 2] == -7).all()), "the output stride was not respected"
    for r in range(rows):
        if r in finished:
            assert int(out[r, 1]) == pad_id and int(unf_d[r]) == 0 and float(aux[r, 0]) == -5.0
            continue
        assert int(out[r, 1]) == int(want[r]), (r, int(out[r, 1]), int(want[r]))
        assert int(unf_d[r]) == (0 if eos_id is not None and int(want[r]) == eos_id else 1)
        assert float(aux[r, 0]) == float(s[r].max())
        lse = float(torch.logsumexp(s[r].double() - s[r].double().max(), dim=0))
        assert abs(float(aux[r, 1]) - lse) <= BAND, (r, float(aux[r, 1]), lse)
    return out[:, 1]


def check_sample(hip, dev, logits, prev, u, *, n_prev=0, penalty=1.0, suppress_eos=False, eos_id=None, temperature=1.0, top_p=1.0, verbose=False):
    """one sampled launch, u f32 [rows]: the kept set through aux's threshold, the token and its CDF interval — for every row, no exclusions"""
    rows, V = logits.shape
    st = row_stats(logits, prev=prev, n_prev=n_prev, penalty=penalty, suppress_eos=suppress_eos, eos_id=eos_id, temperature=temperature, top_p=top_p)
    out = torch.empty(rows, dtype=torch.int32, device=dev)
    aux = torch.empty((rows, 4), device=dev)
    hip.select_tokens(on_device(logits, dev), out, prev=prev.to(dev), n_prev=n_prev, penalty=penalty, suppress_eos=suppress_eos, eos_id=eos_id,
                      sample=True, temperature=temperature, top_p=top_p, u=u.to(dev), aux=aux)
    out, aux = out.cpu().long(), aux.cpu().double()
    cut = 1.0 - top_p if top_p < 1.0 else 0.0
    for r in range(rows):
        thr = float(aux[r, 2])
        tol = (2.0 + abs(torch.log(aux[r, 2].clamp_min(1e-300)).item())) * 2.0 ** -23
        above, below = st.mass[r] > cut + BAND, st.mass[r] < cut - BAND
        in_band = ~above & ~below
        if verbose:
            print(f"row {r}: kept {int(st.kept[r].sum())} band {int(in_band.sum())} thr {thr:.6e} Zk/Z {float(aux[r, 3]):.7f} ref {float(st.Zk[r] / st.Z[r]):.7f}")
        assert float(aux[r, 0]) == float(st.s[r].max())
        assert abs(float(aux[r, 1]) - float(st.Z[r].log())) <= BAND
        assert bool((st.e[r][above] >= thr * (1 - tol)).all()), (r, "a token above the band lies under the threshold")
        assert bool((st.e[r][below] < thr * (1 + tol)).all()) or bool(below[st.amax[r]]), (r, "a token below the band lies at or above the threshold")
        if bool(below.any()) and not bool((st.e[r][below] < thr * (1 + tol)).all()):      # only the argmax may be kept from below the band
            bad = below & (st.e[r] >= thr * (1 + tol))
            assert int(bad.sum()) == 1 and bool(bad[st.amax[r]])
        lo_mass = float(st.e[r][above | (torch.arange(V) == st.amax[r])].sum() / st.Z[r])
        hi_mass = float(st.e[r][~below | (torch.arange(V) == st.amax[r])].sum() / st.Z[r])
        assert lo_mass - BAND <= float(aux[r, 3]) <= hi_mass + BAND, (r, lo_mass, float(aux[r, 3]), hi_mass)
        tok = int(out[r])
        assert 0 <= tok < V and (not bool(below[tok]) or tok == int(st.amax[r])), (r, tok, "the sampled token is neither kept nor in the band")
        target, w = float(u[r].double() * st.Zk[r]), BAND * float(st.Zk[r])
        hi = float(st.cdf[r, tok])
        lo = hi - float(st.ek[r, tok])
        if verbose:
            print(f"        u {float(u[r]):.8f} tok {tok} interval [{lo:.8e}, {hi:.8e}] target {target:.8e}")
        assert lo - w <= target <= hi + w, (r, tok, lo, target, hi, w)
    return out


def check_beam(hip, dev, logits, prev, beam_score, k, *, n_prev=0, penalty=1.0, suppress_eos=False, eos_id=None):
    rows, V = logits.shape
    ref = beam_scores64(logits, beam_score, prev=prev, n_prev=n_prev, penalty=penalty, suppress_eos=suppress_eos, eos_id=eos_id)
    cs, ct = hip.beam_candidates(on_device(logits, dev), beam_score.to(dev), k, prev=prev.to(dev), n_prev=n_prev, penalty=penalty,
                                 suppress_eos=suppress_eos, eos_id=eos_id)
    cs, ct = cs.cpu(), ct.cpu().long()
    for r in range(rows):
        assert bool(((ct[r] >= 0) & (ct[r] < V)).all()) and len(set(ct[r].tolist())) == k, (r, "token range / duplicates")
        if float(beam_score[r]) <= -1e8:
            continue   # every score of such a row is the same fp32 number: range and duplicates only
        for j in range(k):
            want = float(ref[r, ct[r, j]])
            got = float(cs[r, j])
            assert got == want or abs(got - want) <= BAND + 2.0 ** -23 * abs(want), (r, j, got, want)
            if j:
                assert (got < float(cs[r, j - 1])) or (got == float(cs[r, j - 1]) and int(ct[r, j]) > int(ct[r, j - 1])), (r, j, "order")
        kth = float(ref[r][torch.argsort(-ref[r], stable=True)[k - 1]])
        assert bool((ref[r, ct[r]] >= kth - 2 * BAND).all()), (r, "a returned token is not among the k best")
    return cs, ct
