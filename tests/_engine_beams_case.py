"""TEST-ONLY: continuous batching for beam search.  The contracts of stllm_kv_reorder_rows and stllm_beam_candidates_rows
(include/stllm_hip.h) stated once for the contract backend (installed() layers them over tests/_segments_shared_case.py and the selection contracts of
tests/_select_ref.py), the kernel cases that the emulated and the device tests share, and the helpers of the engine-level comparisons: the requests, their
vetted seeds, and the guard that keeps an id comparison from hiding a failure behind a near-tie.

The engine case runs with an EOS that has a probability of a few tenths at every step (eos_probability: a test-local wrapper of `logits_from`; a
synth-filled model gives its EOS id the probability of any other token, and num_beams hypotheses never collect).  Hypotheses then finish mid-way and
`is_done` ends at least one request BEFORE its budget while another runs to its limit — asserted, for the from-scratch runs and for the Engine in both
states —, so the `done` path of _BeamRequest.process, the finalize() that adds no open beams and the early release of a group with the re-admission into it
are all compared with generate().  The cases with penalties and with a stop sequence keep the plain model and the SEEDS table."""
import contextlib

import torch

import _cpu_backend as CB
import _poison
import _segments_case as SC
import _segments_shared_case as SSC
import _select_ref as R


# ---- the contracts ---------------------------------------------------------------------------------------------------------------------------------
def kv_reorder_rows(cache, src, lo, hi, *, nb, max_span):
    """old = cache.clone(); cache[r, p, [k | v]] = old[src[r], p, [k | v]] for every group g of nb rows, every row r of it whose src[r] differs from r and
    lies inside the group, and every p in [max(lo[g], 0), min(hi[g], capacity)); everything else is left alone"""
    rows, cap, D3 = cache.shape
    D = D3 // 3
    assert 1 <= nb <= 16 and rows % nb == 0 and src.dtype == lo.dtype == hi.dtype == torch.int32
    assert src.numel() == rows and lo.numel() == hi.numel() == rows // nb and max_span > 0
    old = cache.clone()
    for g in range(rows // nb):
        p0, p1 = max(int(lo[g]), 0), min(int(hi[g]), cap)
        assert p1 - p0 <= max_span, "max_span bounds hi - lo"
        for r in range(g * nb, (g + 1) * nb):
            s = int(src[r])
            if p1 > p0 and s != r and g * nb <= s < (g + 1) * nb:
                cache[r, p0:p1, D:] = old[s, p0:p1, D:]
    return cache


def beam_candidates_rows(logits, src, beam_score, k, *, prev=None, n_prev, penalty=1.0, min_length=0, eos_id=None, cand_score=None, cand_token=None,
                         one=None):
    """stllm_beam_candidates, row by row: candidate row r reads logits row src[r] behind prev[r, :n_prev[r]]; an unserved row is untouched.
    one: the one-row launch to build on (default: the fp64 contract `_select_ref.beam_candidates`; the kernel tests pass hip.beam_candidates)"""
    one = one or R.beam_candidates
    rows = src.numel()
    if cand_score is None:
        cand_score, cand_token = torch.empty((rows, k), dtype=torch.float32), torch.empty((rows, k), dtype=torch.int32)
    for r in range(rows):
        s = int(src[r])
        if not 0 <= s < logits.shape[0]:
            continue
        n = int(n_prev[r])
        c = min(max(n, 0), 0 if prev is None else prev.shape[1])
        cs, ct = one(logits[s:s + 1], beam_score[r:r + 1], k, prev=prev[r:r + 1] if c else None, n_prev=c, penalty=penalty,
                     suppress_eos=eos_id is not None and n < min_length, eos_id=eos_id)
        cand_score[r], cand_token[r] = cs[0], ct[0]
    return cand_score, cand_token


CONTRACTS = {"kv_reorder_rows": kv_reorder_rows, "beam_candidates_rows": beam_candidates_rows}


@contextlib.contextmanager
def installed():
    """SSC.installed(), the selection contracts of generate(selection="device"), the two contracts above (and the answer that they are there)"""
    with SSC.installed(), CB._patched(dict(CONTRACTS, beam_candidates=R.beam_candidates, select_tokens=R.select_tokens, beam_rows_available=lambda device: True)):
        yield


@contextlib.contextmanager
def counting():
    """SSC.counting() that also records the two new entry points (inside installed())"""
    from stllm_amd import hip

    def wrap(name, f):
        def g(*a, **k):
            CB.CALLS.append(name)
            return f(*a, **k)
        return g
    with SSC.counting() as calls, CB._patched({n: wrap(n, getattr(hip, n)) for n in CONTRACTS}):
        yield calls


# ---- the re-order kernel case ------------------------------------------------------------------------------------------------------------------------
HIDDEN, CAPACITY = 256, 40
# (nb, src, lo, hi).  hidden = 256: a position is 64 cells of 16 bytes in bf16 / fp16 and 128 in fp32, a workgroup of 256 threads covers 4 / 2 positions
REORDER_CASES = {
    # a 3-cycle over 17 positions (a multiple of neither 4 nor 2); a full fan-out with lo below 0 and hi beyond the capacity; an identity group
    "cycle, fan-out, identity": (3, [1, 2, 0, 3, 3, 3, 6, 7, 8], [3, -2, 0], [20, 45, 40]),
    # a mix over ONE position; a permutation whose group has hi <= lo (and one with hi < lo would be the same branch); row 6 names another group's row,
    # row 7 a row outside [0, rows) — both ignored — and row 8 takes row 6
    "one position, empty range, bad entries": (3, [0, 0, 1, 4, 3, 5, 0, 99, 6], [7, 10, 5], [8, 10, 9]),
    "hi < lo": (3, [1, 2, 0, 5, 3, 4, 7, 8, 6], [9, 30, 39], [3, 31, 40]),
    # nb = 5: a fan-out from row 0 (the admission's re-order), and a 2-cycle next to a 3-cycle across the last positions
    "five beams": (5, [0, 0, 0, 0, 0, 6, 5, 8, 9, 7], [0, 32], [33, 39]),
    # nb = 16: the largest group; a mapping with a long cycle, fan-outs and fixed points
    "sixteen beams": (16, [5, 0, 2, 2, 9, 15, 6, 6, 1, 4, 10, 3, 3, 3, 7, 8], [1], [38]),
}


def reorder_buffers(dtype, rows, seed):
    """(raw, cache): raw [rows, CAPACITY + 1, 3 * HIDDEN] filled with the poison pattern of tests/_poison.py (0xFF bytes), then its first CAPACITY
    positions — the view `cache`, whose row stride is larger than CAPACITY positions — overwritten with random BYTES (any bit pattern: the kernel moves
    bytes); the position behind the capacity stays poison"""
    es = torch.empty(0, dtype=dtype).element_size()
    raw = torch.full((rows, CAPACITY + 1, 3 * HIDDEN * es), 0xFF, dtype=torch.uint8)
    g = torch.Generator().manual_seed(9100 + seed)
    raw[:, :CAPACITY] = torch.randint(0, 256, (rows, CAPACITY, 3 * HIDDEN * es), generator=g, dtype=torch.uint8)
    raw = raw.view(dtype)
    return raw, raw[:, :CAPACITY]


def reorder_want(cache, nb, src, lo, hi):
    """the torch restatement of the issue: old = buf.clone(); buf[r, p, D:] = old[src[r], p, D:] — and the mask of what the contract allows to change"""
    rows, cap, D3 = cache.shape
    D = D3 // 3
    want, old = cache.clone(), cache.clone()
    written = torch.zeros((rows, cap, D3), dtype=torch.bool)
    for g in range(rows // nb):
        p0, p1 = max(lo[g], 0), min(hi[g], cap)
        for r in range(g * nb, (g + 1) * nb):
            if p1 > p0 and src[r] != r and g * nb <= src[r] < (g + 1) * nb:
                want[r, p0:p1, D:] = old[src[r], p0:p1, D:]
                written[r, p0:p1, D:] = True
    return want, written


def check_reorder(hip, dev, dtype, name):
    """one case on `dev`: the whole allocation bit for bit against the restatement — the q columns, the other positions, the untouched rows and the poison
    behind the capacity keep their bits —, and the same call on the same bytes again"""
    nb, src, lo, hi = REORDER_CASES[name]
    rows = len(src)
    raw, cache = reorder_buffers(dtype, rows, seed=len(name))
    want, written = reorder_want(cache, nb, src, lo, hi)
    span = max(1, max(min(h, CAPACITY) - max(l, 0) for l, h in zip(lo, hi)))
    i32 = lambda x: torch.tensor(x, dtype=torch.int32).to(dev)
    got = []
    for _ in range(2):
        d_raw = raw.clone().to(dev)
        hip.kv_reorder_rows(d_raw[:, :CAPACITY], i32(src), i32(lo), i32(hi), nb=nb, max_span=span)
        got.append(d_raw.cpu())
    assert _poison.bits_equal(got[0][:, :CAPACITY], want), (name, dtype, "the re-ordered rows")
    assert _poison.bits_equal(got[0][:, CAPACITY:], raw[:, CAPACITY:]), (name, dtype, "the position behind the capacity keeps its poison")
    keep = ~written
    assert _poison.bits_equal(got[0][:, :CAPACITY][keep], cache[keep]), (name, dtype, "outside the written region nothing changes")
    assert _poison.bits_equal(got[0], got[1]), (name, dtype, "the same call twice gives the same bytes")
    return int(written.sum())


def check_reorder_unsupported(hip, dev, dtype=torch.bfloat16):
    """nb = 17: STLLM_ERR_UNSUPPORTED, and nothing is written"""
    import pytest
    raw, cache = reorder_buffers(dtype, 17, seed=17)
    d_raw = raw.clone().to(dev)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32).to(dev)
    with pytest.raises(RuntimeError, match=r"\(-4\).*nb=17"):
        hip.kv_reorder_rows(d_raw[:, :CAPACITY], i32([1] * 17), i32([0]), i32([CAPACITY]), nb=17, max_span=CAPACITY)
    assert _poison.bits_equal(d_raw.cpu(), raw)


# ---- the candidates kernel case ------------------------------------------------------------------------------------------------------------------------
LD_PREV, MIN_LENGTH = 12, 2
CAND_N_PREV = [0, 1, 7, LD_PREV, 7, 1]      # per candidate row: rows 0, 1 and 5 are under MIN_LENGTH and suppress the EOS, rows 2 and 3 do not
CAND_SRC = [2, 0, 0, 3, -1, 9]              # rows 1 and 2 name ONE logits row; row 4 and row 5 (an entry >= n_logits_rows = 4) are not served


def check_candidates(hip, dev, V, k, penalty):
    """6 candidate rows over 4 logits rows: every served row bit-identical to a stllm_beam_candidates launch of that row alone with that row's n_prev and
    suppression; the unserved rows keep their poison; ids behind n_prev (out of range: a read would be skipped, so the last one is IN range and would
    visibly move a score) are never read"""
    logits, _ = R.make_case(4, V, scale=4.0, seed=31 + k)
    eos = V // 2
    logits[:, eos] = logits.max(dim=1).values + 1.0            # the EOS would be every row's best candidate: suppression shows
    g = torch.Generator().manual_seed(77 * V + k)
    prev = torch.full((6, LD_PREV), 2 ** 30, dtype=torch.int32)
    for r, n in enumerate(CAND_N_PREV):
        prev[r, :n] = torch.randint(0, V, (n,), generator=g).to(torch.int32)
        if n >= 4:
            prev[r, n // 2:n] = prev[r, :n - n // 2].clone()   # duplicates
        if n:
            prev[r, 0] = int(logits[max(CAND_SRC[r], 0) % 4].argsort(descending=True)[1])   # the runner-up is in the history: the penalty moves the order
        if n < LD_PREV:
            prev[r, LD_PREV - 1] = int(logits[max(CAND_SRC[r], 0) % 4].argsort(descending=True)[2])   # in range, behind n_prev: never read
    prev[prev == eos] = eos + 1                                # (the EOS itself is not in a history: a penalty must not move it)
    beam_score = torch.tensor([0.0, -1e9, -0.5, -3.25, 0.0, -1.0])   # row 1: a beam of the admission step, every score of it one fp32 number
    src, n_prev = torch.tensor(CAND_SRC, dtype=torch.int32), torch.tensor(CAND_N_PREV, dtype=torch.int32)
    poison_s, poison_t = torch.full((6, k), float("nan")), torch.full((6, k), -1, dtype=torch.int32)
    poison_s.view(torch.int32).fill_(-1)
    lg = R.on_device(logits, dev)
    cs, ct = poison_s.clone().to(dev), poison_t.clone().to(dev)
    hip.beam_candidates_rows(lg, src.to(dev), beam_score.to(dev), k, prev=prev.to(dev), n_prev=n_prev.to(dev), penalty=penalty, min_length=MIN_LENGTH,
                             eos_id=eos, cand_score=cs, cand_token=ct)
    cs, ct = cs.cpu(), ct.cpu()

    want_s, want_t = poison_s.clone(), poison_t.clone()
    for r, (s, n) in enumerate(zip(CAND_SRC, CAND_N_PREV)):
        if 0 <= s < 4:
            a, b = hip.beam_candidates(lg[s:s + 1], beam_score[r:r + 1].to(dev), k, prev=prev[r:r + 1].to(dev) if n else None, n_prev=n, penalty=penalty,
                                       suppress_eos=n < MIN_LENGTH, eos_id=eos)
            want_s[r], want_t[r] = a.cpu()[0], b.cpu()[0]
    assert _poison.bits_equal(cs, want_s) and _poison.bits_equal(ct, want_t), (V, k, penalty, cs.tolist(), want_s.tolist())
    for r in (0, 1):
        assert eos not in ct[r].tolist(), (r, "the EOS is suppressed under min_length")
    assert int(ct[3, 0]) == eos and int(ct[2, 0]) == eos, "... and is the best candidate of the rows at or behind it"
    return cs, ct


# ---- the engine case -----------------------------------------------------------------------------------------------------------------------------------
REQ_PROMPTS, REQ_MAX_NEW = SC.REQ_PROMPTS, [6, 3, 8, 4, 5]
VIDEO_LEN = 11
# prompt seeds T("beams.req{i}.{seed}") / T("beams.video.{seed}"), searched on the CPU contract backend (fp32) so that the from-scratch runs satisfy the guard
# below with room to spare: SMALL is the 256-wide model of the CPU suites, WIDE the full-width two-layer model of the device suites
# SEEDS[which][(nb, with_video)] = (the five seeds, the EOS id that some request's beams emit mid-way)
SEEDS = {"small": {(3, False): ([0, 2, 1, 0, 0], 30), (3, True): ([0, 0, 23, 0, 0], 336), (5, False): ([5, 1, 1, 39, 1], 210), (5, True): ([0, 0, 58, 0, 0], 336)},
         "wide": {(3, False): ([7, 0, 4, 0, 2], 8408), (3, True): ([0, 0, 1, 0, 4], 29603), (5, False): ([23, 4, 4, 1, 14], 23642), (5, True): ([25, 1, 31, 0, 9], 14642)}}


# EARLY[which][(nb, with_video)] = (the five seeds, the EOS id, its probability at every step — eos_probability below): searched in the same way, so that
# in the from-scratch runs `is_done` ends at least one request before its budget (request 2 with its budget of 8, or request 0), another runs to its limit,
# and the guard holds with room to spare
EARLY = {"small": {(3, False): ([30, 4, 39, 26, 31], 30, 0.4), (3, True): ([21, 28, 23, 17, 12], 336, 0.4),
                   (5, False): ([30, 18, 21, 16, 20], 210, 0.4), (5, True): ([15, 30, 5, 16, 37], 336, 0.4)},
         "wide": {(3, False): ([7, 22, 14, 9, 16], 8408, 0.4), (3, True): ([12, 15, 0, 23, 3], 29603, 0.4),
                  (5, False): ([7, 0, 11, 1, 5], 23642, 0.8), (5, True): ([6, 6, 71, 5, 6], 14642, 0.65)}}


def requests(which, nb, D, device="cpu", with_video=False, seeds=None):
    from _util import T
    seeds = SEEDS[which][(nb, with_video)][0] if seeds is None else seeds
    return [T(f"beams.req{i}.{s}", (n, D), 0.05).to(device) for i, (n, s) in enumerate(zip(REQ_PROMPTS, seeds))]


@contextlib.contextmanager
def eos_probability(model, eos_id, p):
    """TEST-LOCAL stand-in for a checkpoint that HAS an end-of-sequence token: inside the context `model.logits_from` returns its logits with the EOS entry
    of every row replaced by logsumexp(the other entries) + log(p / (1 - p)), so the EOS has probability p at every step of every request, for generate()
    and the Engine alike (both take their logits from `logits_from`; nothing else of the model changes).  The synth-filled models give their EOS id the
    probability of any other token (1e-3 .. 1e-5), so EOS candidates hardly ever rank among the first num_beams and num_beams hypotheses never collect;
    with p of a few tenths they collect within a few steps, and `_BeamHypotheses.is_done` ends a request as soon as a step's best candidate, averaged
    over its length, falls behind the worst of them."""
    import math
    orig, shift = model.logits_from, math.log(p / (1.0 - p))

    def logits_from(h16, B, S):
        lg = orig(h16, B, S)
        rest = lg.float().clone()
        rest[..., eos_id] = float("-inf")
        lg[..., eos_id] = (rest.logsumexp(dim=-1) + shift).to(lg.dtype)
        return lg
    model.logits_from = logits_from
    try:
        yield
    finally:
        model.__dict__.pop("logits_from", None)


def video(which, D, device="cpu"):
    from _util import T
    return T("beams.video.0", (VIDEO_LEN, D), 0.05).to(device)


@contextlib.contextmanager
def recorded_candidates():
    """records the merged candidate scores of every beam step inside the context, from both sides of the comparison:
      rec["alone"]   [scores f64 [2 * nb + 1]] per step of a from-scratch run — torch.topk as _generate_beams calls it, asked for one candidate more —, or
                     the 2 * nb merged scores of generation._device_candidates (selection="device": the kernel gives no more)
      rec["engine"]  [scores [2 * nb]] per generation._BeamRequest.process call
    a test slices them per request (it knows the order of its calls)"""
    from stllm_amd import generation
    rec = {"alone": [], "engine": []}
    topk, dev_cand, process = torch.topk, generation._device_candidates, generation._BeamRequest.process

    def topk_spy(x, k, *a, **kw):
        if x.dim() == 2 and x.shape[0] == 1 and kw.get("sorted") and x.shape[1] > k:
            rec["alone"].append(topk(x, k + 1, *a, **kw).values[0].double().cpu())
        return topk(x, k, *a, **kw)

    def dev_spy(*a, **kw):
        cs, ct, cb = dev_cand(*a, **kw)
        rec["alone"].append(cs[0].double())
        return cs, ct, cb

    def process_spy(self, cs, ct, cb):
        rec["engine"].append((id(self), cs.double().clone()))
        return process(self, cs, ct, cb)
    torch.topk, generation._device_candidates, generation._BeamRequest.process = topk_spy, dev_spy, process_spy
    try:
        yield rec
    finally:
        torch.topk, generation._device_candidates, generation._BeamRequest.process = topk, dev_cand, process


def alone(model, prompts, nb, vid=None, max_new=REQ_MAX_NEW, **k):
    """generate(num_beams=nb) of every request alone, from scratch ([video,] prompt prefilled in one call): (ids per request, the recorded candidate scores
    per request and step)"""
    out, steps = [], []
    for p, n in zip(prompts, max_new):
        whole = p if vid is None else torch.cat([vid, p])
        with recorded_candidates() as rec:
            out.append(model.generate(inputs_embeds=whole[None], max_new_tokens=n, num_beams=nb, **k)[0])
        steps.append(rec["alone"])
    return out, steps


def serve(model, prompts, nb, slots, max_len, prefix=None, base=None, max_new=REQ_MAX_NEW, **k):
    """the same requests through serving.Engine(num_beams=nb): (ids per request in submission order, the engine, the candidate scores per request and
    step).  At the end the engine is idle and every row is back at 0 (with a base: at the base's length)."""
    from stllm_amd import serving
    eng = serving.Engine(model, slots, max_len, num_beams=nb, base=base, **k)
    assert eng.cache.batch == slots * nb
    handles = [eng.submit(p, prefix=prefix, max_new_tokens=n) for p, n in zip(prompts, max_new)]
    order = {}
    with recorded_candidates() as rec:
        got = {}
        while not eng.idle():
            for r in list(eng.running.values()) + list(eng.queue):
                order[r.handle] = r
            got.update(dict(eng.step()))
        eng.run()
    P = base.len if base is not None else 0
    assert sorted(got) == sorted(handles) and eng.idle() and eng.cache.row_lens() == [P] * (slots * nb)
    by_state = {}
    for key, cs in rec["engine"]:
        by_state.setdefault(key, []).append(cs)
    steps = [by_state[id(order[h].beam)] for h in handles]
    return [got[h] for h in handles], eng, steps


MAX_LEN = 40        # positions of a slot: video 11 + prompt <= 9 + max_new_tokens <= 8 fit with room


def check_engine(model, which, nb, mode, device, extra=None, eos=True, poisoned=False):
    """the engine case: five requests of different prompt lengths and max_new_tokens over 2 slots with nb beams — mode "none" (whole prompts), "prefix"
    (submit(prefix=) behind a prefilled video) or "base" (Engine(base=)) — in BOTH states: every request's ids equal generate(num_beams=nb) of that request
    alone (state="device": generate(selection="device")), under the guard; both kinds of step ran; the prefix / base keeps its bits.
    eos without extra: the EARLY table — an EOS id with a probability of a few tenths at every step (eos_probability): hypotheses finish mid-way and
    `is_done` ends at least one request BEFORE its budget while another runs to its limit, asserted for the from-scratch runs and for the Engine in both
    states.  extra: more options (penalties, stop sequences) on the SEEDS table, whose EOS id some request's beams emit mid-way; eos=False: no EOS id."""
    with_video = mode != "none"
    if eos and not extra:
        seeds, eos_id, p = EARLY[which][(nb, with_video)]
        with eos_probability(model, eos_id, p):
            return _check_engine(model, which, nb, mode, device, seeds, eos_id, {}, poisoned, early=True)
    seeds, eos_id = SEEDS[which][(nb, with_video)]
    return _check_engine(model, which, nb, mode, device, seeds, eos_id if eos else None, extra or {}, poisoned, early=False)


def _check_engine(model, which, nb, mode, device, seeds, eos_id, extra, poisoned, early):
    lm = model.model
    D = lm.config.hidden_size
    with_video = mode != "none"
    prompts = requests(which, nb, D, device, with_video, seeds)
    vid = video(which, D, device) if with_video else None
    k = dict(do_sample=False, min_length=1, eos_token_id=eos_id)   # (min_length 1, as Chat.answer: an EOS hypothesis of length 0 has no score)
    k.update(extra)
    want, a_steps = alone(model, prompts, nb, vid, **k)
    want_dev, d_steps = alone(model, prompts, nb, vid, selection="device", **k)

    def ended_early(steps):
        """per request: is_done closed it before its budget (it ran fewer beam steps than max_new_tokens; no stop sequence, no criterion in this case)"""
        return [len(s) < n for s, n in zip(steps, REQ_MAX_NEW)]
    if early:
        # the precondition, from the from-scratch runs: is_done ends a request before its budget, another one runs to its limit; and a best hypothesis
        # that ended on the EOS is returned with the EOS appended
        for steps in (a_steps, d_steps):
            assert any(ended_early(steps)) and not all(ended_early(steps)), (which, nb, mode, [len(s) for s in steps])
        assert any(w.numel() < n and int(w[-1]) == eos_id for w, n in zip(want, REQ_MAX_NEW))
    pre = before = None
    if with_video:
        pre = lm.new_cache(1, VIDEO_LEN, device)
        lm.prefill(vid[None], None, cache=pre)
        before = [x.clone() for x in pre.qkv]
    out = {}
    for state, ref in (("host", want), ("device", want_dev)):
        ctx = _poison.poisoned_allocations() if poisoned else contextlib.nullcontext()
        with ctx as counts:
            got, eng, e_steps = serve(model, prompts, nb, 2, MAX_LEN, prefix=pre if mode == "prefix" else None, base=pre if mode == "base" else None,
                                      state=state, **k)
        assert not poisoned or counts.allocations > 0
        guard(a_steps, e_steps, nb, f"{which} nb={nb} {mode} {state}")
        # (the guard asserts that every request ran the from-scratch run's number of steps; said once more for the case this is about)
        assert not early or (ended_early(e_steps) == ended_early(a_steps) and any(ended_early(e_steps))), (which, nb, mode, state)
        assert len(got) == len(ref) == len(REQ_PROMPTS), "no request is dropped from the comparison"
        for i, (g, w) in enumerate(zip(got, ref)):
            assert g.dtype == torch.long and g.dim() == 1 and g.tolist() == w.tolist(), (which, nb, mode, state, i, g.tolist(), w.tolist())
        assert eng.steps["segments"] >= 3 and eng.steps["decode"] >= 1 and eng.steps["reorder"] >= 1, eng.steps
        out[state] = got
    if with_video:
        assert pre.len == VIDEO_LEN and all(_poison.bits_equal(x, y) for x, y in zip(pre.qkv, before)), "the prefix / base is only read"
    return out, want


def guard(alone_steps, engine_steps, nb, what=""):
    """the condition that keeps an id comparison from hiding a failure: over all requests and steps, the smallest gap between adjacent entries of the
    top 2 * nb + 1 merged candidates of the from-scratch run is at least 100 x the largest deviation between the Engine's and the from-scratch run's candidate
    scores at the same step.  Scores at or below -1e8 (everything behind a -1e9 beam score: one fp32 number for a whole beam) and -inf (a suppressed EOS)
    take no part in either.  Returns (gap, deviation)."""
    gap, dev = float("inf"), 0.0
    for a_steps, e_steps in zip(alone_steps, engine_steps):
        assert len(a_steps) == len(e_steps), (what, "a request ran a different number of steps", len(a_steps), len(e_steps))
        for a, e in zip(a_steps, e_steps):
            live = a[torch.isfinite(a) & (a > -1e8)]
            if live.numel() > 1:
                gap = min(gap, float((live[:-1] - live[1:]).min()))
            n = min(a.numel(), e.numel())
            both = torch.isfinite(a[:n]) & (a[:n] > -1e8) & torch.isfinite(e[:n]) & (e[:n] > -1e8)
            if both.any():
                dev = max(dev, float((a[:n][both] - e[:n][both]).abs().max()))
    print(f"[{what}] smallest gap among the top {2 * nb + 1} from-scratch candidates {gap:.3e}, largest Engine-vs-from-scratch score deviation {dev:.3e}")
    assert gap >= 100 * dev, (what, "the guard: choose other prompt seeds", gap, dev)
    return gap, dev
