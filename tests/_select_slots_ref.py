"""TEST-ONLY: the contract of stllm_select_slots (include/stllm_hip.h) stated once, on the CPU, with the signature of hip.select_slots: `_select_ref.select_tokens`
row by row — every served live slot with ITS n_prev, suppress_eos and u — plus the state update.  `_cpu_backend._patched({"select_slots": select_slots})`
runs serving.Engine(state="device") without a GPU; the kernel tests (emulated and on the device) run `check` below, which compares a launch with
hip.select_tokens called once per slot (bit-equal token and aux) followed by `update` (the state and id tables)."""
import torch

import _select_ref as R

LIVE, N_GEN, MAX_NEW, PENDING = 0, 1, 2, 3


def ends_in_stop(hist, stops, stop_len):
    """the contract's stop rule on a list of ids: some j with 0 < stop_len[j] <= len(hist) whose ids are the tail of hist"""
    for j in range(0 if stops is None else stops.shape[0]):
        n = int(stop_len[j])
        if 0 < n <= len(hist) and n <= stops.shape[1] and hist[len(hist) - n:] == stops[j, :n].tolist():
            return True
    return False


def update(state_row, ids_row, token, *, eos_id, stops, stop_len):
    """the state update of one live served slot, in place; token: the int that selection gave"""
    ld = ids_row.numel()
    c = min(max(int(state_row[N_GEN]), 0), ld - 1)
    ids_row[c] = token
    hist = ids_row[:c + 1].tolist()
    dead = (eos_id is not None and token == eos_id) or c + 1 >= int(state_row[MAX_NEW]) or ends_in_stop(hist, stops, stop_len)
    state_row[LIVE], state_row[N_GEN], state_row[PENDING] = (0 if dead else 1), c + 1, token


def select_slots(logits, src, state, ids, *, penalty=1.0, min_length=0, eos_id=None, pad_id=0, sample=False, temperature=1.0, top_p=1.0, u=None, stops=None,
                 stop_len=None, aux=None, select=None):
    """select: the one-row selection to build on (default: the fp64 contract `_select_ref.select_tokens`; `check` passes hip.select_tokens)"""
    select = select or R.select_tokens
    rows = logits.shape[0]
    for s in range(src.numel()):
        r = int(src[s])
        if not 0 <= r < rows:
            continue
        if int(state[s, LIVE]) == 0:
            state[s, PENDING] = pad_id
            continue
        n_gen = int(state[s, N_GEN])
        c = min(max(n_gen, 0), ids.shape[1] - 1)
        out = torch.empty(1, dtype=torch.int32)
        select(logits[r:r + 1], out, prev=ids[s:s + 1], n_prev=c, penalty=penalty, suppress_eos=eos_id is not None and n_gen < min_length, eos_id=eos_id,
               pad_id=pad_id, sample=sample, temperature=temperature, top_p=top_p, u=u[s:s + 1] if sample else None, aux=aux[s:s + 1] if aux is not None else None)
        update(state[s], ids[s], int(out[0]), eos_id=eos_id, stops=stops, stop_len=stop_len)
    return state


# ---- the kernel case, shared by tests/test_select_slots_cpu.py (host-emulated kernel) and tests/test_select_slots_gpu.py (the device) -------------------------
STOPS = [[7], [3, 4], [2, 9, 5], [1, 2, 3, 4, 5, 6]]        # lengths 1, 2, 3 and one longer than the short histories
IN_RANGE_SENTINEL, OUT_OF_RANGE_SENTINEL = 0, 2 ** 30


def stop_tables(stops=STOPS, pad=-3):
    ld = max(len(s) for s in stops)
    t = torch.full((len(stops), ld), pad, dtype=torch.int32)   # behind stop_len: never read, so a value that no token can equal would not matter either
    for j, s in enumerate(stops):
        t[j, :len(s)] = torch.tensor(s, dtype=torch.int32)
    return t, torch.tensor([len(s) for s in stops], dtype=torch.int32)


class SlotCase:
    """n_slots slots over `rows = n_slots + 1` logits rows [rows, V] (padded, NaN / +inf behind V): src is a permutation of the rows with -1 entries and one
    entry >= rows (from 5 slots on); slot s holds n_gen = {0, 1, 300, ld_ids - 1}[(s + rot) % 4] ids, so one launch mixes them; some slots are dead; max_new
    is reached exactly by the even slots and missed by one by the odd ones; ids behind n_gen hold `sentinel`.  plant(): make a token this step's argmax."""

    def __init__(self, n_slots, V, ld_ids, *, seed=0, rot=0, scale=4.0, sentinel=OUT_OF_RANGE_SENTINEL, n_gens=None):
        self.n_slots, self.V, self.ld_ids = n_slots, V, ld_ids
        g = torch.Generator().manual_seed(7000 * seed + 31 * V + n_slots)
        self.rows = n_slots + 1
        self.logits = R.padded_logits(torch.randn(self.rows, V, generator=g) * scale)
        perm = torch.randperm(self.rows, generator=g)[:n_slots].to(torch.int32)
        self.src = perm.clone()
        if n_slots >= 5:
            self.src[1], self.src[3] = -1, self.rows + 2          # not served: a negative entry and one >= rows
        cyc = n_gens or [0, 1, 300, ld_ids - 1]
        self.n_gen = [min(cyc[(s + rot) % len(cyc)], ld_ids - 1) for s in range(n_slots)]
        self.ids = torch.full((n_slots, ld_ids), sentinel, dtype=torch.int32)
        for s, n in enumerate(self.n_gen):
            self.ids[s, :n] = torch.randint(0, V, (n,), generator=g).to(torch.int32)
            if n >= 4:
                self.ids[s, n // 2:n] = self.ids[s, :n - n // 2].clone()   # duplicates, as _select_ref.make_case
        self.state = torch.zeros((n_slots, 4), dtype=torch.int32)
        for s, n in enumerate(self.n_gen):
            live = 0 if (n_slots >= 5 and s % 5 == 2) else 1       # dead slots
            max_new = n + 1 if s % 2 == 0 else n + 2               # reached exactly by this step / missed by one
            self.state[s] = torch.tensor([live, n, max_new, -9], dtype=torch.int32)
        self.u = torch.rand(n_slots, generator=g)

    def served(self):
        return [s for s in range(self.n_slots) if 0 <= int(self.src[s]) < self.rows]

    def plant(self, slot, token, boost=50.0):
        """make `token` the clear argmax of the slot's row, whatever the penalty does to it"""
        self.logits[int(self.src[slot]), token] = float(self.logits[int(self.src[slot])].max()) + boost


def launch(hip, dev, case, **kw):
    """one hip.select_slots launch of the case on `dev`: (state, ids, aux) back on the CPU"""
    state, ids = case.state.clone().to(dev), case.ids.clone().to(dev)
    aux = torch.full((case.n_slots, 4), -5.0, device=dev)
    k = dict(kw)
    for n in ("stops", "stop_len"):
        if k.get(n) is not None:
            k[n] = k[n].to(dev)
    hip.select_slots(R.on_device(case.logits, dev), case.src.to(dev), state, ids, u=case.u.to(dev) if kw.get("sample") else None, aux=aux, **k)
    return state.cpu(), ids.cpu(), aux.cpu()


def per_slot(hip, dev, case, **kw):
    """the same step as hip.select_tokens launches, one per served live slot, on `dev`, plus the reference's state update: (state, ids, aux)"""
    state, ids = case.state.clone(), case.ids.clone()
    aux = torch.full((case.n_slots, 4), -5.0)
    lg = R.on_device(case.logits, dev)

    def one(logits, out, *, prev, u, aux, **k):
        o, a = out.to(dev), aux.to(dev)
        hip.select_tokens(logits, o, prev=prev.to(dev), u=u.to(dev) if u is not None else None, aux=a, **k)
        out.copy_(o.cpu())
        aux.copy_(a.cpu())
    select_slots(lg, case.src, state, ids, u=case.u, aux=aux, select=one, **kw)
    return state, ids, aux


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def check(hip, dev, case, twice=True, **kw):
    """a launch against per-slot select_tokens launches: state and ids tables equal, aux bit-equal (untouched rows keep their fill); nothing behind n_gen and
    nothing of an unserved slot is written; a second launch gives the same bits.  Returns the state table."""
    want_state, want_ids, want_aux = per_slot(hip, dev, case, **kw)
    state, ids, aux = launch(hip, dev, case, **kw)
    assert torch.equal(state, want_state), (state.tolist(), want_state.tolist())
    assert torch.equal(ids, want_ids), "the id table"
    assert torch.equal(bits(aux), bits(want_aux)), (aux.tolist(), want_aux.tolist())
    for s in range(case.n_slots):
        if s not in case.served():
            assert torch.equal(state[s], case.state[s]) and torch.equal(ids[s], case.ids[s]) and bool((aux[s] == -5.0).all()), (s, "an unserved slot was touched")
        elif int(case.state[s, LIVE]) == 0:
            assert state[s].tolist() == [0, case.n_gen[s], int(case.state[s, MAX_NEW]), kw.get("pad_id", 0)] and torch.equal(ids[s], case.ids[s])
            assert bool((aux[s] == -5.0).all())
        else:
            c = case.n_gen[s]
            keep = torch.ones(case.ld_ids, dtype=torch.bool)
            keep[c] = False
            assert torch.equal(ids[s][keep], case.ids[s][keep]), (s, "only ids[s, n_gen] is written")
            assert int(state[s, N_GEN]) == c + 1 and int(state[s, PENDING]) == int(ids[s, c])
    if not twice:
        return state
    again = launch(hip, dev, case, **kw)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(again, (state, ids, aux))), "the same launch twice gives the same bits"
    return state
