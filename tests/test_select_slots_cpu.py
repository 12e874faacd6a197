"""CPU: token selection with per-slot state (stllm_select_slots).

  1. ABI: the name is declared, exported, listed and bound; the ctypes structure mirrors the header name by name; the version stays 7.
  2. select_slots_kernel of st-llm_amd/csrc/elementwise.hip compiled for the host (tests/hipemu) and called through hip.select_slots, against
     hip.select_tokens called once per slot on the same emulated library (token and aux bit-equal) and the state update of tests/_select_slots_ref.py:
     slots 1 / 5 / 17, V 1 .. 4097 (32001 at one slot), n_gen 0 / 1 / 300 / ld_ids - 1 mixed in one launch with ld_ids 301 and 512, src a permutation with a
     -1 and an entry >= rows, dead slots, min_length = 2 against an EOS that is the argmax, max_new reached exactly and missed by one, EOS emitted, stop
     sequences of lengths 1 / 2 / 3 (match, near miss, longer than the history, n_stop = 0), sentinels behind n_gen, greedy and the five sampling
     configurations of test_select_cpu.py with u = 0 / 0.5 / 1 - 2^-24 and seeded values, the same launch twice, a row that does not fit the LDS."""
import os
import re

import pytest
import torch

import _hipemu
import _select_ref as R
import _select_slots_ref as SR
from test_select_cpu import SAMPLE_CONFIGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
emu = pytest.mark.skipif(not _hipemu.available(), reason="ROCm clang++ not found: cannot build the emulated kernels")
SHAPES = [(1, 1), (1, 17), (5, 5), (63, 17), (64, 1), (65, 5), (1000, 17), (4097, 5), (32001, 1)]   # (V, slots)


# ---- 1. ABI ----------------------------------------------------------------------------------------------------------------------------------------
def test_abi_declares_exports_and_binds_select_slots():
    from stllm_amd import hip
    header = open(os.path.join(ROOT, "include", "stllm_hip.h")).read()
    assert re.search(r"^int stllm_select_slots\(const stllm_select_slots_args\* args, void\* stream\);", header, re.M)
    assert "stllm_select_slots" in hip.EXPORTS and callable(hip.select_slots)

    class _L:
        pass
    fake = _L()
    for n in hip.EXPORTS:
        setattr(fake, n, _L())
    hip._bind(fake)
    assert fake.stllm_select_slots.argtypes[0]._type_ is hip.SelectSlotsArgs and len(fake.stllm_select_slots.argtypes) == 2
    body = re.search(r"typedef struct stllm_select_slots_args \{(.*?)\} stllm_select_slots_args;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") if decl.strip() for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip().replace("*", " "))]
    assert names == [f[0] for f in hip.SelectSlotsArgs._fields_], names
    shared = ["V", "ldl", "penalty", "eos_id", "pad_id", "sample", "temperature", "top_p", "u", "aux"]   # the scalar options of stllm_select_args
    assert all(n in names and n in [f[0] for f in hip.SelectArgs._fields_] for n in shared)
    if os.path.exists(hip.LIB_PATH):
        L = hip.lib()
        assert L.stllm_abi_version() == 7 and hasattr(L, "stllm_select_slots")


# ---- 2. the kernel, host-emulated --------------------------------------------------------------------------------------------------------------------
def _rots(V, slots):
    return (2, 3) if V >= 32000 else (range(4) if slots < 17 else (0,))


def greedy_state_and_ids(hip, dev, V, slots):
    """every live served slot's row has the EOS planted as its argmax: with min_length = 2 the slots at n_gen 0 and 1 suppress it (and stay live unless
    max_new is reached), the others emit it and drop `live`; repetition penalty over each slot's own history"""
    stops, stop_len = SR.stop_tables()
    for ld_ids in (301, 512):
        for rot in _rots(V, slots):
            case = SR.SlotCase(slots, V, ld_ids, seed=rot, rot=rot)
            eos = V // 2
            for s in case.served():
                case.plant(s, eos)
            kw = dict(penalty=1.5, min_length=2, eos_id=eos, pad_id=9, stops=stops, stop_len=stop_len)
            state = SR.check(hip, dev, case, **kw)
            for s in case.served():
                if int(case.state[s, SR.LIVE]) == 0:
                    continue
                n, tok = case.n_gen[s], int(state[s, SR.PENDING])
                if n < 2 and V > 1:
                    assert tok != eos, (s, "EOS is suppressed under min_length")
                    if not SR.ends_in_stop(case.ids[s, :n].tolist() + [tok], stops, stop_len):
                        assert int(state[s, SR.LIVE]) == (0 if n + 1 >= int(case.state[s, SR.MAX_NEW]) else 1), (s, "max_new reached exactly / missed by one")
                elif n >= 2:
                    assert tok == eos and int(state[s, SR.LIVE]) == 0, (s, "EOS emitted: the slot is finished")
            SR.check(hip, dev, case, penalty=1.0, eos_id=None)       # no penalty, no EOS, n_stop = 0: only max_new ends a slot
            if V > 1 and rot == 0:
                state = SR.check(hip, dev, case, penalty=1.5, eos_id=None, min_length=2)
                for s in case.served():
                    if int(case.state[s, SR.LIVE]):
                        assert int(state[s, SR.LIVE]) == (0 if s % 2 == 0 else 1), (s, "max_new reached exactly by the even slots, missed by one by the odd ones")


@emu
@pytest.mark.parametrize("V,slots", SHAPES)
def test_emulated_greedy_state_and_ids(V, slots):
    with _hipemu.emulated() as hip:
        greedy_state_and_ids(hip, "cpu", V, slots)


def _stop_case(sentinel=SR.OUT_OF_RANGE_SENTINEL):
    """17 slots, V = 1000, max_new far away: what ends a slot here is a stop sequence alone.  Returns (case, {slot: (why, live expected)})"""
    case = SR.SlotCase(17, 1000, 301, seed=9, sentinel=sentinel, n_gens=[0, 1, 300, 2])
    case.state[:, SR.MAX_NEW] = 1000
    live = [s for s in case.served() if int(case.state[s, SR.LIVE])]
    by_n = {n: [s for s in live if case.n_gen[s] == n] for n in (0, 1, 2, 300)}
    assert all(len(v) >= 2 for v in by_n.values()), by_n
    want = {}

    def tail(s, ids, token, why, alive):
        n = case.n_gen[s]
        if ids:
            case.ids[s, n - len(ids):n] = torch.tensor(ids, dtype=torch.int32)
        case.plant(s, token)
        want[s] = (why, alive)
    a, b = by_n[300][:2]
    tail(a, [2, 9], 5, "length 3, completed by this step's token", 0)
    tail(b, [8, 9], 5, "near miss: differs in the first element", 1)
    if len(by_n[300]) > 2:
        tail(by_n[300][2], [2, 9], 6, "near miss: differs in the last element", 1)
    a, b = by_n[2][:2]
    tail(a, [2, 9], 5, "length 3 over the whole history", 0)
    tail(b, [4, 5], 6, "the six-id sequence is longer than the history: no match", 1)
    a, b = by_n[1][:2]
    tail(a, [3], 4, "length 2", 0)
    tail(b, [9], 5, "length 3 is longer than the history of 2", 1)
    a, b = by_n[0][:2]
    tail(a, [], 7, "length 1 on the first token", 0)
    tail(b, [], 4, "length 2 is longer than the history of 1", 1)
    return case, want


def stop_sequences(hip, dev):
    stops, stop_len = SR.stop_tables()
    case, want = _stop_case()
    state = SR.check(hip, dev, case, penalty=1.0, eos_id=None, stops=stops, stop_len=stop_len)
    for s, (why, alive) in want.items():
        assert int(state[s, SR.LIVE]) == alive, (s, why)
    state = SR.check(hip, dev, case, penalty=1.0, eos_id=None)          # n_stop = 0: nothing matches
    assert all(int(state[s, SR.LIVE]) == 1 for s in want)
    # a stop row whose ids BEHIND stop_len would complete a longer match: they are never read
    stops2 = stops.clone()
    stops2[0, 1:3] = torch.tensor([7, 7], dtype=torch.int32)
    assert torch.equal(SR.check(hip, dev, case, penalty=1.0, eos_id=None, stops=stops2, stop_len=stop_len), SR.check(hip, dev, case, penalty=1.0,
                                                                                                                   eos_id=None, stops=stops, stop_len=stop_len))


@emu
def test_emulated_stop_sequences():
    with _hipemu.emulated() as hip:
        stop_sequences(hip, "cpu")


def ids_behind_n_gen_do_not_matter(hip, dev):
    """the history behind n_gen filled with an out-of-range and with an in-range sentinel (id 0, which a penalty would visibly move): the same results"""
    stops, stop_len = SR.stop_tables()
    kw = dict(penalty=1.5, eos_id=None, stops=stops, stop_len=stop_len)
    got = []
    for sentinel in (SR.OUT_OF_RANGE_SENTINEL, SR.IN_RANGE_SENTINEL, 7):
        case, _ = _stop_case(sentinel)
        for s in case.served():
            case.logits[int(case.src[s]), 0] = float(case.logits[int(case.src[s])].max()) + 0.25   # id 0 nearly wins: penalising it by mistake would show
        SR.check(hip, dev, case, **kw)
        state, ids, aux = SR.launch(hip, dev, case, **kw)
        got.append((state, [ids[s, :case.n_gen[s] + 1].tolist() for s in case.served() if int(case.state[s, SR.LIVE])], SR.bits(aux)))
    for g in got[1:]:
        assert torch.equal(g[0], got[0][0]) and g[1] == got[0][1] and torch.equal(g[2], got[0][2])


@emu
def test_emulated_ids_behind_n_gen_do_not_matter():
    with _hipemu.emulated() as hip:
        ids_behind_n_gen_do_not_matter(hip, "cpu")


def sample(hip, dev, V, slots, config):
    """the five sampling configurations (their top_p, temperature and penalty; n_prev is each slot's own n_gen here), u = 0, 0.5, 1 - 2^-24 on the first
    live served slots and seeded values on the others"""
    i, (top_p, temp, _, pen) = config, SAMPLE_CONFIGS[config]
    stops, stop_len = SR.stop_tables()
    ld_ids = (301, 512)[i % 2]
    for rot in ((i % 4,) if slots > 1 else ((2 + i % 2,) if V >= 32000 else range(3))):
        case = SR.SlotCase(slots, V, ld_ids, seed=20 + i, rot=rot, scale=(1.0, 4.0, 12.0)[(i + rot) % 3])
        live = [s for s in case.served() if int(case.state[s, SR.LIVE])]
        for j, s in enumerate(live[:3] if slots > 1 else live):
            case.u[s] = R.U_SPECIAL[(j + rot) % 3]
        eos = int(case.logits[int(case.src[live[0]])].argmax())
        SR.check(hip, dev, case, twice=(i == 1), sample=True, temperature=temp, top_p=top_p, penalty=pen, min_length=2, eos_id=eos, pad_id=3, stops=stops,
                 stop_len=stop_len)


@emu
@pytest.mark.parametrize("config", range(len(SAMPLE_CONFIGS)))
@pytest.mark.parametrize("V,slots", SHAPES)
def test_emulated_sample(V, slots, config):
    with _hipemu.emulated() as hip:
        sample(hip, "cpu", V, slots, config)


@emu
def test_emulated_reference_contract_agrees():
    """tests/_select_slots_ref.select_slots on the fp64 contract of _select_ref (what the Engine tests install) gives the tables of the kernel, greedy, on a
    case whose rows have a planted, clear argmax"""
    stops, stop_len = SR.stop_tables()
    case, want = _stop_case()
    kw = dict(penalty=1.5, eos_id=5, min_length=2, pad_id=9, stops=stops, stop_len=stop_len)
    state, ids = case.state.clone(), case.ids.clone()
    for s in case.served():
        if s not in want:
            case.plant(s, 11 + s)
    SR.select_slots(case.logits, case.src, state, ids, **kw)
    with _hipemu.emulated() as hip:
        got_state, got_ids, _ = SR.launch(hip, "cpu", case, **kw)
    assert torch.equal(got_state, state) and torch.equal(got_ids, ids)


@emu
def test_emulated_row_that_does_not_fit_raises():
    """V + ld_ids floats must fit the LDS: a vocabulary that stllm_select_tokens still takes alone is refused with a history of 512 behind it"""
    V = 39500
    lg = torch.zeros(1, V)
    src, state = torch.zeros(1, dtype=torch.int32), torch.tensor([[1, 0, 4, 0]], dtype=torch.int32)
    with _hipemu.emulated() as hip:
        hip.select_tokens(lg, torch.zeros(1, dtype=torch.int32))
        with pytest.raises(RuntimeError, match="LDS"):
            hip.select_slots(lg, src, state, torch.zeros((1, 512), dtype=torch.int32))
        assert state.tolist() == [[1, 0, 4, 0]]
        with pytest.raises(RuntimeError, match="LDS"):
            hip.select_slots(torch.zeros(1, 160 * 1024 // 4), src, state, torch.zeros((1, 1), dtype=torch.int32))
