"""CPU: device token selection (stllm_select_tokens / stllm_beam_candidates, generate(selection="device")).

  1. ABI: both names declared, exported, listed, bound; the version stays 7 (an additive change).
  2. the kernels of st-llm_amd/csrc/elementwise.hip compiled for the host (tests/hipemu) and called through hip.py's bindings, against the contract in
     tests/_select_ref.py (fp64): rows 1 / 5 / 17, V 1 .. 32001 in rows padded to 128 with NaN / +inf behind V, n_prev
     0 / 1 / 300 with duplicates, penalty 1 / 1.5, EOS suppressed at the argmax, maximum at 0 and at V - 1, exact ties, temperature, top_p, logit scale,
     u = 0 / 0.5 / 1 - 2^-24 + 64 seeded values, k 1 / 6 / 10 / 32, finished rows.  The bands are derived in _select_ref.py.
  3. the reference itself against today's torch code (generation._process_logits / _warp_logits / the topk flow).
  4. generate(selection="device") on the contract backend with the two reference functions in place of the kernels: the ids of the default path."""
import contextlib
import os
import re

import pytest
import torch

import _cpu_backend as CB
import _hipemu
import _select_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
emu = pytest.mark.skipif(not _hipemu.available(), reason="ROCm clang++ not found: cannot build the emulated kernels")


# ---- 1. ABI ----------------------------------------------------------------------------------------------------------------------------------------
def test_abi_declares_exports_and_binds_the_selection_entry_points():
    from stllm_amd import hip
    header = open(os.path.join(ROOT, "include", "stllm_hip.h")).read()
    assert re.search(r"^int stllm_select_tokens\(const stllm_select_args\* args, void\* stream\);", header, re.M)
    assert re.search(r"^int stllm_beam_candidates\(const stllm_beam_args\* args, void\* stream\);", header, re.M)
    for name in ("stllm_select_tokens", "stllm_beam_candidates"):
        assert name in hip.EXPORTS

    class _L:
        pass
    fake = _L()
    for n in hip.EXPORTS:
        setattr(fake, n, _L())
    hip._bind(fake)
    assert len(fake.stllm_select_tokens.argtypes) == 2 and len(fake.stllm_beam_candidates.argtypes) == 2
    # the ctypes structures mirror the header's field lists, name by name
    for struct, cls in (("stllm_select_args", hip.SelectArgs), ("stllm_beam_args", hip.BeamArgs)):
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for decl in body.split(";") if decl.strip() for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip().replace("*", " "))]
        assert names == [f[0] for f in cls._fields_], (struct, names)
    if os.path.exists(hip.LIB_PATH):
        L = hip.lib()
        assert L.stllm_abi_version() == 7
        assert hasattr(L, "stllm_select_tokens") and hasattr(L, "stllm_beam_candidates")


# ---- 2. the kernels, host-emulated -------------------------------------------------------------------------------------------------------------------
@emu
@pytest.mark.parametrize("V,rows", [(1, 1), (1, 17), (5, 5), (63, 17), (64, 1), (65, 5), (1000, 17), (4097, 5), (32000, 1), (32001, 1)])
def test_emulated_greedy(V, rows):
    with _hipemu.emulated() as hip:
        for n_prev, pen in ((0, 1.0), (1, 1.5), (300, 1.5), (300, 1.0)):
            lg, prev = R.make_case(rows, V, scale=4.0, n_prev=n_prev, seed=rows)
            R.check_greedy(hip, "cpu", lg, prev, n_prev=n_prev, penalty=pen, finished=(rows - 2,) if rows > 2 else ())
        for at in (0, V - 1):                                      # the maximum at either end; then the EOS suppressed where it is the argmax
            lg, prev = R.make_case(rows, V, scale=1.0, n_prev=0, seed=7, max_at=at)
            tok = R.check_greedy(hip, "cpu", lg, prev)
            assert bool((tok == at).all())
            if V > 1:
                tok = R.check_greedy(hip, "cpu", lg, prev, suppress_eos=True, eos_id=at)
                assert bool((tok != at).all())
            R.check_greedy(hip, "cpu", lg, prev, eos_id=at)        # ... and emitted: the row's `unfinished` drops to 0
        lg, prev = R.make_case(rows, V, scale=2.0, seed=3, tie=True)
        tok = R.check_greedy(hip, "cpu", lg, prev)                 # an exact tie of the maximum: the lowest index
        if V >= 2:
            assert bool((tok == V // 3).all())


SAMPLE_CONFIGS = [(1.0, 1.0, 0, 1.0), (0.9, 0.7, 300, 1.5), (0.3, 1.0, 1, 1.5), (1e-6, 0.7, 0, 1.0), (0.999, 1.0, 300, 1.5)]   # top_p, temperature, n_prev, penalty
VOCABS = [1, 5, 63, 64, 65, 1000, 4097, 32000, 32001]


@emu
@pytest.mark.parametrize("V", VOCABS)
def test_emulated_sample(V):
    """every configuration at one logit scale each (the scales rotate with V and the configuration; the device test runs the full product and all 67
    draws): one launch of 17 rows = u in {0, 0.5, 1 - 2^-24} + 14 seeded values; the full-vocabulary cases run one row per launch, four draws"""
    u = R.u_values(14)
    rows = 1 if V >= 32000 else 17
    with _hipemu.emulated() as hip:
        for i, (top_p, temp, n_prev, pen) in enumerate(SAMPLE_CONFIGS):
            scale = (1.0, 4.0, 12.0)[(i + VOCABS.index(V)) % 3]
            lg, prev = R.make_case(rows, V, scale=scale, n_prev=n_prev, seed=11)
            kw = dict(n_prev=n_prev, penalty=pen, temperature=temp, top_p=top_p, suppress_eos=(V > 5), eos_id=int(lg[0].argmax()))
            for i0 in range(0, 17 if rows > 1 else 4, rows):
                tok = R.check_sample(hip, "cpu", lg, prev, u[i0:i0 + rows].clone(), **kw)
                if top_p == 1e-6:                                  # a nucleus of one token: the argmax whatever u says
                    kw2 = {k: v for k, v in kw.items()}
                    assert torch.equal(tok, R.row_stats(lg, prev=prev, **kw2).amax)


@emu
def test_emulated_sample_finished_rows_and_reproducibility():
    lg, prev = R.make_case(5, 1000, scale=4.0, n_prev=300, seed=5)
    u = R.u_values()[3:8].clone()
    with _hipemu.emulated() as hip:
        outs = []
        for _ in range(2):
            unf = torch.tensor([1, 0, 1, 1, 0], dtype=torch.int32)
            out = torch.full((5,), -1, dtype=torch.int32)
            aux = torch.zeros(5, 4)
            hip.select_tokens(lg, out, prev=prev, n_prev=300, penalty=1.5, eos_id=2, pad_id=9, sample=True, temperature=0.7, top_p=0.9, u=u, unfinished=unf, aux=aux)
            assert out[1] == 9 and out[4] == 9 and unf.tolist() == [1, 0, 1, 1, 0]
            outs.append((out.clone(), aux.clone()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "a launch is bit-reproducible"


@emu
@pytest.mark.parametrize("V", [1, 5, 63, 64, 65, 1000, 4097, 32000, 32001])
def test_emulated_beam_candidates(V):
    rows = 1 if V >= 32000 else 5
    bs = torch.tensor([0.0, -0.3, -1.1, -2.0, -1e9])[:rows]
    with _hipemu.emulated() as hip:
        for k in (1, 6, 10, 32):
            if k > V:
                continue
            for n_prev, pen, sup in ((0, 1.0, False), (300, 1.5, True), (1, 1.5, True)):
                lg, prev = R.make_case(rows, V, scale=4.0, n_prev=n_prev, seed=k)
                R.check_beam(hip, "cpu", lg, prev, bs, k, n_prev=n_prev, penalty=pen, suppress_eos=sup, eos_id=int(lg[0].argmax()))
    if V >= 10:
        with _hipemu.emulated() as hip:                            # 17 rows: more than one beam group, the planted maximum at V - 1
            lg, prev = R.make_case(17, V, scale=1.0, n_prev=300, seed=2, max_at=V - 1) if V < 32000 else R.make_case(1, V, scale=1.0, n_prev=300, seed=2, max_at=V - 1)
            R.check_beam(hip, "cpu", lg, prev, torch.linspace(0, -3, lg.shape[0]), 10, n_prev=300, penalty=1.5)


@emu
def test_emulated_unsupported_vocabulary_raises():
    """a row that does not fit the LDS is an error of the entry point, through the binding: nothing else runs in its place"""
    lg = torch.zeros(1, 160 * 1024 // 4)
    with _hipemu.emulated() as hip:
        with pytest.raises(RuntimeError, match="LDS"):
            hip.select_tokens(lg, torch.zeros(1, dtype=torch.int32))
        with pytest.raises(RuntimeError, match="LDS"):
            hip.beam_candidates(lg, torch.zeros(1), 4)
        with pytest.raises(RuntimeError, match="k="):
            hip.beam_candidates(lg[:, :5], torch.zeros(1), 6)


# ---- 3. the reference against today's torch code -----------------------------------------------------------------------------------------------------
def test_reference_matches_todays_processors():
    from stllm_amd import generation as G
    for V, scale in ((5, 1.0), (1000, 4.0), (32001, 12.0), (32001, 1.0)):
        lg, prev = R.make_case(4, V, scale=scale, n_prev=300, seed=21)
        eos = int(lg[0].argmax())
        ids = prev[:, :300].long()
        # greedy = _process_logits + argmax (the penalty is one fp32 operation on both sides: bit-equal scores)
        today = G._process_logits(lg.contiguous(), ids, 0, 1.5, 3, eos)
        out = torch.empty(4, dtype=torch.int32)
        R.select_tokens(lg, out, prev=prev, n_prev=300, penalty=1.5, suppress_eos=True, eos_id=eos)
        assert torch.equal(R.processed(lg.float(), prev, 300, 1.5, True, eos), today)
        assert torch.equal(out.long(), today.argmax(dim=-1))
        # kept set = the finite entries of _warp_logits, outside the band
        for top_p in (0.3, 0.9, 0.999):
            st = R.row_stats(lg, prev=prev, n_prev=300, penalty=1.5, suppress_eos=True, eos_id=eos, temperature=0.7, top_p=top_p)
            kept_today = torch.isfinite(G._warp_logits(today, 0.7, top_p))
            outside = ((st.mass - (1 - top_p)).abs() > R.BAND)
            assert torch.equal(st.kept[outside], kept_today[outside]), (V, scale, top_p)


@pytest.mark.parametrize("nb", [3, 5])
def test_reference_merged_candidates_match_todays_topk(nb):
    from stllm_amd import generation as G
    V, B = 32001, 2
    lg, prev = R.make_case(B * nb, V, scale=4.0, n_prev=300, seed=31)
    eos = int(lg[0].argmax())
    beam_scores = torch.tensor([0.0, -0.3, -1.1, -2.0, -1e9][:nb - 1] + [-1e9] + [0.0] + [-1e9] * (nb - 1))
    with CB._patched({"beam_candidates": R.beam_candidates}):
        cs, ct, cb = G._device_candidates(lg, prev[:, :300].long(), beam_scores, B, nb, repetition_penalty=1.5, suppress_eos=True, eos_token_id=eos)
    logp = G._process_logits(lg.contiguous().log_softmax(dim=-1), prev[:, :300].long(), 0, 1.5, 1, eos)
    want_s, want_t = torch.topk((logp + beam_scores[:, None]).view(B, nb * V), 2 * nb, dim=1)
    live = want_s > -1e8                                           # behind a -1e9 beam score every candidate is the same fp32 number: any of them will do
    assert torch.equal((cb * V + ct)[live], want_t[live])
    assert float((cs - want_s)[live].abs().max()) <= R.BAND
    assert torch.equal(cs[~live], want_s[~live])
    flat = (cb * V + ct)
    assert all(len(set(row.tolist())) == 2 * nb for row in flat) and bool(((ct >= 0) & (ct < V)).all())


# ---- 4. generate(selection="device") on the contract backend ----------------------------------------------------------------------------------------------
HID, INTER, LAYERS, HEADS, VOCAB = 256, 512, 2, 2, 256


@pytest.fixture(scope="module")
def model():
    from stllm_amd import synth
    from stllm_amd.models.st_llm import STLLMForCausalLM, StllmConfig
    m = STLLMForCausalLM(StllmConfig(hidden_size=HID, intermediate_size=INTER, num_hidden_layers=LAYERS, num_attention_heads=HEADS, vocab_size=VOCAB,
                                     rms_norm_eps=1e-6), device="cpu")
    synth.fill_module_(m, 5, "")
    with torch.no_grad():
        m.lm_head.weight.mul_(40.0)
    return m


@contextlib.contextmanager
def _backend():
    from stllm_amd import runtime
    with CB.installed(), CB._patched({"select_tokens": R.select_tokens, "beam_candidates": R.beam_candidates}), runtime.use_dtype("fp32"):
        yield


def _emb(B, S, seed):
    return torch.randn(B, S, HID, generator=torch.Generator().manual_seed(seed)) * 0.5


def _both(model, emb, **kw):
    with _backend():
        return model.generate(inputs_embeds=emb, **kw), model.generate(inputs_embeds=emb, selection="device", **kw)


def test_generate_device_greedy_matches_default(model):
    want, got = _both(model, _emb(1, 6, 0), max_new_tokens=8, min_length=2, repetition_penalty=1.5)
    assert got.dtype == torch.long and torch.equal(got, want)
    want, got = _both(model, _emb(1, 6, 0), max_new_tokens=8, min_length=2, repetition_penalty=1.5, use_cache=False)
    assert torch.equal(got, want)


def test_generate_device_ragged_prefix_and_eos(model):
    emb = _emb(3, 7, 1)
    mask = torch.tensor([[1] * 7, [1] * 4 + [0] * 3, [1] * 6 + [0]])
    kw = dict(max_new_tokens=7, min_length=1, repetition_penalty=1.5, attention_mask=mask, batching="ragged")
    want, got = _both(model, emb, **kw)
    assert torch.equal(got, want)
    # an EOS hit: a token the free run emits in the middle of row 0 ends that row, the others go on; lengths are reported as today
    seq = want[0].tolist()
    eos = next(seq[i] for i in range(1, len(seq)) if seq[i] not in seq[:i])
    (want, wn), (got, gn) = _both(model, emb, eos_token_id=eos, return_lengths=True, **kw)
    assert torch.equal(got, want) and gn == wn and min(wn) < 7
    with _backend():
        prefix = model.model.new_cache(1, 4, "cpu")
        model.model.prefill(_emb(1, 4, 2), None, cache=prefix)
        q = _emb(1, 5, 3)
        k = dict(max_new_tokens=6, repetition_penalty=1.5, prefix_cache=prefix)
        assert torch.equal(model.generate(inputs_embeds=q, selection="device", **k), model.generate(inputs_embeds=q, **k))
        k = dict(k, num_beams=3, share_prefix=True)
        assert torch.equal(model.generate(inputs_embeds=q, selection="device", **k), model.generate(inputs_embeds=q, **k))


@pytest.mark.parametrize("nb", [3, 5])
def test_generate_device_beams_match_default(model, nb):
    emb = _emb(1, 5, 10 + nb)
    kw = dict(max_new_tokens=7, num_beams=nb, repetition_penalty=1.5, min_length=3)
    want, got = _both(model, emb, **kw)
    assert torch.equal(got, want)
    seq = want[0].tolist()
    eos = seq[4]                                                   # an EOS hit behind min_length: hypotheses close early
    want, got = _both(model, emb, eos_token_id=eos, **kw)
    assert torch.equal(got, want)
    stop = [torch.tensor(seq[2:4])]
    want, got = _both(model, emb, stop_sequences=stop, **kw)
    assert torch.equal(got, want) and want.shape[1] < 7
    want, got = _both(model, _emb(2, 5, 20 + nb), **kw)            # two prompts
    assert torch.equal(got, want)


def test_generate_device_stop_sequences_and_sync_every(model):
    emb = _emb(3, 6, 4)
    free = _both(model, emb, max_new_tokens=9, repetition_penalty=1.5)[0]
    stop = [free[1, 2:4].clone()]
    seq = free[0].tolist()
    eos = next(seq[i] for i in range(2, len(seq)) if seq[i] not in seq[:i])
    kw = dict(max_new_tokens=9, repetition_penalty=1.5, stop_sequences=stop, eos_token_id=eos, return_lengths=True)
    (want, wn), (got, gn) = _both(model, emb, **kw)
    assert torch.equal(got, want) and gn == wn
    with _backend():
        for K in (4, 100):
            ids, n = model.generate(inputs_embeds=emb, selection="device", sync_every=K, **kw)
            assert torch.equal(ids, want) and n == wn, K
        # every row finishes early: the result is cut where the last of them had, whatever the read-back interval
        one = dict(max_new_tokens=9, repetition_penalty=1.5, eos_token_id=int(free[0, 1]))
        a = model.generate(inputs_embeds=emb[:1], **one)
        b = model.generate(inputs_embeds=emb[:1], selection="device", sync_every=4, **one)
        assert a.shape[1] == 2 and torch.equal(a, b)

        class StopAt3:
            def __call__(self, ids, scores):
                return ids.shape[1] >= 3
        a = model.generate(inputs_embeds=emb, max_new_tokens=9, stopping_criteria=[StopAt3()])
        b = model.generate(inputs_embeds=emb, max_new_tokens=9, stopping_criteria=[StopAt3()], selection="device", sync_every=4)   # a criterion forces K = 1
        assert a.shape[1] == 3 and torch.equal(a, b)
        with pytest.raises(ValueError):
            model.generate(inputs_embeds=emb, selection="cuda")


def test_generate_device_sampling(model):
    emb = _emb(2, 5, 6)
    g = lambda: torch.Generator().manual_seed(123)
    with _backend():
        greedy = model.generate(inputs_embeds=emb, max_new_tokens=6, repetition_penalty=1.5)
        tiny = model.generate(inputs_embeds=emb, max_new_tokens=6, repetition_penalty=1.5, do_sample=True, top_p=1e-6, generator=g(), selection="device")
        assert torch.equal(tiny, greedy), "a nucleus of one token is greedy search"
        kw = dict(max_new_tokens=6, do_sample=True, top_p=0.95, temperature=4.0, selection="device")
        a, b = model.generate(inputs_embeds=emb, generator=g(), **kw), model.generate(inputs_embeds=emb, generator=g(), **kw)
        assert torch.equal(a, b), "the same seed gives the same ids"
        c = model.generate(inputs_embeds=emb, generator=torch.Generator().manual_seed(7), **kw)
        assert not torch.equal(a, c)


def test_generate_device_uses_no_torch_selection_operator(model, monkeypatch):
    def boom(name):
        def f(*a, **k):
            raise AssertionError(f"{name} ran in device mode")
        return f
    emb = _emb(1, 5, 8)
    with _backend():
        want = [model.generate(inputs_embeds=emb, max_new_tokens=5, repetition_penalty=1.5, **kw) for kw in (dict(), dict(num_beams=3))]
        for name in ("sort", "multinomial", "topk"):
            monkeypatch.setattr(torch, name, boom("torch." + name))
        monkeypatch.setattr(torch.Tensor, "log_softmax", boom("Tensor.log_softmax"))
        with pytest.raises(AssertionError):
            model.generate(inputs_embeds=emb, max_new_tokens=5, num_beams=3)
        got = [model.generate(inputs_embeds=emb, max_new_tokens=5, repetition_penalty=1.5, selection="device", **kw) for kw in (dict(), dict(num_beams=3))]
        model.generate(inputs_embeds=emb, max_new_tokens=5, do_sample=True, top_p=0.9, generator=torch.Generator().manual_seed(1), selection="device")
    assert all(torch.equal(a, b) for a, b in zip(got, want))
