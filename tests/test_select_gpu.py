"""GPU: device token selection.  The kernel cases of tests/test_select_cpu.py on the device — here the full product of vocabulary sizes, row counts, logit
scales and configurations, and all 67 draws per configuration — against the fp64 contract in tests/_select_ref.py (the bands are derived there); then
generate(selection="device") against the default path on a 2-layer, head_dim-128 decoder in bf16 and fp16."""
import pytest
import torch

import _select_ref as R

pytestmark = pytest.mark.gpu
VOCABS = [1, 5, 63, 64, 65, 1000, 4097, 32000, 32001]
SAMPLE_CONFIGS = [(1.0, 1.0, 0, 1.0), (0.9, 0.7, 300, 1.5), (0.3, 1.0, 1, 1.5), (1e-6, 0.7, 0, 1.0), (0.999, 1.0, 300, 1.5)]   # top_p, temperature, n_prev, penalty


@pytest.fixture(scope="module")
def hip():
    from stllm_amd import hip as h
    h.lib()
    return h


@pytest.mark.parametrize("V", VOCABS)
def test_greedy(hip, V):
    for rows in (1, 5, 17):
        for n_prev, pen in ((0, 1.0), (1, 1.5), (300, 1.5), (300, 1.0)):
            lg, prev = R.make_case(rows, V, scale=4.0, n_prev=n_prev, seed=rows)
            R.check_greedy(hip, "cuda", lg, prev, n_prev=n_prev, penalty=pen, finished=(rows - 2,) if rows > 2 else ())
        for at in (0, V - 1):                                      # the maximum at either end; then the EOS suppressed where it is the argmax
            lg, prev = R.make_case(rows, V, scale=1.0, n_prev=0, seed=7, max_at=at)
            assert bool((R.check_greedy(hip, "cuda", lg, prev) == at).all())
            if V > 1:
                assert bool((R.check_greedy(hip, "cuda", lg, prev, suppress_eos=True, eos_id=at) != at).all())
            R.check_greedy(hip, "cuda", lg, prev, eos_id=at)       # ... and emitted: the row's `unfinished` drops to 0
        lg, prev = R.make_case(rows, V, scale=2.0, seed=3, tie=True)
        tok = R.check_greedy(hip, "cuda", lg, prev)                # an exact tie of the maximum: the lowest index
        if V >= 2:
            assert bool((tok == V // 3).all())


@pytest.mark.parametrize("scale", [1.0, 4.0, 12.0])
@pytest.mark.parametrize("V", VOCABS)
def test_sample(hip, V, scale):
    """every draw of every configuration, no exclusions: 67 values of u over four launches of 17 rows; rows 1 and 5 take the first of them"""
    u = R.u_values()
    u = torch.cat([u, u[:1]])
    for top_p, temp, n_prev, pen in SAMPLE_CONFIGS:
        lg, prev = R.make_case(17, V, scale=scale, n_prev=n_prev, seed=11)
        kw = dict(n_prev=n_prev, penalty=pen, temperature=temp, top_p=top_p, suppress_eos=(V > 5), eos_id=int(lg[0].argmax()))
        for i0 in range(0, 68, 17):
            tok = R.check_sample(hip, "cuda", lg, prev, u[i0:i0 + 17].clone(), **kw)
            if top_p == 1e-6:                                      # a nucleus of one token: the argmax whatever u says
                assert torch.equal(tok, R.row_stats(lg, prev=prev, **kw).amax)
        for rows in (1, 5):
            lg, prev = R.make_case(rows, V, scale=scale, n_prev=n_prev, seed=12)
            R.check_sample(hip, "cuda", lg, prev, u[:rows].clone(), **dict(kw, eos_id=int(lg[0].argmax())))


def test_sample_finished_rows_and_reproducibility(hip):
    lg, prev = R.make_case(5, 32001, scale=4.0, n_prev=300, seed=5)
    lg_d, prev_d, u = R.on_device(lg, "cuda"), prev.cuda(), R.u_values()[3:8].cuda()
    outs = []
    for _ in range(2):
        unf = torch.tensor([1, 0, 1, 1, 0], dtype=torch.int32).cuda()
        out = torch.full((5,), -1, dtype=torch.int32).cuda()
        aux = torch.zeros(5, 4).cuda()
        hip.select_tokens(lg_d, out, prev=prev_d, n_prev=300, penalty=1.5, eos_id=2, pad_id=9, sample=True, temperature=0.7, top_p=0.9, u=u, unfinished=unf, aux=aux)
        assert int(out[1]) == 9 and int(out[4]) == 9 and unf.tolist() == [1, 0, 1, 1, 0]
        outs.append((out.cpu(), aux.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "a launch is bit-reproducible"


@pytest.mark.parametrize("V", VOCABS)
def test_beam_candidates(hip, V):
    for rows in (1, 5, 17):
        bs = torch.tensor([0.0, -0.3, -1.1, -2.0, -1e9] * 4)[:rows]
        for k in (1, 6, 10, 32):
            if k > V:
                continue
            for n_prev, pen, sup in ((0, 1.0, False), (300, 1.5, True), (1, 1.5, True)):
                lg, prev = R.make_case(rows, V, scale=4.0, n_prev=n_prev, seed=k)
                R.check_beam(hip, "cuda", lg, prev, bs, k, n_prev=n_prev, penalty=pen, suppress_eos=sup, eos_id=int(lg[0].argmax()))
        if V >= 10:
            lg, prev = R.make_case(rows, V, scale=1.0, n_prev=300, seed=2, max_at=V - 1)
            R.check_beam(hip, "cuda", lg, prev, torch.linspace(0, -3, rows), 10, n_prev=300, penalty=1.5)


def test_unsupported_vocabulary_raises(hip):
    lg = torch.zeros(1, 160 * 1024 // 4, device="cuda")
    with pytest.raises(RuntimeError, match="LDS"):
        hip.select_tokens(lg, torch.zeros(1, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="LDS"):
        hip.beam_candidates(lg, torch.zeros(1, device="cuda"), 4)


# ---- generate(selection="device") on the device ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def decoder():
    from stllm_amd import synth
    from stllm_amd.models.st_llm import STLLMForCausalLM, StllmConfig
    m = STLLMForCausalLM(StllmConfig(num_hidden_layers=2), device="cuda")
    synth.fill_module_(m, 0, "")
    with torch.no_grad():
        m.lm_head.weight.mul_(20.0)                                # a livelier next-token distribution than N(0, 0.02) weights give
    return m


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_generate_device_matches_torch_selection(hip, decoder, mode):
    """Greedy: both paths read the same logits and the penalty is one fp32 operation on either side, so the ids are equal whatever the gaps.  Beams: the
    kernel's log-softmax and torch's differ by fp32 rounding, which can only reorder candidates tied to ~1e-6; seed 0 has no such tie (a seed that puts a
    top-2 gap under 1e-4 would be replaced, and said so here)."""
    from stllm_amd import runtime
    emb = torch.randn(2, 12, 4096, generator=torch.Generator().manual_seed(0)).cuda() * 0.05
    with runtime.use_dtype(mode):
        kw = dict(max_new_tokens=8, repetition_penalty=1.5, min_length=2)
        want = decoder.generate(inputs_embeds=emb, **kw)
        for K in (1, 4):
            got = decoder.generate(inputs_embeds=emb, selection="device", sync_every=K, **kw)
            assert got.dtype == torch.long and torch.equal(got, want), (K, got, want)
        assert torch.equal(decoder.generate(inputs_embeds=emb[1:], selection="device", **kw), decoder.generate(inputs_embeds=emb[1:], **kw)), \
            "one row: the ids column is a one-element view"
        kw = dict(max_new_tokens=6, repetition_penalty=1.5, min_length=2, num_beams=5)
        want = decoder.generate(inputs_embeds=emb[:1], **kw)
        got = decoder.generate(inputs_embeds=emb[:1], selection="device", **kw)
        assert torch.equal(got, want), (got, want)
        kw = dict(max_new_tokens=6, do_sample=True, top_p=0.9, temperature=0.8, repetition_penalty=1.5, selection="device")
        a = decoder.generate(inputs_embeds=emb, generator=torch.Generator(device="cuda").manual_seed(5), **kw)
        b = decoder.generate(inputs_embeds=emb, generator=torch.Generator(device="cuda").manual_seed(5), **kw)
        assert torch.equal(a, b), "a sampled run reproduces under its seed"
