"""GPU: int8 weight-only decode (W8A16) — the kernels of stllm_gemv_w8 against fp64 of the quantised contract in the decode regime, the int8
decode step against a re-prefill by a model whose weights are q * scale, generate() under runtime.use_decode_weights("int8"), and the (reported,
not gated) deviation of int8 from 16-bit weights."""
import os

import pytest
import torch

from _util import T
from test_w8_cpu import _expected_kernel, w8_case, w8_fused_norm_case

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def hip():
    from stllm_amd import hip as h
    h.lib()
    return h


def dev(t):
    return t.cuda()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("M,mfma", [(1, -1), (2, -1), (3, -1), (4, -1), (5, -1), (8, -1), (12, -1), (16, -1), (3, 0), (5, 0), (8, 0), (1, 1), (2, 1)])
@pytest.mark.parametrize("N,K", [(4096, 4096), (256, 11008), (1536, 704)])
def test_gemv_w8_decode_regime(hip, dtype, M, N, K, mfma):
    """the parametrisation and the checks of test_gemv_decode_regime over int8 weights: STORE f32 with bias, RESID, strided rows, SWIGLU, ROPE against
    fp64 of scale * (A @ q^T) + bias at ACC_TOL / OUT_TOL, the expected kernel, weights and scales unchanged.  Where the VALU kernel's staged rows
    do not fit the LDS (M = 8, K = 11008 with gemv_mfma = 0) the call must refuse: there is no other int8 kernel to run."""
    hip.set_option("gemv_mfma", mfma)
    try:
        w8_case(hip, dtype, M, N, K, _expected_kernel(M, K, mfma), dev=dev)
    finally:
        hip.set_option("gemv_mfma", -1)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("M", [1, 2])
def test_gemv_w8_fused_rmsnorm_operand(hip, dtype, M):
    w8_fused_norm_case(hip, dtype, M, 1024, 4096, dev=dev)
    with pytest.raises(RuntimeError, match="no kernel for M="):
        from stllm_amd import pack
        q, s = pack.quant8_rows(T("w8.wbig", (128, 4096), 0.05).cuda().to(hip.torch_dtype(dtype)))
        hip.gemv_w8(None, q, s, dtype=dtype, a_norm=(T("w8.nx9", (9, 4096), 1.0).cuda(), torch.ones(4096, device="cuda"), 1e-6))


def _model(layers=3):
    from stllm_amd import synth
    from stllm_amd.models.st_llm import STLLMForCausalLM, StllmConfig
    m = STLLMForCausalLM(StllmConfig(num_hidden_layers=layers), device="cuda")
    synth.fill_module_(m, 0, "")
    return m


def _dequantised_model(layers, dt):
    """the same synthetic model with its decoder Linear weights replaced by q * scale of the int8 format (quantising the original rows commutes with the
    packers' row orders)"""
    from stllm_amd import pack
    m = _model(layers)
    for l in m.model.layers:
        for lin in (l.self_attn.q_proj, l.self_attn.k_proj, l.self_attn.v_proj, l.self_attn.o_proj, l.mlp.gate_proj, l.mlp.up_proj, l.mlp.down_proj):
            q, s = pack.quant8_rows(lin.weight.to(dt))
            lin.weight.copy_(q.float() * s[:, None])
    return m


def _decode_logits(model, emb, new_emb):
    lm = model.model
    B, S = emb.shape[:2]
    cache = lm.new_cache(B, S + new_emb.shape[1], "cuda")
    lm.prefill(emb, None, cache=cache)
    out = []
    for t in range(new_emb.shape[1]):
        _, h16 = lm.decode_step(new_emb[:, t:t + 1], cache)
        out.append(model.logits_from(h16, B, 1)[:, 0].float().clone())
    return out


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_w8_decode_matches_dequantised_model(hip, mode):
    """follows test_kv_cache_decode_matches_reprefill (3 layers, full width, B = 2, S = 37, 4 new tokens) on the copy of the model whose decoder Linear
    weights are q * scale: the logits of its int8 decode steps against its own prefill over the extended sequence.  Every path then computes the same
    math — the prefill that fills the cache included, which always runs on the 16-bit weights: on the unquantised model it would put the quantisation
    error of 37 prefilled positions (measured 2.8e-2 x scale in fp16) into a comparison that is about the decode kernels.  Quantising q * scale rounded to
    16 bits gives q and scale back (|q| 2^-8 < 1/2), so the int8 copy is the one of the original model: asserted.  bf16: 5e-2 x scale, the project's bound
    for this comparison; fp16: the larger of 1e-2 x scale and the deviation of the 16-bit fp16 decode from the same re-prefill (the quantised path must
    be no worse than the unquantised one against an independent computation of the same math)."""
    from stllm_amd import pack, runtime
    B, S, n_new = 2, 37, 4
    emb = T("input.inputs_embeds", (B, S, 4096), 0.05).cuda()
    with runtime.use_dtype(mode):
        dt = runtime.compute_dtype()
        deq = _dequantised_model(3, dt)
        new_emb = deq.model.embed_tokens(torch.tensor([[5, 9, 1234, 77], [31000, 8, 4, 2]]))
        seen = []
        orig = hip.gemv_w8

        def spy(*a, **k):
            r = orig(*a, **k)
            seen.append(hip.lib().stllm_last_kernel().decode())
            return r
        hip.gemv_w8 = spy
        try:
            with runtime.use_decode_weights("int8"):
                got = _decode_logits(deq, emb, new_emb)
                w_orig = _model(3).model.layers[2].mlp.down_proj.weight
                q0, s0 = pack.quant8_rows(w_orig.to(dt))
                q1, s1 = deq.model.pack_w8(dt)[2]["wdown"]
                assert torch.equal(q0, q1) and torch.equal(s0, s1), "re-quantising q * scale must give the int8 weights of the original model"
                del w_orig
        finally:
            hip.gemv_w8 = orig
        assert len(seen) == n_new * 3 * 4 and all(s.startswith("gemv_w8_kernel<") for s in seen), seen[:4]
        ran = seen[-1]
        full = deq(samples=None, inputs_embeds=torch.cat([emb, new_emb], dim=1)).logits.float()
        same16 = _decode_logits(deq, emb, new_emb)      # the unquantised 16-bit decode of the same math
    scale = float(full.abs().max())
    err8 = max(float((g - full[:, S + t]).abs().max()) for t, g in enumerate(got))
    err16 = max(float((g - full[:, S + t]).abs().max()) for t, g in enumerate(same16))
    print(f"w8 decode vs re-prefill of the q*scale model [{mode}]: int8 {err8 / scale:.3e} x scale, 16-bit decode {err16 / scale:.3e} x scale (scale {scale:.3f}); last kernel {ran}")
    bound = 5e-2 * scale if mode == "bf16" else max(1e-2 * scale, err16)
    assert err8 <= bound, f"{mode}: {err8:.3e} > {bound:.3e} (scale {scale:.3f}, 16-bit decode {err16:.3e})"


def test_w8_generate_paths(hip):
    """greedy, top-p with a fixed seed, 5 beams, a padded batch of 3 and a prompt behind a prefix cache: under "int8" every path completes with ids in
    range and ITS decode steps ran on the w8 kernels (hip.gemv_w8 is wrapped: calls counted per path, the kernel each one launched recorded); with the mode
    off again no call is made and the ids are those of the run before it was switched on"""
    from stllm_amd import runtime
    model = _model(2)
    emb = T("input.inputs_embeds", (1, 21, 4096), 0.05).cuda()
    emb3 = T("w8.emb3", (3, 12, 4096), 0.05).cuda()
    mask3 = torch.tensor([[1] * 12, [1] * 9 + [0] * 3, [1] * 12])
    seen = []
    orig = hip.gemv_w8

    def spy(*a, **k):
        r = orig(*a, **k)
        seen.append(hip.lib().stllm_last_kernel().decode())
        return r

    def runs():
        """[(ids, kernels of the gemv_w8 calls of that path)]"""
        g = torch.Generator(device="cuda").manual_seed(11)
        prefix = model.model.new_cache(1, 12, "cuda")
        model.model.prefill(emb[:, :12], None, cache=prefix)
        paths = [lambda: model.generate(inputs_embeds=emb, max_new_tokens=6),
                 lambda: model.generate(inputs_embeds=emb, max_new_tokens=6, do_sample=True, top_p=0.9, generator=g),
                 lambda: model.generate(inputs_embeds=emb, max_new_tokens=6, num_beams=5),
                 lambda: model.generate(inputs_embeds=emb3, attention_mask=mask3.cuda(), max_new_tokens=5),
                 lambda: model.generate(inputs_embeds=emb[:, 12:], prefix_cache=prefix, max_new_tokens=6)]
        out = []
        for f in paths:
            del seen[:]
            ids = f()
            out.append((ids, list(seen)))
        return out
    hip.gemv_w8 = spy
    try:
        with runtime.use_dtype("bf16"):
            before = runs()
            with runtime.use_decode_weights("int8"):
                on = runs()
            after = runs()
    finally:
        hip.gemv_w8 = orig
    names = ["greedy", "top-p", "5 beams", "padded batch of 3", "prefix cache"]
    for name, (ids, kernels) in zip(names, on):
        assert ids.numel() > 0 and int(ids.min()) >= 0 and int(ids.max()) < 32000, name
        assert len(kernels) > 0 and len(kernels) % 8 == 0, (name, len(kernels))           # 2 layers x 4 projections per decode step
        want = "gemv_w8_mfma_kernel<bf16_t" if name == "5 beams" else "gemv_w8_kernel<bf16_t"   # 5 rows: matrix cores; 1-2 rows: the VALU kernel
        assert all(k.startswith(want) for k in kernels), (name, sorted(set(kernels)))
        print(f"w8 generate [{name}]: {len(kernels)} gemv_w8 launches, ids {ids.flatten().tolist()}")
    assert on[0][0].shape == (1, 6) and on[3][0].shape[0] == 3 and on[4][0].shape[0] == 1
    assert all(k == [] for _, k in before) and all(k == [] for _, k in after), "mode off: no int8 launch"
    assert model.model._quant is None, "mode off: the int8 copy is freed by the next decode step"
    assert all(torch.equal(a[0], b[0]) for a, b in zip(before, after)), "mode off again: the ids of the run before it was switched on"


def test_w8_quantisation_deviation_report(hip):
    """NOT gated (synthetic Gaussian weights are not Vicuna, nobody has measured the real model): max-abs deviation and top-1 agreement of the int8 decode
    logits against the 16-bit decode of the same model, per mode; printed, and written to the file STLLM_W8_REPORT names"""
    from stllm_amd import runtime
    model = _model(3)
    B, S, n_new = 2, 37, 8
    emb = T("input.inputs_embeds", (B, S, 4096), 0.05).cuda()
    new_emb = model.model.embed_tokens(torch.tensor([[5, 9, 1234, 77, 12, 400, 9000, 3], [31000, 8, 4, 2, 77, 1, 50, 600]]))
    lines = []
    for mode in ("bf16", "fp16"):
        with runtime.use_dtype(mode):
            ref = _decode_logits(model, emb, new_emb)
            with runtime.use_decode_weights("int8"):
                got = _decode_logits(model, emb, new_emb)
        scale = max(float(r.abs().max()) for r in ref)
        dev_ = max(float((g - r).abs().max()) for g, r in zip(got, ref))
        agree = sum(int((g.argmax(-1) == r.argmax(-1)).sum()) for g, r in zip(got, ref))
        lines.append(f"{mode}: int8 vs 16-bit decode logits, 3 layers, B=2, {n_new} steps: max-abs {dev_:.4e} ({dev_ / scale:.3e} x logits abs-max {scale:.3f}); "
                     f"top-1 agreement {agree}/{B * n_new}")
        assert all(bool(torch.isfinite(g).all()) for g in got)
    print("\n".join(lines))
    if os.environ.get("STLLM_W8_REPORT"):
        with open(os.environ["STLLM_W8_REPORT"], "w") as f:
            f.write("\n".join(lines) + "\n")
