"""GPU: int4 weight-only decode (W4A16, group-scaled) — the kernels of stllm_gemv_q4 against fp64 of the quantised contract in the decode regime, the
int4 decode step against a re-prefill by a model whose weights are q * scale, generate() under runtime.use_decode_weights("int4g128") against the 16-bit
decode of that model, and the (reported, not gated) deviation of int4 from 16-bit weights."""
import pytest
import torch

from _util import T
from test_q4_cpu import _expected_kernel, deq, q4_case, q4_fused_norm_case

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
@pytest.mark.parametrize("N,K", [(4096, 4096), (256, 11008), (1536, 640)])
def test_gemv_q4_decode_regime(hip, dtype, M, N, K, mfma):
    """the parametrisation and the checks of test_gemv_w8_decode_regime over 4-bit weights: STORE f32 with bias, RESID, strided rows, SWIGLU, ROPE against
    fp64 of sum_g scale (A_g @ q_g^T) + bias at ACC_TOL / OUT_TOL, the expected kernel, weights and scales unchanged.  Where the VALU kernel's staged rows
    do not fit the LDS (M = 8, K = 11008 with gemv_mfma = 0) the call must refuse: there is no other 4-bit kernel to run."""
    want = _expected_kernel(M, K, mfma)
    assert (want is None) == ((M, K, mfma) == (8, 11008, 0))
    hip.set_option("gemv_mfma", mfma)
    try:
        q4_case(hip, dtype, M, N, K, want, dev=dev)
    finally:
        hip.set_option("gemv_mfma", -1)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("M", [1, 2])
def test_gemv_q4_fused_rmsnorm_operand(hip, dtype, M):
    q4_fused_norm_case(hip, dtype, M, 1024, 4096, dev=dev)
    with pytest.raises(RuntimeError, match="no kernel for M="):
        from stllm_amd import pack
        qp, s = pack.quant4_groups(T("q4.wbig", (128, 4096), 0.05).cuda().to(hip.torch_dtype(dtype)))
        hip.gemv_q4(None, qp, s, dtype=dtype, a_norm=(T("q4.nx9", (9, 4096), 1.0).cuda(), torch.ones(4096, device="cuda"), 1e-6))


def _model(layers=3):
    from stllm_amd import synth
    from stllm_amd.models.st_llm import STLLMForCausalLM, StllmConfig
    m = STLLMForCausalLM(StllmConfig(num_hidden_layers=layers), device="cuda")
    synth.fill_module_(m, 0, "")
    return m


def _dequantised_model(layers, dt):
    """the same synthetic model with its decoder Linear weights replaced by q * scale of the 4-bit format (quantising the original rows commutes with the
    packers' row orders)"""
    from stllm_amd import pack
    m = _model(layers)
    for l in m.model.layers:
        for lin in (l.self_attn.q_proj, l.self_attn.k_proj, l.self_attn.v_proj, l.self_attn.o_proj, l.mlp.gate_proj, l.mlp.up_proj, l.mlp.down_proj):
            lin.weight.copy_(deq(*pack.quant4_groups(lin.weight.to(dt))).float())
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


class _Spy:
    """hip.gemv_q4 wrapped: the kernel every call launched"""

    def __init__(self, hip):
        self.hip, self.orig, self.seen = hip, hip.gemv_q4, []

    def __enter__(self):
        def spy(*a, **k):
            r = self.orig(*a, **k)
            self.seen.append(self.hip.lib().stllm_last_kernel().decode())
            return r
        self.hip.gemv_q4 = spy
        return self.seen

    def __exit__(self, *exc):
        self.hip.gemv_q4 = self.orig


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_q4_decode_matches_dequantised_model(hip, mode):
    """the recipe of test_w8_decode_matches_dequantised_model (3 layers, full width, B = 2, S = 37, 4 new tokens) on the copy of the model whose decoder
    Linear weights are q * scale: the logits of its int4 decode steps against its own prefill over the extended sequence, so that every path computes the
    same math.  Re-quantising q * scale rounded to 16 bits gives (qp, scale) back — the group maximum is +-7 scale, which rounds back to amax, and
    |q| 2^-8 < 1/2 — so the 4-bit copy is the one of the original model: asserted.  Bounds, those of the int8 twin (the same comparison): bf16 5e-2 x scale;
    fp16 the larger of 1e-2 x scale and the deviation of the 16-bit fp16 decode from the same re-prefill."""
    from stllm_amd import pack, runtime
    B, S, n_new = 2, 37, 4
    emb = T("input.inputs_embeds", (B, S, 4096), 0.05).cuda()
    with runtime.use_dtype(mode):
        dt = runtime.compute_dtype()
        deq_m = _dequantised_model(3, dt)
        new_emb = deq_m.model.embed_tokens(torch.tensor([[5, 9, 1234, 77], [31000, 8, 4, 2]]))
        with _Spy(hip) as seen:
            with runtime.use_decode_weights("int4g128"):
                got = _decode_logits(deq_m, emb, new_emb)
                w_orig = _model(3).model.layers[2].mlp.down_proj.weight
                q0, s0 = pack.quant4_groups(w_orig.to(dt))
                q1, s1 = deq_m.model.pack_q4(dt)[2]["wdown"]
                assert torch.equal(q0, q1) and torch.equal(s0, s1), "re-quantising q * scale must give the 4-bit weights of the original model"
                del w_orig
        assert len(seen) == n_new * 3 * 4 and all(s.startswith("gemv_q4_kernel<") for s in seen), seen[:4]
        full = deq_m(samples=None, inputs_embeds=torch.cat([emb, new_emb], dim=1)).logits.float()
        same16 = _decode_logits(deq_m, emb, new_emb)      # the unquantised 16-bit decode of the same math
    scale = float(full.abs().max())
    err4 = max(float((g - full[:, S + t]).abs().max()) for t, g in enumerate(got))
    err16 = max(float((g - full[:, S + t]).abs().max()) for t, g in enumerate(same16))
    print(f"q4 decode vs re-prefill of the q*scale model [{mode}]: int4 {err4 / scale:.3e} x scale, 16-bit decode {err16 / scale:.3e} x scale (scale {scale:.3f}); last kernel {seen[-1]}")
    bound = 5e-2 * scale if mode == "bf16" else max(1e-2 * scale, err16)
    assert err4 <= bound, f"{mode}: {err4:.3e} > {bound:.3e} (scale {scale:.3f}, 16-bit decode {err16:.3e})"


@pytest.fixture(scope="module")
def gen_model():
    return _dequantised_model(2, torch.float16)


@pytest.mark.parametrize("path", ["greedy", "5 beams", "ragged", "share_prefix"])
def test_q4_generate_paths(hip, gen_model, path):
    """generate() under "int4g128" on the model whose weights are q * scale (so its 4-bit copy stands for exactly its 16-bit weights): the q4 kernels ran
    — the VALU kernel for 1-2 rows, the matrix-core kernel for 5 beams — and the ids equal those of the same model decoded in 16 bits under the same
    settings.  fp16: products a * w of the 16-bit step and scale * sum(a * q) of the 4-bit step differ only in fp32 rounding."""
    from stllm_amd import runtime
    model = gen_model
    emb = T("input.inputs_embeds", (1, 21, 4096), 0.05).cuda()
    emb2 = T("q4.emb2", (2, 12, 4096), 0.05).cuda()
    mask2 = torch.tensor([[1] * 12, [1] * 8 + [0] * 4]).cuda()
    with runtime.use_dtype("fp16"):
        prefix = model.model.new_cache(1, 12, "cuda")
        model.model.prefill(emb[:, :12], None, cache=prefix)
        run = {"greedy": lambda: model.generate(inputs_embeds=emb, max_new_tokens=6),
               "5 beams": lambda: model.generate(inputs_embeds=emb, max_new_tokens=6, num_beams=5),
               "ragged": lambda: model.generate(inputs_embeds=emb2, attention_mask=mask2, max_new_tokens=5, batching="ragged"),
               "share_prefix": lambda: model.generate(inputs_embeds=emb[:, 12:], prefix_cache=prefix, max_new_tokens=6, num_beams=5, share_prefix=True)}[path]
        with _Spy(hip) as seen:
            want = run()
            assert seen == [], "mode off: no 4-bit launch"
            with runtime.use_decode_weights("int4g128"):
                got = run()
            kernels = list(seen)
            again = run()
        assert len(seen) == len(kernels) and model.model._quant is None, "mode off again: no launch, the 4-bit copy freed by the next decode step"
    assert len(kernels) > 0 and len(kernels) % 8 == 0, len(kernels)           # 2 layers x 4 projections per decode step
    fam = "gemv_q4_mfma_kernel<f16_t" if path in ("5 beams", "share_prefix") else "gemv_q4_kernel<f16_t"
    assert all(k.startswith(fam) for k in kernels), (path, sorted(set(kernels)))
    print(f"q4 generate [{path}]: {len(kernels)} gemv_q4 launches, ids {got.flatten().tolist()}")
    assert int(got.min()) >= 0 and int(got.max()) < 32000
    assert torch.equal(got, want), (path, got.tolist(), want.tolist())
    assert torch.equal(again, want)


def test_q4_quantisation_deviation_report(hip):
    """NOT gated (synthetic Gaussian weights say nothing about a trained checkpoint): max-abs deviation and top-1 agreement of the int4 decode logits against
    the 16-bit decode of the same, unquantised model, per mode; printed.  Finiteness only is asserted."""
    from stllm_amd import runtime
    model = _model(3)
    B, S, n_new = 2, 37, 8
    emb = T("input.inputs_embeds", (B, S, 4096), 0.05).cuda()
    new_emb = model.model.embed_tokens(torch.tensor([[5, 9, 1234, 77, 12, 400, 9000, 3], [31000, 8, 4, 2, 77, 1, 50, 600]]))
    for mode in ("bf16", "fp16"):
        with runtime.use_dtype(mode):
            ref = _decode_logits(model, emb, new_emb)
            with runtime.use_decode_weights("int4g128"):
                got = _decode_logits(model, emb, new_emb)
        scale = max(float(r.abs().max()) for r in ref)
        dev_ = max(float((g - r).abs().max()) for g, r in zip(got, ref))
        agree = sum(int((g.argmax(-1) == r.argmax(-1)).sum()) for g, r in zip(got, ref))
        print(f"{mode}: int4g128 vs 16-bit decode logits, 3 layers, B=2, {n_new} steps: max-abs {dev_:.4e} ({dev_ / scale:.3e} x logits abs-max {scale:.3f}); "
              f"top-1 agreement {agree}/{B * n_new}")
        assert all(bool(torch.isfinite(g).all()) for g in got)
