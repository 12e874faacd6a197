"""CPU: int8 weight-only decode (W8A16) — the quantiser (pack.quant8_rows), the kernels of stllm_gemv_w8 on the host emulator (tests/hipemu)
against fp64 of the contract, LlamaModel.decode_step / generate under runtime.use_decode_weights("int8") on the test-only contract backend
(tests/_cpu_backend.py), and the C ABI surface."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _cpu_backend as CB
import _hipemu
from _util import T, decode_run, small_llama
from test_kernels_gpu import ACC_TOL, OUT_TOL   # the 16-bit GEMV's error model: the products a * q are exact

torch.set_grad_enabled(False)
TOL = 2e-4   # x logits abs-max: tests/test_prefix_cache_cpu.py::test_extend_then_decode_matches_token_by_token_forward
SMALL = dict(num_hidden_layers=2, hidden_size=256, intermediate_size=704, num_attention_heads=2, vocab_size=512)
W8_KEYS = ("wqkv", "wo", "wgu", "wdown")


# ---- quantiser ------------------------------------------------------------------------------------------------------------------
def _numpy_recipe(w):
    """the recipe of the quantised format restated with numpy: amax / 127 in fp32, 1 for a zero row; rint (half-even) of the fp64 quotient, clamp"""
    w = w.float().numpy().astype(np.float32)
    amax = np.abs(w).max(axis=1).astype(np.float32)
    scale = np.where(amax > 0, (amax / np.float32(127.0)).astype(np.float32), np.float32(1.0)).astype(np.float32)
    q = np.clip(np.rint(w.astype(np.float64) / scale.astype(np.float64)[:, None]), -127, 127).astype(np.int8)
    return q, scale


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_quant8_rows_recipe_and_bound(dtype):
    from stllm_amd import pack
    w = T("w8.q.w", (192, 704), 0.05)
    w[3] = 0.0                                   # a row of zeros
    w[7, 100] = 9.0                              # a row with one outlier
    w = w.to(dtype)
    q, scale = pack.quant8_rows(w)
    assert q.dtype == torch.int8 and q.is_contiguous() and q.shape == w.shape and scale.dtype == torch.float32 and scale.shape == (192,)
    assert int(q.min()) >= -127 and int(q.max()) <= 127 and bool((scale > 0).all())
    assert float(scale[3]) == 1.0 and int(q[3].abs().max()) == 0
    assert int(q[7, 100]) == 127 and int(q[7].abs().sort().values[-2]) <= 3
    err = (w.double() - q.double() * scale.double()[:, None]).abs()
    bound = scale.double()[:, None] / 2 * (1 + 2.0 ** -20)
    print("quant8_rows: max |w - q scale| / (scale / 2) =", float((err / (scale.double()[:, None] / 2)).max()))
    assert bool((err <= bound).all())
    qn, sn = _numpy_recipe(w)
    assert np.array_equal(q.numpy(), qn) and np.array_equal(scale.numpy().view(np.uint32), sn.view(np.uint32))


def test_quant8_rows_commutes_with_the_packed_row_orders():
    from stllm_amd import pack
    dt = torch.bfloat16
    wq, wk, wv = T("w8.wq", (256, 256), 0.05), T("w8.wk", (256, 256), 0.05), T("w8.wv", (256, 256), 0.05)
    q, s = pack.quant8_rows(pack.llama_qkv(wq, wk, wv, dt, n_heads=2))
    perm = pack.rope_head_perm(2)
    parts = [pack.quant8_rows(x.to(dt)) for x in (wq, wk, wv)]
    assert torch.equal(q, torch.cat((parts[0][0][perm], parts[1][0][perm], parts[2][0])))
    assert torch.equal(s, torch.cat((parts[0][1][perm], parts[1][1][perm], parts[2][1])))
    wg, wu = T("w8.wg", (704, 256), 0.05), T("w8.wu", (704, 256), 0.05)
    q, s = pack.quant8_rows(pack.llama_gate_up(wg, wu, dt))
    (qg, sg), (qu, su) = pack.quant8_rows(wg.to(dt)), pack.quant8_rows(wu.to(dt))
    assert torch.equal(q.view(22, 2, 32, 256)[:, 0].reshape(704, 256), qg) and torch.equal(q.view(22, 2, 32, 256)[:, 1].reshape(704, 256), qu)
    assert torch.equal(s.view(22, 2, 32)[:, 0].reshape(-1), sg) and torch.equal(s.view(22, 2, 32)[:, 1].reshape(-1), su)


# ---- kernels on the host emulator -----------------------------------------------------------------------------------------------
def _expected_kernel(M, K, mfma):
    """stllm_gemv_w8's choice: the matrix-core kernel from M = 3 (option 1: from M = 1; 0: never), else the VALU kernel for M <= 8"""
    if mfma != 0 and M >= (1 if mfma == 1 else 3) and K % 64 == 0:
        return "gemv_w8_mfma_kernel<"
    mr = M if M <= 2 else (M + 1) // 2 * 2
    return f"gemv_w8_kernel<MR{mr}" if M <= 8 and mr * K * 2 <= 150 * 1024 else None


def _ran(hip, want, what):
    name = hip.lib().stllm_last_kernel().decode()
    if want.startswith("gemv_w8_kernel<MR"):
        assert name.startswith("gemv_w8_kernel<") and name.endswith("," + want[len("gemv_w8_kernel<MR"):] + ">"), (what, name, want)
    else:
        assert name.startswith(want), (what, name, want)
    return name


def _check(got, ref, tol, what):
    got, ref = got.detach().double().cpu(), ref.double()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), what
    scale = max(float(ref.abs().max()), 1e-6)
    err = float((got - ref).abs().max())
    assert err <= tol * scale, f"{what}: max err {err:.3e} > {tol:.1e} * {scale:.3e}"


def rope_ref(acc, cos, sin, rope_seq, rope_cols):
    """the ROPE epilogue in the packed layout, fp64: inside every 64-column group the partners are (c, c + 32); group g uses the table columns
    32 (g % 2) + c; columns >= rope_cols pass through"""
    M, N = acc.shape
    x = acc.view(M, N // 64, 2, 32).clone()
    for g in range(N // 64):
        if g * 64 >= rope_cols:
            continue
        for m in range(M):
            c = cos[m % rope_seq, 32 * (g % 2):32 * (g % 2) + 32].double()
            s = sin[m % rope_seq, 32 * (g % 2):32 * (g % 2) + 32].double()
            a, b = acc.view(M, N // 64, 2, 32)[m, g, 0], acc.view(M, N // 64, 2, 32)[m, g, 1]
            x[m, g, 0], x[m, g, 1] = a * c - b * s, b * c + a * s
    return x.reshape(M, N)


def w8_case(hip, dtype, M, N, K, want, dev=lambda t: t, full=True):
    """every epilogue of stllm_gemv_w8 against fp64 of its contract on the int8 values and scales actually passed (shared with tests/test_w8_gpu.py)"""
    from stllm_amd import pack
    td = hip.torch_dtype(dtype)
    a = T("w8.a", (M, K), 0.5).to(td)
    q, scale = pack.quant8_rows(T("w8.w", (N, K), 0.05).to(td))
    b = T("w8.b", (N,), 0.5)
    a64, q64, s64 = a.double(), q.double(), scale.double()
    ref = (a64 @ q64.t()) * s64 + b.double()
    import _poison
    # a leading dimension larger than K with NaN in the columns [K, lda): never read (include/stllm_hip.h: memory regions)
    ad, qd, sd, bd = _poison.nan_padded(dev(a)), dev(q), dev(scale), dev(b)
    q0, s0 = qd.clone(), sd.clone()
    if want is None:
        with pytest.raises(RuntimeError, match="no kernel for M="):
            hip.gemv_w8(ad, qd, sd, dtype=dtype, out_f32=True)
        return
    g32 = _poison.Guarded(M, N, torch.float32, device=ad.device)     # the output inside a 0xFF-filled buffer: rows around it, columns [N, ldo)
    out = hip.gemv_w8(ad, qd, sd, dtype=dtype, bias=bd, out_f32=True, out=g32.out)
    _ran(hip, want, "store f32")
    _check(out, ref, ACC_TOL[dtype], "w8 store f32")
    assert g32.intact(), "w8 store f32: a byte outside the M x N output was written"
    x = T("w8.x", (M, N), 2.0)
    xd = _poison.nan_padded(dev(x.clone()))                          # resid columns [N, ldr): NaN, never read, never written
    hip.gemv_w8(ad, qd, sd, dtype=dtype, epilogue=hip.EPI_RESID, bias=bd, resid=xd)
    _check(xd, x.double() + ref, ACC_TOL[dtype], "w8 resid")
    assert bool(torch.isnan(torch.as_strided(xd, (M, 8), (xd.stride(0), 1), xd.storage_offset() + N)).all()), "w8 resid: the columns [N, ldr) were written"
    g16 = _poison.Guarded(M, N, td, device=ad.device)
    o16 = hip.gemv_w8(ad, qd, sd, dtype=dtype, bias=bd, out=g16.out)
    _check(o16, ref, OUT_TOL[dtype], "w8 store T")
    assert g16.intact(), "w8 store T: a byte outside the M x N output was written"
    buf = dev(torch.zeros((M, 3, N), dtype=td))       # output rows with a stride, untouched neighbours
    hip.gemv_w8(ad, qd, sd, dtype=dtype, out=buf[:, 1])
    _check(buf[:, 1], ref - b.double(), OUT_TOL[dtype], "w8 strided rows")
    assert float(buf[:, 0].abs().max()) == 0.0 and float(buf[:, 2].abs().max()) == 0.0
    if full:
        o = hip.gemv_w8(ad, qd, sd, dtype=dtype, epilogue=hip.EPI_SWIGLU)
        _ran(hip, want, "swiglu")
        g = (ref - b.double()).view(M, N // 64, 2, 32)
        _check(o, (F.silu(g[:, :, 0]) * g[:, :, 1]).reshape(M, N // 2), OUT_TOL[dtype], "w8 swiglu")
        cos, sin = pack.rope_tables(7)
        pos, rope_cols = 5, (N // 128 // 2) * 128 if N >= 256 else N      # the last columns stay unrotated where N allows
        o = hip.gemv_w8(ad, qd, sd, dtype=dtype, epilogue=hip.EPI_ROPE, rope=(dev(cos[pos:pos + 1].contiguous()), dev(sin[pos:pos + 1].contiguous())),
                        rope_seq=1, rope_cols=rope_cols)
        _ran(hip, want, "rope")
        _check(o, rope_ref(ref - b.double(), cos[pos:pos + 1], sin[pos:pos + 1], 1, rope_cols), OUT_TOL[dtype], "w8 rope")
    assert torch.equal(qd, q0) and torch.equal(sd, s0), "the weights and scales are read-only"


def w8_fused_norm_case(hip, dtype, M, I, K, dev=lambda t: t):
    """the fused RMSNorm operand: fp64 of RMSNorm rounded to the compute dtype, then the contract (the reference of test_gemv_fused_rmsnorm_operand)"""
    from stllm_amd import pack
    td = hip.torch_dtype(dtype)
    x = T("w8.nx", (M, K), 1.7)
    gamma = T("w8.ngamma", (K,), 0.2) + 1.0
    q, scale = pack.quant8_rows(pack.llama_gate_up(T("w8.wg", (I, K), 0.05), T("w8.wu", (I, K), 0.05), td))
    one = hip.gemv_w8(None, dev(q), dev(scale), dtype=dtype, epilogue=hip.EPI_SWIGLU, a_norm=(dev(x), dev(gamma), 1e-6))
    name = hip.lib().stllm_last_kernel().decode()
    assert name.startswith("gemv_w8_kernel<") and name.endswith(f",{M}>"), name
    x64 = x.double()
    hn = (gamma.double() * x64 * torch.rsqrt((x64 ** 2).mean(-1, keepdim=True) + 1e-6)).to(td).double()
    g = ((hn @ q.double().t()) * scale.double()).view(M, 2 * I // 64, 2, 32)
    _check(one, (F.silu(g[:, :, 0]) * g[:, :, 1]).reshape(M, I), OUT_TOL[dtype], "w8 fused rmsnorm swiglu vs fp64")


EMU_CASES = [(1, -1), (2, -1), (1, 1), (2, 1), (3, -1), (5, -1), (8, -1), (16, -1), (3, 0), (5, 0), (8, 0), (16, 0)]


@pytest.mark.skipif(not _hipemu.available() or _hipemu.ON_DEVICE, reason="host emulation of the kernel sources needs ROCm's clang++")
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("N,K", [(256, 704), (128, 1024)])
def test_gemv_w8_kernels_emulated(dtype, N, K):
    with _hipemu.emulated() as hip:
        try:
            for M, mfma in EMU_CASES:
                hip.set_option("gemv_mfma", mfma)
                w8_case(hip, dtype, M, N, K, _expected_kernel(M, K, mfma), full=(N == 256 or M in (1, 5)))
            hip.set_option("gemv_mfma", -1)
            for M in (1, 2):
                w8_fused_norm_case(hip, dtype, M, N // 2, K)
        finally:
            hip.set_option("gemv_mfma", -1)
        a = T("w8.a", (17, K), 0.5).to(hip.torch_dtype(dtype))
        q, s = torch.zeros((N, K), dtype=torch.int8), torch.ones(N)
        with pytest.raises(RuntimeError, match="decode regime"):
            hip.gemv_w8(a, q, s, dtype=dtype)
        with pytest.raises(RuntimeError, match="K %% 16|K % 16"):
            hip.gemv_w8(a[:1, :K - 8], q[:, :K - 8], s, dtype=dtype)


# ---- model ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    return small_llama(SMALL)


@pytest.fixture(scope="module")
def baseline(small):
    """decode logits of the 16-bit path before the int8 mode was ever switched on: no quantised entry point is reached"""
    from stllm_amd import runtime
    emb = T("w8.emb", (2, 12, 256), 0.05)
    with CB.installed(), runtime.use_dtype("bf16"):
        CB.CALLS_W8.clear(); CB.CALLS_Q4.clear()
        base16 = decode_run(small, emb, 8, 4)
        assert CB.CALLS_W8 == [] and CB.CALLS_Q4 == []
        return emb, base16


def test_int8_decode_equals_the_dequantised_model(small, baseline):
    from stllm_amd import pack, runtime
    emb, base16 = baseline
    lm = small.model
    with CB.installed(), runtime.use_dtype("bf16"):
        CB.CALLS_W8.clear(); CB.CALLS_Q4.clear()
        with runtime.use_decode_weights("int8"):
            got = decode_run(small, emb, 8, 4)
        assert len(CB.CALLS_W8) == 4 * 2 * 4 and all(c[1] == 2 for c in CB.CALLS_W8) and CB.CALLS_Q4 == []
        assert sum(c[4] for c in CB.CALLS_W8) == 4 * 2 * 2, "B = 2 <= FUSE_NORM_ROWS: the qkv and gate/up projections take the fused-norm form"
        assert runtime.decode_weights() is None

        def dequantise():   # the SAME 16-bit decode path over q * scale (fp32 tensors in place of the packed weights; the prefill before it used the originals)
            for pk in lm.pack(torch.bfloat16):
                for k in W8_KEYS:
                    q, s = pack.quant8_rows(pk[k])
                    pk[k] = q.float() * s[:, None]
        CB.CALLS_W8.clear()
        try:
            want = decode_run(small, emb, 8, 4, before_decode=dequantise)
        finally:
            lm.repack()
        assert CB.CALLS_W8 == []
        # mode None (the default): bit-identical to the run made before the mode was ever switched on
        again = decode_run(small, emb, 8, 4)
    scale = max(float(w.abs().max()) for w in want)
    for g, w in zip(got, want):
        assert float((g - w).abs().max()) <= TOL * scale, (float((g - w).abs().max()), scale)
    assert not any(torch.equal(g, b) for g, b in zip(got, base16)), "int8 weights must move the logits"
    assert all(torch.equal(a, b) for a, b in zip(again, base16))


def test_int8_weight_cache_follows_the_parameters_and_the_mode(small):
    """the int8 copy is keyed by the parameter fingerprint of the 16-bit pack (models/layers.py: `_version` + `data_ptr()`): an in-place edit of a master
    rebuilds both.  (The edit is `p.copy_` as in test_packed_weight_caches_follow_in_place_edits_of_the_masters: a write through `p.data` bypasses
    torch's version counter, for this cache as for the 16-bit one — such writers call repack().)"""
    from stllm_amd import runtime
    lm = small.model
    emb = T("w8.emb", (1, 6, 256), 0.05)
    w = lm.layers[1].mlp.down_proj.weight
    w0 = w.detach().clone()
    try:
        with CB.installed(), runtime.use_dtype("bf16"):
            runtime.set_decode_weights("int8")
            assert runtime.decode_weights() == "int8"
            a = decode_run(small, emb, 4, 2)
            assert lm._quant[:2] == ("int8", torch.bfloat16)
            first = lm._quant.layers
            assert set(first[0]) == set(W8_KEYS) and first[1]["wdown"][0].dtype == torch.int8 and first[1]["wdown"][1].shape == (256,)
            decode_run(small, emb, 4, 1)
            assert lm._quant[:2] == ("int8", torch.bfloat16) and lm._quant.layers is first, "unchanged parameters: the cached copy"
            w.copy_(w0 * 1.5)
            b = decode_run(small, emb, 4, 2)
            assert lm._quant[:2] == ("int8", torch.bfloat16)
            second = lm._quant.layers
            assert second is not first and not torch.equal(second[1]["wdown"][1], first[1]["wdown"][1])
            assert torch.equal(second[0]["wqkv"][0], first[0]["wqkv"][0]) and not torch.equal(a[-1], b[-1])
            runtime.set_decode_weights(None)
            decode_run(small, emb, 4, 1)
            assert lm._quant is None, "mode off: the int8 copy is freed"
            with pytest.raises(ValueError):
                runtime.set_decode_weights("int4")
    finally:
        runtime.set_decode_weights(None)
        w.copy_(w0)
        lm.repack()


def test_int8_rejects_the_modes_it_does_not_serve():
    from stllm_amd import runtime
    m = small_llama(SMALL)
    emb = T("w8.emb", (1, 6, 256), 0.05)
    with CB.installed(), runtime.use_decode_weights("int8"):
        with runtime.use_dtype("fp32"):
            c = m.model.new_cache(1, 8, "cpu")
            m.model.prefill(emb[:, :4], None, cache=c)
        for mode in ("fp32", "bf16x3", "mixed"):
            with runtime.use_dtype(mode), pytest.raises(NotImplementedError, match="16-bit compute mode"):
                m.model.decode_step(emb[:, 4:5], c)
        assert c.len == 4
        m.add_lora(8, 16)
        for i, mod in enumerate(m._lora_modules()):
            mod.B.copy_(T(f"w8.lora.B{i}", tuple(mod.B.shape), 0.02))
        with runtime.use_dtype("bf16"):
            with pytest.raises(NotImplementedError, match=r"merge_adapter\(\) first"):
                decode_run(m, emb, 4, 1)
            m.merge_adapter()
            CB.CALLS_W8.clear()
            decode_run(m, emb, 4, 1)
            assert len(CB.CALLS_W8) == 8


def test_generate_runs_through_the_int8_path(small):
    from stllm_amd import runtime
    emb = T("w8.gen", (1, 9, 256), 0.05)
    kw = dict(max_new_tokens=5, do_sample=False, min_length=5)
    with CB.installed(), runtime.use_dtype("bf16"):
        off = small.generate(inputs_embeds=emb, num_beams=5, **kw)
        prefix = small.model.new_cache(1, 5, "cpu")
        small.model.prefill(emb[:, :5], None, cache=prefix)
        before = [b.clone() for b in prefix.qkv]
        with runtime.use_decode_weights("int8"):
            CB.CALLS_W8.clear()
            ids = small.generate(inputs_embeds=emb[:, 5:], prefix_cache=prefix, num_beams=1, **kw)
            n1 = len(CB.CALLS_W8)
            assert ids.shape == (1, 5) and int(ids.min()) >= 0 and int(ids.max()) < 512
            assert n1 > 0 and n1 % 8 == 0 and all(c[1] == 1 and c[2:4] in ((768, 256), (256, 256), (1408, 256), (256, 704)) for c in CB.CALLS_W8)
            assert prefix.len == 5 and all(torch.equal(x, y) for x, y in zip(prefix.qkv, before))
            CB.CALLS_W8.clear()
            ids5 = small.generate(inputs_embeds=emb, num_beams=5, **kw)
            assert ids5.shape[0] == 1 and int(ids5.min()) >= 0 and int(ids5.max()) < 512
            assert len(CB.CALLS_W8) > 0 and len(CB.CALLS_W8) % 8 == 0 and all(c[1] == 5 and not c[4] for c in CB.CALLS_W8), "5 beams: 5 rows, norms not fused"
        CB.CALLS_W8.clear()
        assert torch.equal(small.generate(inputs_embeds=emb, num_beams=5, **kw), off) and CB.CALLS_W8 == []


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
def test_abi_declares_and_exports_gemv_w8():
    from stllm_amd import hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "stllm_hip.h")).read()
    assert "stllm_gemv_w8" in hip.EXPORTS and re.search(r"^int stllm_gemv_w8\(const stllm_gemv_w8_args\* args, void\* stream\);", header, re.M)
    assert re.search(r"\}\s*stllm_gemv_w8_args;", header)
    assert callable(hip.gemv_w8)
    if os.path.exists(hip.LIB_PATH):
        L = hip.lib()
        assert hasattr(L, "stllm_gemv_w8") and L.stllm_abi_version() == 7
