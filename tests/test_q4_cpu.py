"""CPU: int4 weight-only decode (W4A16, group-scaled) — the quantiser (pack.quant4_groups / dequant4_groups), the kernels of stllm_gemv_q4 on the host
emulator (tests/hipemu) against fp64 of the contract, LlamaModel.decode_step / generate under runtime.use_decode_weights("int4g128") on the test-only
contract backend (tests/_cpu_backend.py), and the C ABI surface."""
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
from test_w8_cpu import EMU_CASES, rope_ref

torch.set_grad_enabled(False)
TOL = 2e-4   # x logits abs-max: the bound of test_w8_cpu.py::test_int8_decode_equals_the_dequantised_model (same comparison, same backend)
SMALL = dict(num_hidden_layers=2, hidden_size=256, intermediate_size=768, num_attention_heads=2, vocab_size=512)   # both K are multiples of 128
Q4_KEYS = ("wqkv", "wo", "wgu", "wdown")


def deq(qp, scale):
    """the fp64 weight a (qp, scale) pair stands for, through pack.dequant4_groups"""
    from stllm_amd import pack
    q, s = pack.dequant4_groups(qp, scale)
    n, k = q.shape
    return (q.double().view(n, k // 128, 128) * s.double()[:, :, None]).reshape(n, k)


# ---- quantiser ------------------------------------------------------------------------------------------------------------------
def _numpy_recipe(w):
    """the recipe restated with numpy: per 128-group amax / 7 in fp32, 1 for a zero group; rint (half-even) of the fp64 quotient, clamp to [-7, 7]"""
    w = w.float().numpy().astype(np.float32)
    n, k = w.shape
    g = w.reshape(n, k // 128, 128)
    amax = np.abs(g).max(axis=2).astype(np.float32)
    scale = np.where(amax > 0, (amax / np.float32(7.0)).astype(np.float32), np.float32(1.0)).astype(np.float32)
    q = np.clip(np.rint(g.astype(np.float64) / scale.astype(np.float64)[:, :, None]), -7, 7).astype(np.int8)
    return q.reshape(n, k), scale


def _numpy_place(q):
    """the documented nibble placement, element by element: of the 8 elements of a little-endian dword, element 2 t -> bits [4 t, 4 t + 4), element
    2 t + 1 -> bits [16 + 4 t, 16 + 4 t + 4)"""
    n, k = q.shape
    u = (q.astype(np.int64) + 8).reshape(n, k // 8, 8)
    dw = np.zeros((n, k // 8), dtype=np.uint64)
    for t in range(4):
        dw |= (u[:, :, 2 * t].astype(np.uint64) << np.uint64(4 * t)) | (u[:, :, 2 * t + 1].astype(np.uint64) << np.uint64(16 + 4 * t))
    return dw.astype("<u4").view(np.uint8).reshape(n, k // 2)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_quant4_groups_recipe_and_bound(dtype):
    from stllm_amd import pack
    w = T("q4.q.w", (192, 640), 0.05)
    w[3, 128:256] = 0.0                          # a group of zeros
    w[7, 300] = 9.0                              # a group with one outlier
    w = w.to(dtype)
    qp, scale = pack.quant4_groups(w)
    assert qp.dtype == torch.uint8 and qp.is_contiguous() and qp.shape == (192, 320)
    assert scale.dtype == torch.float32 and scale.is_contiguous() and scale.shape == (192, 5) and bool((scale > 0).all())
    lo, hi = qp & 15, qp >> 4
    assert int(lo.min()) >= 1 and int(hi.min()) >= 1 and int(lo.max()) <= 15 and int(hi.max()) <= 15, "nibbles in [1, 15]: -8 never occurs"
    q, s = pack.dequant4_groups(qp, scale)
    assert q.dtype == torch.int8 and q.shape == (192, 640) and int(q.min()) >= -7 and int(q.max()) <= 7 and torch.equal(s, scale)
    assert float(scale[3, 1]) == 1.0 and int(q[3, 128:256].abs().max()) == 0
    assert int(q[7, 300]) == 7 and int(q[7, 256:384].abs().sort().values[-2]) <= 1
    err = (w.double() - deq(qp, scale)).abs().view(192, 5, 128)
    half = scale.double()[:, :, None] / 2
    print("quant4_groups: max |w - q scale| / (scale / 2) =", float((err / half).max()))
    assert bool((err <= half * (1 + 2.0 ** -20)).all())
    qn, sn = _numpy_recipe(w)
    assert np.array_equal(q.numpy(), qn) and np.array_equal(scale.numpy().view(np.uint32), sn.view(np.uint32))
    assert np.array_equal(qp.numpy(), _numpy_place(qn)), "the nibble placement of the docstring"
    # a 32-aligned slice of K is self-contained: its bytes are the bytes of the slice quantised with the same scales
    assert torch.equal(pack.dequant4_groups(qp[:, 16:32].contiguous(), scale)[0], q[:, 32:64])


def test_quant4_groups_commutes_with_the_packed_row_orders():
    from stllm_amd import pack
    dt = torch.bfloat16
    wq, wk, wv = T("q4.wq", (256, 256), 0.05), T("q4.wk", (256, 256), 0.05), T("q4.wv", (256, 256), 0.05)
    q, s = pack.quant4_groups(pack.llama_qkv(wq, wk, wv, dt, n_heads=2))
    perm = pack.rope_head_perm(2)
    parts = [pack.quant4_groups(x.to(dt)) for x in (wq, wk, wv)]
    assert torch.equal(q, torch.cat((parts[0][0][perm], parts[1][0][perm], parts[2][0])))
    assert torch.equal(s, torch.cat((parts[0][1][perm], parts[1][1][perm], parts[2][1])))
    wg, wu = T("q4.wg", (704, 256), 0.05), T("q4.wu", (704, 256), 0.05)
    q, s = pack.quant4_groups(pack.llama_gate_up(wg, wu, dt))
    (qg, sg), (qu, su) = pack.quant4_groups(wg.to(dt)), pack.quant4_groups(wu.to(dt))
    assert torch.equal(q.view(22, 2, 32, 128)[:, 0].reshape(704, 128), qg) and torch.equal(q.view(22, 2, 32, 128)[:, 1].reshape(704, 128), qu)
    assert torch.equal(s.view(22, 2, 32, 2)[:, 0].reshape(704, 2), sg) and torch.equal(s.view(22, 2, 32, 2)[:, 1].reshape(704, 2), su)


# ---- kernels on the host emulator -----------------------------------------------------------------------------------------------
def _expected_kernel(M, K, mfma):
    """stllm_gemv_q4's choice: the matrix-core kernel from M = 3 (option 1: from M = 1; 0: never), else the VALU kernel for M <= 8 whose staged rows fit"""
    if mfma != 0 and M >= (1 if mfma == 1 else 3):
        return "gemv_q4_mfma_kernel<"
    mr = M if M <= 2 else (M + 1) // 2 * 2
    return f"gemv_q4_kernel<MR{mr}" if M <= 8 and mr * K * 2 <= 150 * 1024 else None


def _ran(hip, want, what):
    name = hip.lib().stllm_last_kernel().decode()
    if want.startswith("gemv_q4_kernel<MR"):
        assert name.startswith("gemv_q4_kernel<") and name.endswith("," + want[len("gemv_q4_kernel<MR"):] + ">"), (what, name, want)
    else:
        assert name.startswith(want), (what, name, want)
    return name


def _check(got, ref, tol, what):
    got, ref = got.detach().double().cpu(), ref.double()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), what
    scale = max(float(ref.abs().max()), 1e-6)
    err = float((got - ref).abs().max())
    print(f"{what}: max err {err / scale:.3e} x scale (bound {tol:.1e})")
    assert err <= tol * scale, f"{what}: max err {err:.3e} > {tol:.1e} * {scale:.3e}"


def q4_case(hip, dtype, M, N, K, want, dev=lambda t: t, full=True):
    """every epilogue of stllm_gemv_q4 against fp64 of its contract on the nibbles and scales actually passed (shared with tests/test_q4_gpu.py)"""
    from stllm_amd import pack
    td = hip.torch_dtype(dtype)
    a = T("q4.a", (M, K), 0.5).to(td)
    qp, scale = pack.quant4_groups(T("q4.w", (N, K), 0.05).to(td))
    b = T("q4.b", (N,), 0.5)
    ref = a.double() @ deq(qp, scale).t() + b.double()
    import _poison
    # a leading dimension larger than K with NaN in the columns [K, lda): never read (include/stllm_hip.h: memory regions)
    ad, qd, sd, bd = _poison.nan_padded(dev(a)), dev(qp), dev(scale), dev(b)
    q0, s0 = qd.clone(), sd.clone()
    if want is None:
        with pytest.raises(RuntimeError, match="no kernel for M="):
            hip.gemv_q4(ad, qd, sd, dtype=dtype, out_f32=True)
        return
    g32 = _poison.Guarded(M, N, torch.float32, device=ad.device)     # the output inside a 0xFF-filled buffer: rows around it, columns [N, ldo)
    out = hip.gemv_q4(ad, qd, sd, dtype=dtype, bias=bd, out_f32=True, out=g32.out)
    _ran(hip, want, "store f32")
    _check(out, ref, ACC_TOL[dtype], "q4 store f32")
    assert g32.intact(), "q4 store f32: a byte outside the M x N output was written"
    x = T("q4.x", (M, N), 2.0)
    xd = _poison.nan_padded(dev(x.clone()))                          # resid columns [N, ldr): NaN, never read, never written
    hip.gemv_q4(ad, qd, sd, dtype=dtype, epilogue=hip.EPI_RESID, bias=bd, resid=xd)
    _check(xd, x.double() + ref, ACC_TOL[dtype], "q4 resid")
    assert bool(torch.isnan(torch.as_strided(xd, (M, 8), (xd.stride(0), 1), xd.storage_offset() + N)).all()), "q4 resid: the columns [N, ldr) were written"
    g16 = _poison.Guarded(M, N, td, device=ad.device)
    o16 = hip.gemv_q4(ad, qd, sd, dtype=dtype, bias=bd, out=g16.out)
    _check(o16, ref, OUT_TOL[dtype], "q4 store T")
    assert g16.intact(), "q4 store T: a byte outside the M x N output was written"
    buf = dev(torch.zeros((M, 3, N), dtype=td))       # output rows with a stride, untouched neighbours
    hip.gemv_q4(ad, qd, sd, dtype=dtype, out=buf[:, 1])
    _check(buf[:, 1], ref - b.double(), OUT_TOL[dtype], "q4 strided rows")
    assert float(buf[:, 0].abs().max()) == 0.0 and float(buf[:, 2].abs().max()) == 0.0
    if full:
        o = hip.gemv_q4(ad, qd, sd, dtype=dtype, epilogue=hip.EPI_SWIGLU)
        _ran(hip, want, "swiglu")
        g = (ref - b.double()).view(M, N // 64, 2, 32)
        _check(o, (F.silu(g[:, :, 0]) * g[:, :, 1]).reshape(M, N // 2), OUT_TOL[dtype], "q4 swiglu")
        cos, sin = pack.rope_tables(7)
        pos, rope_cols = 5, (N // 128 // 2) * 128 if N >= 256 else N      # the last columns stay unrotated where N allows
        o = hip.gemv_q4(ad, qd, sd, dtype=dtype, epilogue=hip.EPI_ROPE, rope=(dev(cos[pos:pos + 1].contiguous()), dev(sin[pos:pos + 1].contiguous())),
                        rope_seq=1, rope_cols=rope_cols)
        _ran(hip, want, "rope")
        _check(o, rope_ref(ref - b.double(), cos[pos:pos + 1], sin[pos:pos + 1], 1, rope_cols), OUT_TOL[dtype], "q4 rope")
    assert torch.equal(qd, q0) and torch.equal(sd, s0), "the weights and scales are read-only"


def q4_fused_norm_case(hip, dtype, M, I, K, dev=lambda t: t):
    """the fused RMSNorm operand: fp64 of RMSNorm rounded to the compute dtype, then the contract (the reference of test_gemv_fused_rmsnorm_operand)"""
    from stllm_amd import pack
    td = hip.torch_dtype(dtype)
    x = T("q4.nx", (M, K), 1.7)
    gamma = T("q4.ngamma", (K,), 0.2) + 1.0
    qp, scale = pack.quant4_groups(pack.llama_gate_up(T("q4.wg", (I, K), 0.05), T("q4.wu", (I, K), 0.05), td))
    one = hip.gemv_q4(None, dev(qp), dev(scale), dtype=dtype, epilogue=hip.EPI_SWIGLU, a_norm=(dev(x), dev(gamma), 1e-6))
    name = hip.lib().stllm_last_kernel().decode()
    assert name.startswith("gemv_q4_kernel<") and name.endswith(f",{M}>"), name
    x64 = x.double()
    hn = (gamma.double() * x64 * torch.rsqrt((x64 ** 2).mean(-1, keepdim=True) + 1e-6)).to(td).double()
    g = (hn @ deq(qp, scale).t()).view(M, 2 * I // 64, 2, 32)
    _check(one, (F.silu(g[:, :, 0]) * g[:, :, 1]).reshape(M, I), OUT_TOL[dtype], "q4 fused rmsnorm swiglu vs fp64")


@pytest.mark.skipif(not _hipemu.available() or _hipemu.ON_DEVICE, reason="host emulation of the kernel sources needs ROCm's clang++")
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("N,K", [(256, 640), (128, 2176)])
def test_gemv_q4_kernels_emulated(dtype, N, K):
    """K = 640 is 5 groups: the VALU kernel's one step is ragged (20 of 64 lanes) and 3 of the 8 matrix-core waves have no step; K = 2176 is one full
    2048-element VALU step plus a ragged one (4 lanes), 17 matrix-core steps"""
    with _hipemu.emulated() as hip:
        try:
            for M, mfma in EMU_CASES:
                hip.set_option("gemv_mfma", mfma)
                q4_case(hip, dtype, M, N, K, _expected_kernel(M, K, mfma), full=(N == 256 or M in (1, 5)))
            hip.set_option("gemv_mfma", -1)
            for M in (1, 2):
                q4_fused_norm_case(hip, dtype, M, N // 2, K)
        finally:
            hip.set_option("gemv_mfma", -1)
        td = hip.torch_dtype(dtype)
        a = T("q4.a", (17, K), 0.5).to(td)
        qp, s = torch.full((N, K // 2), 0x88, dtype=torch.uint8), torch.ones((N, K // 128))
        with pytest.raises(RuntimeError, match="decode regime"):
            hip.gemv_q4(a, qp, s, dtype=dtype)
        with pytest.raises(RuntimeError, match="K %% 128|K % 128"):
            hip.gemv_q4(a[:1, :K - 64], qp[:, :(K - 64) // 2], s, dtype=dtype)
        with pytest.raises(RuntimeError, match="no kernel for M="):
            hip.gemv_q4(None, qp, s, dtype=dtype, a_norm=(T("q4.nx9", (9, K), 1.0), torch.ones(K), 1e-6))


# ---- model ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    return small_llama(SMALL)


@pytest.fixture(scope="module")
def baseline(small):
    """decode logits of the 16-bit path before a quantised mode was ever switched on: no quantised entry point is reached"""
    from stllm_amd import runtime
    emb = T("q4.emb", (2, 12, 256), 0.05)
    with CB.installed(), runtime.use_dtype("bf16"):
        CB.CALLS_W8.clear(); CB.CALLS_Q4.clear()
        base16 = decode_run(small, emb, 8, 4)
        assert CB.CALLS_W8 == [] and CB.CALLS_Q4 == []
        return emb, base16


def test_int4_decode_equals_the_dequantised_model(small, baseline):
    from stllm_amd import pack, runtime
    emb, base16 = baseline
    lm = small.model
    with CB.installed(), runtime.use_dtype("bf16"):
        CB.CALLS_Q4.clear()
        with runtime.use_decode_weights("int4g128"):
            got = decode_run(small, emb, 8, 4)
        assert len(CB.CALLS_Q4) == 4 * 2 * 4 and all(c[1] == 2 for c in CB.CALLS_Q4), "4 projections per layer and step"
        assert sum(c[4] for c in CB.CALLS_Q4) == 4 * 2 * 2, "B = 2 <= FUSE_NORM_ROWS: the qkv and gate/up projections take the fused-norm form"
        assert runtime.decode_weights() is None

        def dequantise():   # the SAME 16-bit decode path over q * scale (fp32 tensors in place of the packed weights; the prefill before it used the originals)
            for pk in lm.pack(torch.bfloat16):
                for k in Q4_KEYS:
                    pk[k] = deq(*pack.quant4_groups(pk[k])).float()
        CB.CALLS_Q4.clear()
        try:
            want = decode_run(small, emb, 8, 4, before_decode=dequantise)
        finally:
            lm.repack()
        assert CB.CALLS_Q4 == []
        again = decode_run(small, emb, 8, 4)   # mode None (the default): bit-identical to the run made before the mode was ever switched on
    scale = max(float(w.abs().max()) for w in want)
    for g, w in zip(got, want):
        assert float((g - w).abs().max()) <= TOL * scale, (float((g - w).abs().max()), scale)
    assert not any(torch.equal(g, b) for g, b in zip(got, base16)), "4-bit weights must move the logits"
    assert all(torch.equal(a, b) for a, b in zip(again, base16))


def test_int4_weight_cache_follows_the_parameters_and_the_mode(small):
    """the 4-bit copy is keyed by the parameter fingerprint like the int8 one; one quantised copy at a time: int8 <-> int4g128 frees the other at the next step"""
    from stllm_amd import runtime
    lm = small.model
    emb = T("q4.emb", (1, 6, 256), 0.05)
    w = lm.layers[1].mlp.down_proj.weight
    w0 = w.detach().clone()
    try:
        with CB.installed(), runtime.use_dtype("bf16"):
            runtime.set_decode_weights("int4g128")
            assert runtime.decode_weights() == "int4g128"
            a = decode_run(small, emb, 4, 2)
            assert lm._quant[:2] == ("int4g128", torch.bfloat16)
            first = lm._quant.layers
            assert set(first[0]) == set(Q4_KEYS) and first[1]["wdown"][0].dtype == torch.uint8
            assert first[1]["wdown"][0].shape == (256, 384) and first[1]["wdown"][1].shape == (256, 6) and first[0]["wqkv"][1].shape == (768, 2)
            decode_run(small, emb, 4, 1)
            assert lm._quant[:2] == ("int4g128", torch.bfloat16) and lm._quant.layers is first, "unchanged parameters: the cached copy"
            w.copy_(w0 * 1.5)
            b = decode_run(small, emb, 4, 2)
            assert lm._quant[:2] == ("int4g128", torch.bfloat16)
            second = lm._quant.layers
            assert second is not first and not torch.equal(second[1]["wdown"][1], first[1]["wdown"][1])
            assert torch.equal(second[0]["wqkv"][0], first[0]["wqkv"][0]) and not torch.equal(a[-1], b[-1])
            assert lm._quant.mode != "int8", "no int8 copy is held"
            runtime.set_decode_weights("int8")
            CB.CALLS_Q4.clear(); CB.CALLS_W8.clear()
            decode_run(small, emb, 4, 1)
            assert lm._quant[:2] == ("int8", torch.bfloat16) and CB.CALLS_Q4 == [] and len(CB.CALLS_W8) == 8, "int8: the 4-bit copy is freed"
            runtime.set_decode_weights("int4g128")
            CB.CALLS_W8.clear()
            decode_run(small, emb, 4, 1)
            assert lm._quant[:2] == ("int4g128", torch.bfloat16) and len(CB.CALLS_Q4) == 8 and CB.CALLS_W8 == [], "and back: the int8 copy is freed"
            lm.repack()
            assert lm._quant is None
            decode_run(small, emb, 4, 1)
            runtime.set_decode_weights(None)
            decode_run(small, emb, 4, 1)
            assert lm._quant is None, "mode off: no quantised copy"
            for bad in ("int4", "int4g64", "q4"):
                with pytest.raises(ValueError, match="int4g128"):
                    runtime.set_decode_weights(bad)
            assert runtime.decode_weights() is None
    finally:
        runtime.set_decode_weights(None)
        w.copy_(w0)
        lm.repack()


def test_int4_rejects_the_modes_it_does_not_serve():
    from stllm_amd import runtime
    m = small_llama(SMALL)
    emb = T("q4.emb", (1, 6, 256), 0.05)
    with CB.installed(), runtime.use_decode_weights("int4g128"):
        with runtime.use_dtype("fp32"):
            c = m.model.new_cache(1, 8, "cpu")
            m.model.prefill(emb[:, :4], None, cache=c)
        for mode in ("fp32", "bf16x3", "mixed"):
            with runtime.use_dtype(mode), pytest.raises(NotImplementedError, match="int4g128 decode weights need a 16-bit compute mode"):
                m.model.decode_step(emb[:, 4:5], c)
        assert c.len == 4
        m.add_lora(8, 16)
        for i, mod in enumerate(m._lora_modules()):
            mod.B.copy_(T(f"q4.lora.B{i}", tuple(mod.B.shape), 0.02))
        with runtime.use_dtype("bf16"):
            with pytest.raises(NotImplementedError, match=r"int4g128 decode weights with active LoRA adapters: merge_adapter\(\) first"):
                decode_run(m, emb, 4, 1)
            m.merge_adapter()
            CB.CALLS_Q4.clear()
            decode_run(m, emb, 4, 1)
            assert len(CB.CALLS_Q4) == 8


def test_generate_runs_through_the_int4_path(small):
    """greedy behind a prefix cache, 5 beams, batching="ragged" and share_prefix=True: every decode step makes 4 q4 calls per layer, the norms fused for <= 2 rows"""
    from stllm_amd import runtime
    emb = T("q4.gen", (1, 9, 256), 0.05)
    emb2 = T("q4.gen2", (2, 9, 256), 0.05)
    mask2 = torch.tensor([[1] * 9, [1] * 6 + [0] * 3])
    kw = dict(max_new_tokens=5, do_sample=False, min_length=5)
    shapes = ((768, 256), (256, 256), (1536, 256), (256, 768))

    def counted(rows, fused):
        n = len(CB.CALLS_Q4)
        assert n > 0 and n % 8 == 0, n
        assert all(c[1] == rows and c[2:4] in shapes for c in CB.CALLS_Q4), sorted(set(CB.CALLS_Q4))
        per_step = [CB.CALLS_Q4[i:i + 8] for i in range(0, n, 8)]
        assert all([c[2:4] for c in st] == list(shapes) * 2 for st in per_step), "qkv, o, gate/up, down per layer"
        assert all(sum(c[4] for c in st) == (4 if fused else 0) for st in per_step)
        return n
    with CB.installed(), runtime.use_dtype("bf16"):
        off = small.generate(inputs_embeds=emb, num_beams=5, **kw)
        prefix = small.model.new_cache(1, 5, "cpu")
        small.model.prefill(emb[:, :5], None, cache=prefix)
        before = [b.clone() for b in prefix.qkv]
        with runtime.use_decode_weights("int4g128"):
            CB.CALLS_Q4.clear()
            ids = small.generate(inputs_embeds=emb[:, 5:], prefix_cache=prefix, num_beams=1, **kw)
            assert ids.shape == (1, 5) and int(ids.min()) >= 0 and int(ids.max()) < 512
            counted(1, True)
            assert prefix.len == 5 and all(torch.equal(x, y) for x, y in zip(prefix.qkv, before))
            CB.CALLS_Q4.clear()
            ids5 = small.generate(inputs_embeds=emb, num_beams=5, **kw)
            assert ids5.shape[0] == 1 and int(ids5.min()) >= 0 and int(ids5.max()) < 512
            counted(5, False)
            CB.CALLS_Q4.clear()
            idr = small.generate(inputs_embeds=emb2, attention_mask=mask2, batching="ragged", **kw)
            assert idr.shape[0] == 2
            counted(2, True)
            CB.CALLS_Q4.clear()
            ids_s = small.generate(inputs_embeds=emb[:, 5:], prefix_cache=prefix, num_beams=5, share_prefix=True, **kw)
            assert ids_s.shape[0] == 1
            counted(5, False)
            CB.CALLS_Q4.clear()
            ids_f = small.generate(inputs_embeds=emb[:, 5:], prefix_cache=prefix, num_beams=5, **kw)
            assert torch.equal(ids_s, ids_f), "shared base == forked copies under 4-bit weights"
            assert prefix.len == 5 and all(torch.equal(x, y) for x, y in zip(prefix.qkv, before))
        CB.CALLS_Q4.clear()
        assert torch.equal(small.generate(inputs_embeds=emb, num_beams=5, **kw), off) and CB.CALLS_Q4 == []


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
def test_abi_declares_and_exports_gemv_q4():
    from stllm_amd import hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "stllm_hip.h")).read()
    assert "stllm_gemv_q4" in hip.EXPORTS and re.search(r"^int stllm_gemv_q4\(const stllm_gemv_q4_args\* args, void\* stream\);", header, re.M)
    assert re.search(r"\}\s*stllm_gemv_q4_args;", header)
    assert callable(hip.gemv_q4)
    if os.path.exists(hip.LIB_PATH):
        L = hip.lib()
        assert hasattr(L, "stllm_gemv_q4") and L.stllm_abi_version() == 7
