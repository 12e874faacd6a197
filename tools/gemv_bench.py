#!/usr/bin/env python3
"""Micro-benchmark of the decode-regime GEMMs at Vicuna-7B size (weights rotate over enough copies to come from HBM every launch): the 16-bit
kernels (hip.gemm), the int8-weight kernels (hip.gemv_w8) and the 4-bit group-scaled kernels (hip.gemv_q4) on the four decode shapes, side by side,
with the GB/s of the weight bytes (scales included) each actually reads.
   python tools/gemv_bench.py [rows ...] [--dtype bf16|fp16]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from stllm_amd import hip, pack

argv = sys.argv[1:]
dt = argv.pop(argv.index("--dtype") + 1) if "--dtype" in argv else "bf16"
argv = [a for a in argv if a != "--dtype"]
rows = [int(a) for a in argv] or [1, 5]
td = hip.torch_dtype(dt)
FMTS = ("16", "int8", "int4g128")
SHAPES = [("qkv rope", 12288, 4096, "rope"), ("o resid", 4096, 4096, "resid"), ("gate/up swiglu", 22016, 4096, "swiglu"), ("down resid", 4096, 11008, "resid")]
for M in rows:
    tot = {f: 0.0 for f in FMTS}
    for name, N, K, kind in SHAPES:
        ncopy = max(2, int(600e6 // (N * K * 2)) + 1)
        ws16 = [(torch.randn(N, K, device="cuda") * 0.02).to(td) for _ in range(ncopy)]
        a = (torch.randn(M, K, device="cuda") * 0.5).to(td)
        x = torch.randn(M, N, device="cuda")
        cos = torch.ones(1, 64, device="cuda"); sin = torch.zeros(1, 64, device="cuda")
        epi = dict(resid=dict(epilogue=hip.EPI_RESID, resid=x), swiglu=dict(epilogue=hip.EPI_SWIGLU),
                   rope=dict(epilogue=hip.EPI_ROPE, rope=(cos, sin), rope_seq=1, rope_cols=N // 3 * 2))[kind]
        for fmt in FMTS:   # more copies of the smaller formats keep the rotating set as large in bytes
            if fmt == "16":
                ws = ws16
                run = lambda w: hip.gemm(a, w, dtype=dt, **epi)
            elif fmt == "int8":
                ws = [pack.quant8_rows(w) for w in ws16] + [pack.quant8_rows(w.flip(0)) for w in ws16]
                run = lambda w: hip.gemv_w8(a, w[0], w[1], dtype=dt, **epi)
            else:
                ws = [pack.quant4_groups(w.roll(r, 0)) for w in ws16 for r in range(4)]
                run = lambda w: hip.gemv_q4(a, w[0], w[1], dtype=dt, **epi)
            for w in ws[:2]:
                run(w)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            reps = 3 * len(ws)
            s.record()
            for i in range(reps):
                run(ws[i % len(ws)])
            e.record(); torch.cuda.synchronize()
            us = s.elapsed_time(e) * 1e3 / reps
            tot[fmt] += us
            wb = N * K * {"16": 2.0, "int8": 1.0, "int4g128": 0.5 + 4.0 / 128}[fmt] + (4 * N if fmt == "int8" else 0)
            print(f"M={M:2d} {name:15s} N={N:5d} K={K:5d} weights {fmt:>8s} {us:7.1f} us  {wb / us / 1e3:7.1f} GB/s  [{hip.lib().stllm_last_kernel().decode()}]")
            del ws
        del ws16
    print(f"M={M:2d} per layer: " + ", ".join(f"{f} {tot[f]:.1f} us" for f in FMTS) + " -> x32 = " + " / ".join(f"{tot[f] * 32 / 1e3:.2f}" for f in FMTS) + " ms")
