#!/usr/bin/env python3
"""Micro-benchmark of the decode-regime GEMMs at Vicuna-7B size (weights rotate over enough copies to come from HBM every launch): the 16-bit
kernels (hip.gemm) and the int8-weight kernels (hip.gemv_w8) on the four decode shapes, with the GB/s of the weight bytes each actually reads.
   python tools/gemv_bench.py [rows ...]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from stllm_amd import hip, pack

rows = [int(a) for a in sys.argv[1:]] or [1, 5]
SHAPES = [("qkv rope", 12288, 4096, "rope"), ("o resid", 4096, 4096, "resid"), ("gate/up swiglu", 22016, 4096, "swiglu"), ("down resid", 4096, 11008, "resid")]
dt = "bf16"
for M in rows:
    tot = {"16": 0.0, "int8": 0.0}
    for name, N, K, kind in SHAPES:
        ncopy = max(2, int(600e6 // (N * K * 2)) + 1)
        ws = [(torch.randn(N, K, device="cuda") * 0.02).to(torch.bfloat16) for _ in range(ncopy)]
        a = (torch.randn(M, K, device="cuda") * 0.5).to(torch.bfloat16)
        x = torch.randn(M, N, device="cuda")
        cos = torch.ones(1, 64, device="cuda"); sin = torch.zeros(1, 64, device="cuda")
        epi = dict(resid=dict(epilogue=hip.EPI_RESID, resid=x), swiglu=dict(epilogue=hip.EPI_SWIGLU),
                   rope=dict(epilogue=hip.EPI_ROPE, rope=(cos, sin), rope_seq=1, rope_cols=N // 3 * 2))[kind]
        for fmt in ("16", "int8"):
            if fmt == "int8":   # twice the copies keep the rotating set as large in bytes
                ws = [pack.quant8_rows(w) for w in ws] + [pack.quant8_rows(w.flip(0)) for w in ws]
            run = (lambda w: hip.gemm(a, w, dtype=dt, **epi)) if fmt == "16" else (lambda w: hip.gemv_w8(a, w[0], w[1], dtype=dt, **epi))
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
            wb = N * K * (2 if fmt == "16" else 1)
            print(f"M={M:2d} {name:15s} N={N:5d} K={K:5d} weights {fmt:>4s} {us:7.1f} us  {wb / us / 1e3:7.1f} GB/s  [{hip.lib().stllm_last_kernel().decode()}]")
        del ws
    print(f"M={M:2d} per layer: 16-bit {tot['16']:.1f} us, int8 {tot['int8']:.1f} us -> x32 = {tot['16'] * 32 / 1e3:.2f} / {tot['int8'] * 32 / 1e3:.2f} ms")
