"""Overhead of active LoRA adapters on the c2-shaped Llama prefill (B = 1, S = 576, bf16) — HIP-event timings on one process and one GPU:
base model, adapters active (r = 16, r = 64), adapters merged; the down-projection kernel alone; one decode step with and without adapters.
Prints a markdown table (profiles/lora_overhead.md is a copy of one run).

    python tools/lora_bench.py [--layers 32] [--iters 20] [--mode bf16]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--mode", default="bf16")
    ap.add_argument("--seq", type=int, default=576)
    a = ap.parse_args()
    import stllm_amd  # noqa: F401
    from stllm_amd import hip, runtime, synth
    from stllm_amd.models.st_llm import STLLMForCausalLM, StllmConfig
    torch.set_grad_enabled(False)
    runtime.set_compute_dtype(a.mode)
    dt = runtime.compute_dtype()
    m = STLLMForCausalLM(StllmConfig(num_hidden_layers=a.layers), device="cuda")
    synth.fill_module_(m, 0, "")
    lm = m.model
    emb = synth.normal_(torch.empty((1, a.seq, 4096), device="cuda"), "bench.emb", 0, 0.05)
    tok = synth.normal_(torch.empty((1, 1, 4096), device="cuda"), "bench.tok", 0, 0.05)
    rows = []

    def measure(tag):
        med, best = timed(lambda: lm.prefill(emb), a.iters)
        cache = lm.new_cache(1, a.seq + 8 + 3 + a.iters, "cuda")
        lm.prefill(emb, None, cache=cache)
        dmed, dbest = timed(lambda: lm.decode_step(tok, cache), a.iters)
        rows.append((tag, med, best, dmed, dbest))
        print(f"[lora_bench] {tag}: prefill {med:.3f} ms (best {best:.3f}), decode step {dmed:.3f} ms (best {dbest:.3f})", flush=True)

    measure("base (no adapter modules)")
    for r in (16, 64):
        m.add_lora(r, 32)
        for i, mod in enumerate(m._lora_modules()):
            synth.normal_(mod.B, f"bench.B{i}", 0, 0.02)
        lm.repack()
        measure(f"adapters active, r = {r}")
        if r == 64:
            m.merge_adapter()
            measure("adapters merged, r = 64")
            m.unmerge_adapter()
        m.merge_and_unload()
    measure("base again (after merge_and_unload)")
    down = []
    for r in (8, 16, 64):
        P = hip.lora_pad(r, dt)
        A = torch.randn((2 * r, 4096), device="cuda").to(dt)
        for M in (1, 5, 576, 2304):
            buf = torch.randn((M, 4096 + P), device="cuda").to(dt)
            med, best = timed(lambda: hip.lora_down(buf[:, :4096], A, dtype=dt, out=buf[:, 4096:]), a.iters)
            down.append((r, M, med * 1e3, best * 1e3))
    props = torch.cuda.get_device_properties(0)
    print(f"\n# LoRA overhead — {props.name}, {a.layers} layers, S = {a.seq}, {a.mode}, median of {a.iters} (best in brackets), HIP events\n")
    print("| model | prefill ms | vs base | decode step ms | vs base |\n|---|---|---|---|---|")
    b = rows[0]
    for tag, med, best, dmed, dbest in rows:
        print(f"| {tag} | {med:.3f} ({best:.3f}) | {med / b[1]:.3f}x | {dmed:.3f} ({dbest:.3f}) | {dmed / b[3]:.3f}x |")
    print("\n| stllm_lora_down: r | M | us (incl. launch, host-paced) | best us |\n|---|---|---|---|")
    for r, M, med, best in down:
        print(f"| {r} | {M} | {med:.1f} | {best:.1f} |")


if __name__ == "__main__":
    main()
