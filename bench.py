#!/usr/bin/env python3
"""bench.py — video-tokens/sec through ViT + Q-Former + projector + Vicuna-7B prefill (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config c2|c3|c4|c5] [--dtype bf16|fp16|fp32|bf16x3] [--full] [--no-cpu-baseline]
                    [--dump-outputs DIR]

A plain run (no --full) sets up, warms up, times the K steps and prints the headline line: `metric`, `value`, `unit`, `higher_is_better`,
`dtype`, `ms_per_step` (+ the workload's description and the timed bracket's per-block times).  Everything else the benchmark measures or
checks is behind `--full`: the parity against the reference fixture, the roofline of the dominant GEMM symbol, the device telemetry, the
single-stream bracket, the fp16 / fp32 / split-verify legs, the frame_parallel_projection block (N = 1), the frame_parallel block (N > 1)
and the CPU baseline (the `--no-*` switches below each turn one of them off again inside a `--full` run).
`--dump-outputs DIR`: after the timed steps, rank 0 writes what the last timed step returned as DIR/<name>.npy (float32; see dump_outputs).

`--gpus N` with N > 1 and no WORLD_SIZE in the environment: bench.py starts the N ranks itself (one process per GPU,
rendezvous on 127.0.0.1); under `python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...` it uses the
RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* it is given.  Rank 0 prints ONE JSON line.

A "step" = one pass of the hot path over one batch of synthetic input (frames already resident in HBM):
frames -> EVA-CLIP-g (39 blocks) -> ln_vision -> Q-Former (12 layers) -> llama_proj -> [N > 1, a clip shared by a team of ranks:
point-to-point exchange of the team's token sub-blocks] -> pooling -> token-block assembly -> Vicuna-7B (32 layers) prefill
[sequence-parallel inside the team] -> lm_head (all positions) -> shifted CE.  Random-init weights (stllm_amd.synth), full sizes.

  --config c2 (default; BASELINE.json configs[1], the metric's configuration): per GPU one clip of T=16 frames, 'all' pooling
      (512 video tokens), S = 576.  N > 1 = WEAK scaling: N clips per step, one clip per rank (a team of one: nothing is exchanged).
  --config c3 (BASELINE.json configs[2]; reference config/instructblipbase_stllm_conversation.yaml:14-15,21): B=4 clips of
      T=64 frames, text-conditioned Q-Former, global-local 'residual' pooling R=16 (512 video tokens per clip), S ~ 580.
      STRONG scaling: the same 4 x 64 frames at every N as clip teams (stllm_amd.parallel.TeamPlan): at N = 8 two ranks per clip, 32 frames
      each, token sub-blocks exchanged point-to-point, the clip's prefill sequence-parallel over the pair — where the north star's
      ">= 6x at 8 GPUs" lives.
  --config c4 (BASELINE.json configs[3]; reference st_llm.py:56-92, 480-493): T=32, 'all' pooling (1024 video tokens), dynamic masking
      (the mask the reference drew from numpy's RNG seeded with 1234: rate 0.547, 464 tokens kept) and the MVM branch: TWO prefills per
      step (S = 528 masked with lm_head + CE, S = 1088 un-masked), mvm_decoder + cosine loss.  One clip per GPU.
  --config c5 (BASELINE.json configs[4]; reference config/minigpt4base_stllm_qa.yaml:3,7,11,13-14): BT-Adapter backbone (temporal + spatial
      side branch on the last 3 ViT blocks), T=16, 'all' pooling, mask + MVM.  One clip per GPU (the backbone shards by clip only).
      c3 / c4 / c5 each have a full-size reference fixture (tests/golden/c{3,4,5}_full.npz): their lines carry `parity` like c2's.
  At N > 1 the c2 run with --full ALSO carries the north star's frame-parallel experiment in the same invocation:
      after the c2 timing the ranks build config c3, rank 0 times it ALONE (1-GPU reference, the other ranks wait at a barrier),
      then all N ranks time it as clip teams -> "frame_parallel": {ms_per_step_1gpu, ms_per_step + speedup (steps back to back),
      latency_ms + latency_speedup (one batch between barriers), plan, token_exchange_us, frames_per_rank, received_blocks_bit_identical}.
  At N = 1 (c2) the --full line also carries an fp16 leg, the fp32 "verify" leg and the SPLIT verify leg (bf16x3: three bf16 matrix-core products
      per Linear, fp32 everything else) — ms_per_step + parity each — next to the timed bf16, a `frame_parallel_projection` block (config c3
      timed on this one GPU, then every kind of rank at N = 2 / 4 / 8 played alone on it: throughput_ms and latency_ms from the measured shares + a MODELLED wire),
      the device's clock / power over the timed region (`telemetry`) and the timed region's per-block times (`ms_per_step_blocks`).
  --dry-cpu: plumbing check of the multi-rank code path on CPU (gloo, tests/_cpu_backend.py instead of the HIP library,
      reduced depth): NOT a measurement — used by tests/test_bench_cpu.py.

`value` = video tokens entering the LLM per second, whole job (B * 512 / step time), inputs resident in HBM.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

MFMA_PEAK = {"bf16": 2500.0, "fp16": 2500.0, "fp32": 157.3, "bf16x3": 2500.0, "mixed": 2500.0}  # dense TFLOP/s, MI355X_MICROARCH.md (bf16x3: bf16 MFMAs, 3x the algorithmic FLOPs)
ROUND = 6   # profiles/traffic_r{ROUND:02d}.json is the HBM-traffic measurement that belongs to this round's kernels

CONFIGS = {
    "c2": dict(clips=None, frames=16, scaling="weak",
               model=dict(video_input="all", qformer_text_input=False, max_txt_len=32)),
    "c3": dict(clips=4, frames=64, scaling="strong",
               model=dict(video_input="residual", residual_size=16, qformer_text_input=True, max_txt_len=64)),
    "c4": dict(clips=None, frames=32, scaling="weak",
               model=dict(video_input="all", use_mask=True, mvm_decode=True, qformer_text_input=False, max_txt_len=32)),
    "c5": dict(clips=None, frames=16, scaling="weak",
               model=dict(vit_model="eva_btadapter_g", video_input="all", use_mask=True, mvm_decode=True, qformer_text_input=False, max_txt_len=32)),
}
CONFIG_NAMES = {"c2": "BASELINE configs[1]", "c3": "BASELINE configs[2]", "c4": "BASELINE configs[3]", "c5": "BASELINE configs[4]"}
MASK_SEED = 1234   # numpy's global RNG in front of the mask draw (st_llm.py:482-484) — the seed tests/golden/make_fixtures.py fx_full used


def build_model(device, args, model_cfg=None):
    from stllm_amd import synth
    from stllm_amd.models import st_llm
    from stllm_amd.models.blip2 import Blip2Base
    Blip2Base.vit_depth, Blip2Base.qformer_layers = args.vit_depth, args.qformer_layers
    cfg = dict(vit_model="eva_clip_g", image_size=224, num_query_token=32, video_input="all", use_mask=False,
               mvm_decode=False, qformer_text_input=False, max_txt_len=32, end_sym=" 2",
               llama_model=dict(num_hidden_layers=args.llm_layers))
    cfg.update(model_cfg or {})
    if cfg.get("qformer_text_input"):
        # text-conditioned configs (c3): the token-id conventions of the fixture generator's fake tokenizers (tests/golden/ref_shim.py: BERT side
        # bos id 1 in a 32000-word table, no '[PAD]' growth of the Llama vocabulary), so that bench.py's c3 inputs are exactly what the
        # reference ran for tests/golden/c3_full.npz; the workload's sizes do not change (32000 instead of 32001 lm_head rows)
        from stllm_amd.tokenizer import IdTokenizer
        IdTokenizer.hf_special_tokens = False
        Blip2Base.init_tokenizer = classmethod(lambda cls, truncation_side="right": IdTokenizer(0, 1, 2, 32000))
    model = st_llm.STLLMForCausalLM.from_config(cfg, device=device)
    if getattr(args, "dry_cpu", False):
        # plumbing check on CPU: the values do not matter, the integer-hash generator (bit-identical on CPU and GPU, ~40 s for the
        # full-width tensors on a host core) does cost — every rank draws the same numbers from the same torch seed instead
        g = torch.Generator().manual_seed(1234)
        with torch.no_grad():
            for name, t in model.named_parameters():
                if torch.is_floating_point(t):
                    mean, std = synth._rule(name)
                    t.copy_(torch.randn(t.shape, generator=g) * std + mean)
    else:
        synth.fill_module_(model, 0, "")
    return model.eval()


def make_samples(B, T, device, seed=0, text=False):
    """Fixed token ids + seeded frames.  (B=1, T=16, text=False) is also what tests/golden/make_fixtures.py c2_full fed to
    the reference: do not change it without regenerating tests/golden/c2_full.npz."""
    from stllm_amd import synth
    g = torch.Generator().manual_seed(seed)
    ids = lambda n: " ".join(str(int(x)) for x in torch.randint(3, 32000, (n,), generator=g))
    frames = synth.normal_(torch.empty(B, T, 3, 224, 224, device=device), "input.video", seed, 1.0)
    if text:   # InstructBLIP-style prompt: the Q-Former sees the question (st_llm.py:456-459); its ids must also exist in BERT's 30523-word table
        qids = lambda n: " ".join(str(int(x)) for x in torch.randint(3, 30000, (n,), generator=g))
        instr = [ids(7) + "<ImageHere>" + ids(16) + " Human: " + qids(24) + " ###" for _ in range(B)]
    else:
        instr = [ids(7) + "<ImageHere>" + ids(40) for _ in range(B)]
    return {"image": frames, "instruction_input": instr, "answer": [ids(15) for _ in range(B)]}  # +eos => 16 answer ids


def draw_mask(L, B):
    """The dynamic mask exactly as the reference draws it (st_llm.py:482-485; models/utils.py:4-16): rate ~ N(0.5, 0.1) clipped to
    [0.1, 0.7], then one shuffled 0/1 row per clip, all from numpy's global RNG — seeded like the fixture generator, so that at B = 1
    the mask equals the one stored in tests/golden/c{4,5}_full.npz (checked by parity_vs_fixture)."""
    import numpy as np
    from stllm_amd.models.utils import RandomMaskingGenerator
    np.random.seed(MASK_SEED)
    rate = np.random.normal(0.5, 0.1)
    return RandomMaskingGenerator(L, float(np.clip(rate, 0.1, 0.7)), B)


def algorithmic_flops(T, S, Lt=0, S_unmasked=0, btadapter=False):
    """2*MAC, unpadded; per clip.  S_unmasked: the MVM branch's second prefill (no lm_head).  The BT-Adapter branch
    (3 blocks on T-frame temporal + spatial attention, ~8 % of the backbone) is NOT counted: the figure is a lower bound for c5."""
    vit = T * 520.72e9
    qf_frame = 12.75e9 + (18.30e9 - 12.75e9) * (Lt / 32.0)
    qf = T * qf_frame + T * 0.201e9
    body = lambda s: s * 2 * 32 * (4 * 4096 ** 2 + 3 * 4096 * 11008) + 2 * s * s * 4096 * 32
    llm = body(S) + 2 * 4096 * 32000 * S + (body(S_unmasked) if S_unmasked else 0)
    return vit + qf + llm


def cpu_baseline(T, S, budget_s=25.0):
    """The oracle (a port of the reference's CPU path, oracle/stllm_oracle.py) timed on this box's host cores
    on ONE whole clip of the same workload (reported, never the target)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import shapes
    import stllm_oracle as O
    rnd = lambda shp: {k: torch.randn(v) * 0.02 for k, v in shp.items()}
    # thread count: probed, not assumed (64 threads ran a frame SLOWER than the build container's 8 vCPUs — oversubscription).
    # A small ViT slice (4 frames x 2 blocks) at 8 / 16 / 32 / 64 / all hardware threads; the sample below runs at the fastest, both are reported.
    ncpu = os.cpu_count() or 1
    probe = {}
    with torch.no_grad():
        sdp = rnd(shapes.vit_shapes(2, "v."))
        frp = torch.randn(4, 3, 224, 224)
        for n in sorted({c for c in (8, 16, 32, 64, 96, min(ncpu, 128)) if c <= ncpu} or {1}):
            torch.set_num_threads(n)
            O.vit_forward(frp[:1], sdp, "v.")
            t0 = time.perf_counter(); O.vit_forward(frp, sdp, "v."); probe[n] = time.perf_counter() - t0
    cores = min(probe, key=probe.get)
    torch.set_num_threads(cores)
    # the FULL stack is run once — 16 frames through 39 ViT blocks and 12 Q-Former layers, the S-token sequence through 32 decoder layers
    # and lm_head — instead of a slice multiplied up.  Only the WEIGHT TENSORS are bounded: 8 distinct blocks / layers of random values, block i of the run
    # uses set i % 8 (6.5 GB of decoder weights instead of 26 GB of host memory; still far beyond any cache, so every pass streams its weights from DRAM
    # like distinct ones would).
    NF, VB, QL, LL, WSETS = T, 39, 12, 32, 8
    import re

    def rnd_cycled(shp, pat):
        """random tensors for the shape table; keys whose block / layer index (regex group 1 of `pat`) is >= WSETS alias the tensors of index % WSETS"""
        out = {}
        for k, v in shp.items():
            m = re.search(pat, k)
            if m and int(m.group(1)) >= WSETS:
                continue
            out[k] = torch.randn(v) * 0.02
        for k in shp:
            m = re.search(pat, k)
            if m and int(m.group(1)) >= WSETS:
                out[k] = out[k[:m.start(1)] + str(int(m.group(1)) % WSETS) + k[m.end(1):]]
        return out

    with torch.no_grad():
        sd = rnd_cycled(shapes.vit_shapes(VB, "v."), r"blocks\.(\d+)\.")
        fr = torch.randn(NF, 3, 224, 224)
        O.vit_forward(fr[:1], {k: v for k, v in sd.items()}, "v.")  # warm-up (thread pool, allocator)
        t0 = time.perf_counter(); O.vit_forward(fr, sd, "v."); t_vit = time.perf_counter() - t0
        sd = rnd({**shapes.qformer_shapes(QL, False, p="q."), "qt": (1, 32, 768)})
        enc = torch.randn(NF, 257, 1408)
        O.qformer_forward(sd["qt"].expand(2, -1, -1), enc[:2], sd, "q.")
        t0 = time.perf_counter(); O.qformer_forward(sd["qt"].expand(NF, -1, -1), enc, sd, "q."); t_qf = time.perf_counter() - t0
        sd = rnd_cycled({k: v for k, v in shapes.llama_shapes(LL).items() if "embed" not in k}, r"layers\.(\d+)\.")
        x = torch.randn(1, S, 4096) * 0.05
        O.llama_forward(x[:, :16], None, sd)
        t0 = time.perf_counter(); h = O.llama_forward(x, None, sd); t_llm = time.perf_counter() - t0
        t0 = time.perf_counter(); O.lm_logits(h, sd); t_head = time.perf_counter() - t0
    clip_s = t_vit + t_qf + t_llm + t_head
    return {"value": round(T * 32 / clip_s, 3), "unit": "video-tokens/s", "cores": cores, "kind": "port",
            "dtype": "f32", "host_threads_available": ncpu,
            "thread_probe_s": {str(n): round(t, 3) for n, t in sorted(probe.items())},   # ViT 4 frames x 2 blocks at each thread count: `cores` is the fastest
            "sample": f"oracle on CPU fp32, {cores} threads, ONE whole clip measured (nothing extrapolated): ViT {NF} frames x {VB} blocks ({t_vit:.2f}s), "
                      f"Q-Former {NF} frames x {QL} layers ({t_qf:.2f}s), Llama {LL} layers at S={S} ({t_llm:.2f}s) + lm_head ({t_head:.2f}s) "
                      f"=> {clip_s:.1f} s/clip; weight tensors: {WSETS} distinct random blocks / layers cycled (host memory), every pass streams from DRAM"}


def parity_vs_fixture(logits, loss, name="c2_full", mask=None):
    """Logits of the TIMED dtype against the reference's own CPU fp32 forward on the same inputs and synthetic weights
    (tests/golden/<name>.npz, a data fixture made by tests/golden/make_fixtures.py): max-abs error on the stored
    sub-sampled slice and top-1 agreement over all positions."""
    import numpy as np
    path = os.path.join(ROOT, "tests", "golden", name + ".npz")
    if not os.path.exists(path):
        return None
    g = np.load(path)
    lg = logits.float().cpu()
    want, top = g["logits_slice"], g["top_ids"]
    if want.ndim == 2:   # c2_full stores clip 0 only
        lg, want, top = lg[:1], want[None], top[None]
    if lg.shape[0] != want.shape[0] or lg.shape[1] != int(g["seq_len"][0]):
        return None
    err = float(np.abs(lg[:, ::3, ::499].numpy() - want).max())
    agree = float((lg.argmax(-1).numpy() == top[..., 0]).mean())
    res = {"fixture": f"tests/golden/{name}.npz (reference CPU fp32 forward, same inputs and weights)",
           "logits_max_abs_err": round(err, 5), "logits_abs_max": round(float(g["logits_stats"][1]), 3),
           "top1_agreement": round(agree, 4), "loss_err": round(abs(loss - float(g["loss"][0])), 6)}
    if mask is not None and "mask" in g.files:   # the mask bench.py drew with the package's generator == the one the reference drew
        res["mask_equals_reference"] = bool(np.array_equal(np.asarray(mask).astype(bool), g["mask"].astype(bool)))
    return res


DUMP_LOGITS_BYTES = 48 << 20   # c2's logits are 576 x 32000 fp32 = 70 MiB: more than the 64 MB a dump may hold


def dump_outputs(out, path):
    """--dump-outputs: what the timed step returned to its caller, as float32 .npy files under `path` — `loss`, `loss_mvm` (MVM configs) and
    `logits`, flattened to [rows, vocab].  Logits above DUMP_LOGITS_BYTES are a fixed sample of their rows (numpy seed 0, ascending; the same
    rows for the same shape): `logits_rows` holds the row numbers.  Two builds run with the same arguments are compared file for file."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    arrays = {}
    for name in ("loss", "loss_mvm"):
        v = getattr(out, name, None)
        if v is not None:
            arrays[name] = v.detach().float().cpu().numpy().reshape(-1)
    if out.logits is not None:
        lg = out.logits.detach().float().cpu().numpy()
        lg = lg.reshape(-1, lg.shape[-1])
        if lg.nbytes > DUMP_LOGITS_BYTES:
            rows = np.sort(np.random.default_rng(0).choice(lg.shape[0], DUMP_LOGITS_BYTES // lg[0].nbytes, replace=False))
            arrays["logits_rows"] = rows.astype(np.float32)
            lg = lg[rows]
        arrays["logits"] = np.ascontiguousarray(lg, dtype=np.float32)
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a)
    return sorted(arrays)


def load_traffic(kernel):
    """HBM bytes per launch of `kernel` from THIS round's PMC measurement (tools/pmc_traffic.sh -> profiles/traffic_rNN.json);
    None when the file is missing, from another round, or holds another kernel (a stale constant is worse than null)."""
    tp = os.path.join(ROOT, "profiles", f"traffic_r{ROUND:02d}.json")
    if not os.path.exists(tp):
        return None
    d = json.load(open(tp))
    if d.get("round") != ROUND:
        return None
    e = d.get("kernels", {}).get(kernel)
    return e.get("hbm_bytes_per_launch") if isinstance(e, dict) else None



# the reference's OWN reduced-precision gap on this kind of stack (HF Llama, 4096 wide, S = 178, N(0, 0.02) init, logits
# abs-max ~7; measured with the imported reference at survey time) — the calibration the fast modes' errors are read against
REFERENCE_OWN_GAP = {
    "source": "BASELINE.md §2 (HF Llama math of the reference, CPU, vs its own fp32)",
    "all_bf16_8_layers": {"logits_max_abs_err": 0.82, "top1_agreement": 0.84},
    "all_fp16_8_layers": {"logits_max_abs_err": 0.15, "top1_agreement": 0.99},
    "fp32_stream_bf16_gemm_32_layers": {"logits_max_abs_err": 0.26, "top1_agreement": 0.90},
    "fp32_stream_fp16_gemm_32_layers": {"logits_max_abs_err": 0.029, "top1_agreement": 0.98},
}


def numerics_legs(model, samples, args, sync):
    """N = 1, config c2: the same step in fp16 (the reference's production dtype, demo.py:46 / blip2.py:36-44) and in the fp32-MFMA
    "verify" mode, each with its parity against the reference's CPU logits.  Runs AFTER the timed bf16 region."""
    from stllm_amd import runtime
    out = {}
    for name, warm, steps in (("fp16", 3, 20), ("fp32", 1, 2), ("bf16x3", 2, 5), ("mixed", 2, 5)):
        runtime.set_compute_dtype(name)
        o = None
        for _ in range(warm):
            o = model(samples=samples)
        sync()
        prof = None
        if name == "fp16" and not args.no_roofline:   # the reference's production dtype gets its own roofline block: calibrate, then sample the dominant symbol
            from stllm_amd import hip
            prof = hip.GemmProfiler()
            prof.start_all()
            model(samples=samples)
            sync()
            cal = prof.summary()
            prof.start_target(max(cal, key=lambda k: cal[k]["total_ms"]), sampled=True)
        t0 = time.perf_counter()
        for _ in range(steps):
            o = model(samples=samples)
        sync()
        ms = (time.perf_counter() - t0) / steps * 1e3
        out[name] = {"ms_per_step": round(ms, 3), "steps": steps,
                     "parity": parity_vs_fixture(o.logits, float(o.loss.item()))}
        if prof is not None:
            t = prof.summary().get(prof.target)
            prof.stop()
            if t:
                ach = t["flops"] / (t["total_ms"] * 1e-3) / 1e12
                out[name]["roofline"] = {"bound": "mfma", "kernel": prof.target, "achieved": round(ach, 1), "peak": MFMA_PEAK["fp16"], "unit": "TFLOP/s",
                                         "frac": round(ach / MFMA_PEAK["fp16"], 4), "launches_timed": t["launches"], "avg_launch_ms": round(t["total_ms"] / t["launches"], 5),
                                         "algorithmic_gflop_per_launch": round(t["flops"] / t["launches"] / 1e9, 2), "traffic": None}
    runtime.set_compute_dtype(args.dtype)
    return out


def _c3_setup(args, device):
    conf = CONFIGS["c3"]
    T = args.frames if args.frames else conf["frames"]
    mconf = dict(conf["model"])
    if mconf.get("residual_size", 0) > T:
        mconf["residual_size"] = T
    model = build_model(device, args, mconf)
    B = args.fp_clips if getattr(args, "fp_clips", 0) else conf["clips"]
    return model, model.model.stllm_model, make_samples(B, T, device, text=True), B, T, mconf


def _encode_as_rank(sm, samples, plan, m, T, dt):
    """{clip: tokens} exactly as rank m of the plan computes them: ALL its frame ranges in one encode call (same launch shapes -> same bits)"""
    frames = samples["image"].reshape((-1,) + tuple(samples["image"].shape[2:]))
    qtext = [it.split("Human: ")[1].split(" ###")[0] for it in samples["instruction_input"]]
    all_t = [t for t in qtext for _ in range(T)]
    enc = plan.encodes(m)
    idx = [c * T + f for c, f0, f1 in enc for f in range(f0, f1)]
    if not idx:
        return {}
    contiguous = idx == list(range(idx[0], idx[0] + len(idx)))
    fr = frames[idx[0]: idx[0] + len(idx)] if contiguous else frames[torch.as_tensor(idx, device=frames.device)]
    toks = sm._encode_frames(fr, [all_t[i] for i in idx], T, dt)
    out, o = {}, 0
    for c, f0, f1 in enc:
        out[c] = toks[o: o + (f1 - f0)]
        o += f1 - f0
    return out


def frame_parallel_leg(args, world, rank, device, dry, sync):
    """The north star's multi-GPU experiment, inside the default `--gpus N` run: BASELINE configs[2] (c3: B = 4 clips x T = 64 frames,
    text-conditioned Q-Former, residual pooling R = 16; reference config/instructblipbase_stllm_conversation.yaml:14-15) under STRONG
    scaling — rank 0 alone first (the 1-GPU reference), then the N ranks as clip teams (stllm_amd.parallel.TeamPlan): a clip's frames are
    encoded by its team, the token sub-blocks travel point-to-point inside the team, the clip's prefill runs sequence-parallel over the team.
    Timed twice: back to back (`ms_per_step`: throughput, steps pipeline across ranks) and one batch at a time between barriers
    (`latency_ms`).  Also checks, once, that the token blocks rank 0 received are bit-identical to one GPU encoding the same frame ranges."""
    from stllm_amd import parallel, runtime
    model, sm, samples, B, T, mconf = _c3_setup(args, device)
    n_frames = B * T
    steps1 = 1 if dry else args.fp_steps_1gpu
    stepsN = 1 if dry else max(args.fp_steps, 30)      # >= 30: the pipeline's fill / drain is < 2 % of the bracket
    stepsL = 1 if dry else 10
    # ---- 1 GPU: rank 0 alone -------------------------------------------------------------------------
    ms1 = 0.0
    ref_blocks = None
    sm.set_frame_parallel(rank, world)
    plan = sm._team_plan(B, T)
    sm.set_frame_parallel(0, 1)
    if rank == 0:
        for _ in range(1 if dry else 2):
            model(samples=samples)
        sync_local(dry)
        t0 = time.perf_counter()
        for _ in range(steps1):
            model(samples=samples)
        sync_local(dry)
        ms1 = (time.perf_counter() - t0) / steps1 * 1e3
        dt = runtime.compute_dtype()
        ref_blocks = {}
        for c in plan.clips_of(0):      # the clips rank 0 prefills (a share of): every member's sub-block, computed as that member computes it
            ref_blocks[c] = torch.cat([_encode_as_rank(sm, samples, plan, m, T, dt)[c] for m, (f0, f1) in zip(plan.team[c], plan.frames[c]) if f1 > f0], dim=0)
            if sm.fp_wire_dtype() is not None and len(plan.team[c]) > 1:   # 16-bit wire: every member (the sender too) holds the sub-blocks rounded through it
                ref_blocks[c] = ref_blocks[c].to(sm.fp_wire_dtype()).float()
    sync()
    # ---- N GPUs -----------------------------------------------------------------------------------------
    sm.set_frame_parallel(rank, world)
    sm._fp_keep_tokens = True
    sm._fp_last_tokens = None
    out = None
    for _ in range(1 if dry else 3):
        out = model(samples=samples)
    sync()
    ident, ident_err = None, None
    if rank == 0:
        got = sm._fp_last_tokens
        ident = all(torch.equal(got[c].reshape(ref_blocks[c].shape), ref_blocks[c]) for c in ref_blocks)
        ident_err = max(float((got[c].reshape(ref_blocks[c].shape) - ref_blocks[c]).abs().max().item()) for c in ref_blocks)
        if not (ident_err <= 1e-3):   # a wrong frame, a wrong rank order or a torn transfer: stop — the timing below would be of a broken path
            raise RuntimeError(f"frame-parallel: a received token block differs from the 1-GPU encode of the same frame ranges (max abs diff {ident_err:.3e})")
    sm._fp_keep_tokens = False
    sm._fp_last_tokens = None
    del ref_blocks
    sync()
    t0 = time.perf_counter()
    for _ in range(stepsN):
        out = model(samples=samples)
    sync()
    dtN = time.perf_counter() - t0
    # ---- one batch at a time: barrier + synchronize around every step (what a single request sees) -------
    lat = 0.0
    for _ in range(stepsL):
        sync()
        t1 = time.perf_counter()
        out = model(samples=samples)
        sync()
        lat += time.perf_counter() - t1
    t = torch.tensor([dtN, lat], device=device, dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    msN, msL = float(t[0].item()) / stepsN * 1e3, float(t[1].item()) / stepsL * 1e3
    # ---- the token exchange on its own (same shapes, same stream) --------------------------------------
    local = {c: torch.zeros((f1 - f0, sm.tokens_per_frame, 4096), dtype=torch.float32, device=device) for c, f0, f1 in plan.encodes(rank)}
    x_us = 0.0
    wire = sm.fp_wire_dtype()
    wire_bytes = 2 if wire is not None else 4
    if plan.exchange_needed():
        for _ in range(3):
            parallel.exchange_clip_tokens(local, plan, rank, device=device, token_shape=(sm.tokens_per_frame, 4096), wire_dtype=wire)
        sync()
        t1 = time.perf_counter()
        reps = 2 if dry else 20
        for _ in range(reps):
            parallel.exchange_clip_tokens(local, plan, rank, device=device, token_shape=(sm.tokens_per_frame, 4096), wire_dtype=wire)
        sync()
        x_us = (time.perf_counter() - t1) / reps * 1e6
    R = mconf["residual_size"]
    res = {"config": "c3", "workload": f"BASELINE configs[2]: B={B} clips x T={T} frames, text-conditioned Q-Former, residual pooling R={R} "
                                       f"({R * 32} video tokens per clip), strong scaling (the same {n_frames} frames at every N)",
           "scaling": "strong", "steps_1gpu": steps1, "steps": stepsN, "latency_steps": stepsL,
           "ms_per_step_1gpu": round(ms1, 3), "ms_per_step": round(msN, 3), "speedup": round(ms1 / msN, 3) if msN > 0 else None,
           "latency_ms": round(msL, 3), "latency_speedup": round(ms1 / msL, 3) if msL > 0 else None,
           "video_tokens_per_s": round(B * R * 32 / (msN * 1e-3), 1), "frames_per_s": round(n_frames / (msN * 1e-3), 1),
           "plan": plan.describe(), "sequence_parallel_prefill": bool(any(plan.sp)),
           "token_exchange_us": round(x_us, 1), "token_exchange_in_step": bool(plan.exchange_needed()),
           "token_exchange_wire_dtype": str(wire).replace("torch.", "") if wire is not None else "float32",
           "token_exchange_bytes_sent_per_rank": [sum((f1 - f0) * sm.tokens_per_frame * 4096 * wire_bytes * (len(plan.receivers(c)) - (1 if r in plan.receivers(c) else 0)) for c, f0, f1 in plan.encodes(r))
                                                  for r in range(world)],
           "frames_per_rank": [sum(f1 - f0 for _, f0, f1 in plan.encodes(r)) for r in range(world)],
           "clips_per_rank": [len(plan.clips_of(r)) for r in range(world)],
           "received_blocks_bit_identical": ident, "received_blocks_max_abs_diff": ident_err}
    # ---- the round-4 work split on the same wire, for the trade-off (only where teams exist): the clip's owner prefills alone and encodes fewer
    # frames (water-filled): the better pipelined throughput, the worse one-batch latency
    if plan.exchange_needed() and any(plan.sp):
        sm.set_frame_parallel(rank, world, sp=False, balance="throughput")
        plan2 = sm._team_plan(B, T)
        for _ in range(1 if dry else 3):
            model(samples=samples)
        sync()
        t0 = time.perf_counter()
        for _ in range(stepsN):
            model(samples=samples)
        sync()
        dt2 = time.perf_counter() - t0
        lat2 = 0.0
        for _ in range(stepsL):
            sync()
            t1 = time.perf_counter()
            model(samples=samples)
            sync()
            lat2 += time.perf_counter() - t1
        t = torch.tensor([dt2, lat2], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        ms2, msL2 = float(t[0].item()) / stepsN * 1e3, float(t[1].item()) / stepsL * 1e3
        res["owner_only_throughput_plan"] = {"ms_per_step": round(ms2, 3), "speedup": round(ms1 / ms2, 3) if ms2 > 0 else None, "latency_ms": round(msL2, 3),
                                             "latency_speedup": round(ms1 / msL2, 3) if msL2 > 0 else None,
                                             "frames_per_rank": [sum(f1 - f0 for _, f0, f1 in plan2.encodes(r)) for r in range(world)],
                                             "clips_per_rank": [len(plan2.clips_of(r)) for r in range(world)]}
        sm.set_frame_parallel(rank, world, sp=True, balance="latency")
    del model
    return res


class Telemetry:
    """Device clock and socket power over the timed region (the same tree measures 22.4-25.3 ms/step across boxes, every
    kernel scaling together — without the clock a round-over-round delta below ~8 % is not attributable).  A helper thread samples
    amdsmi (ROCm's SMI library; python package in the image) every `period` seconds: two library calls per sample, no subprocess.
    Absent / failing SMI -> {"source": null}: never an error."""

    def __init__(self, device_index=0, period=0.1):
        import threading
        self.period, self.samples, self.src, self._stop = period, [], None, threading.Event()
        self._thr = None
        self._h = None
        try:
            import amdsmi
            self._smi = amdsmi
            amdsmi.amdsmi_init()
            hs = amdsmi.amdsmi_get_processor_handles()
            want = None
            try:   # match torch's device ordinal to an SMI handle by PCI address (HIP_VISIBLE_DEVICES may renumber)
                pr = torch.cuda.get_device_properties(device_index)
                want = f"{pr.pci_domain_id:04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}"
            except Exception:
                pass
            for h in hs:
                try:
                    bdf = str(amdsmi.amdsmi_get_gpu_device_bdf(h)).lower()
                except Exception:
                    bdf = ""
                if want and bdf.startswith(want):
                    self._h = h
            if self._h is None and hs:
                self._h = hs[min(device_index, len(hs) - 1)]
            if self._h is not None:
                self.src = "amdsmi"
        except Exception as e:   # no driver (CPU container), no library: report nothing
            self.err = repr(e)[:120]

    def _read(self):
        a = self._smi
        clk = pw = None
        try:
            c = a.amdsmi_get_clock_info(self._h, a.AmdSmiClkType.GFX)
            clk = c.get("clk", c.get("cur_clk"))
        except Exception:
            pass
        try:
            p_ = a.amdsmi_get_power_info(self._h)
            for k in ("current_socket_power", "average_socket_power", "socket_power"):
                v = p_.get(k)
                if isinstance(v, (int, float)) and v > 0:
                    pw = v
                    break
        except Exception:
            pass
        return clk, pw

    def start(self):
        if self.src is None:
            return self
        import threading

        def loop():
            while not self._stop.is_set():
                self.samples.append(self._read())
                self._stop.wait(self.period)
        self._thr = threading.Thread(target=loop, daemon=True)
        self._thr.start()
        return self

    def stop(self):
        if self._thr is not None:
            self._stop.set()
            self._thr.join(timeout=2.0)
        st = lambda xs: None if not xs else {"mean": round(sum(xs) / len(xs), 1), "min": round(min(xs), 1), "max": round(max(xs), 1)}
        clk = [float(c) for c, _ in self.samples if isinstance(c, (int, float))]
        pw = [float(p) for _, p in self.samples if isinstance(p, (int, float))]
        return {"source": self.src, "samples": len(self.samples), "period_s": self.period, "sclk_mhz": st(clk), "power_w": st(pw)}


XGMI_LINK_GBS_PER_DIR = 76.8   # MI355X: 7 xGMI links x ~153.6 GB/s bidirectional per GPU, fully connected 8-GPU node => one direct link per peer


def model_p2p_ms(nbytes, efficiency=0.7, latency_us=30.0):
    """MODELLED, not measured (no multi-GPU box in the build loop): one ncclSend / ncclRecv pair of `nbytes` over the direct xGMI link of its two ranks"""
    return latency_us * 1e-3 + nbytes / (XGMI_LINK_GBS_PER_DIR * 1e9 * efficiency) * 1e3


def model_allgather_ms(bytes_per_rank, world, efficiency=0.7, latency_us=50.0):
    """MODELLED: the round 1-4 all-gather of `bytes_per_rank` from each of `world` ranks (fp_mode "allgather").
    ring: (world - 1) steps over ONE link per direction (RCCL's default algorithm, the figure to plan with); direct: every peer's chunk on its own link."""
    bw = XGMI_LINK_GBS_PER_DIR * 1e9 * efficiency
    direct = latency_us * 1e-3 + bytes_per_rank / bw * 1e3
    ring = latency_us * 1e-3 + (world - 1) * bytes_per_rank / bw * 1e3
    return {"ring_ms": round(ring, 3), "direct_ms": round(direct, 3),
            "assumptions": f"modelled (xGMI: {XGMI_LINK_GBS_PER_DIR} GB/s per link and direction x {efficiency} efficiency, {latency_us:.0f} us launch + sync latency)"}


def frame_parallel_projection(args, device):
    """N = 1 only: ground the 8-GPU claim on ONE GPU (UNMEASURED on a multi-GPU node: the driver's SCALE run is the measurement).  Config c3
    (B = 4 clips x T = 64 frames, text Q-Former, residual R = 16; STRONG scaling) is timed whole on this GPU; then, for N = 2 / 4 / 8, every KIND
    of rank of the TeamPlan is played alone on this GPU — its frame ranges' encode, then its (share of the) prefill, receives replaced by
    parallel.Mailbox(dummy) — and timed twice: the encode alone (`enc_ms`) and the whole step (`step_ms`).  From those and a MODELLED wire:
        throughput_ms = max over ranks of step_ms + exchange            (steps back to back: no rank waits for another team)
        latency_ms    = max over clips of [max over the team of enc_ms + token exchange + max over its prefill ranks of (step_ms - enc_ms) + K|V lag]
    i.e. the critical path of ONE batch: a clip's prefill starts when ITS team's frames are in, not when the node's are."""
    from stllm_amd import parallel, runtime
    model, sm, samples, B, T, mconf = _c3_setup(args, device)

    def timed(fn, steps, warm):
        for _ in range(warm):
            fn()
        sync_local(args.dry_cpu)
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        sync_local(args.dry_cpu)
        return (time.perf_counter() - t0) / steps * 1e3
    steps1, stepsN = (1, 1) if args.dry_cpu else (args.fp_steps_1gpu, 5)
    sm.set_frame_parallel(0, 1)
    ms1 = timed(lambda: model(samples=samples), steps1, 1 if args.dry_cpu else 2)
    qtext = [it.split("Human: ")[1].split(" ###")[0] for it in samples["instruction_input"]]
    S = int(model(samples=samples).logits.shape[1])
    per_n = {}
    try:
        for N, variant in ((2, None), (4, None), (8, None), (8, "owner_only"), (8, "owner_only_latency")):
            # variant "owner_only": the round-4 work split on the round-5 wire — the clip's owner prefills alone and encodes fewer frames (water-filled,
            # balance "throughput"): the better PIPELINED throughput, the worse one-batch latency; "owner_only_latency": owner-only prefill with equal
            # frame shares.  Both reported next to the default (sequence-parallel prefill inside the team) for the trade-off.
            spk = dict(sp=False, balance="throughput" if variant == "owner_only" else "latency") if variant else dict(sp=True, balance="latency")
            sm.set_frame_parallel(0, N, mailbox=parallel.Mailbox(dummy=True), **spk)
            plan = sm._team_plan(B, T)

            def kind(r):
                return (tuple((f1 - f0) for _, f0, f1 in plan.encodes(r)), tuple((plan.member_index(c, r), len(plan.team[c]), plan.sp[c]) for c in plan.clips_of(r)))
            meas = {}
            for k in sorted(set(kind(r) for r in range(N))):
                r = min(q for q in range(N) if kind(q) == k)
                sm.set_frame_parallel(r, N, mailbox=parallel.Mailbox(dummy=True), **spk)
                enc_ms = timed(lambda: sm.encode_img(samples["image"], qtext), stepsN, 1)
                step_ms = timed(lambda: model(samples=samples), stepsN, 1)
                meas[k] = (enc_ms, step_ms)
            tok_ms = sp_lag = 0.0
            if plan.exchange_needed():
                tok_ms = max(model_p2p_ms((f1 - f0) * sm.tokens_per_frame * 4096 * (2 if sm.fp_wire_dtype() is not None else 4)) for c in range(B) for f0, f1 in plan.frames[c] if f1 > f0)   # the pairs run concurrently, each on its own link
            if any(plan.sp):
                kmax = max(len(plan.team[c]) for c in range(B) if plan.sp[c])
                sp_lag = (kmax - 1) * model_p2p_ms(S // kmax * 2 * 4096 * 2)     # member j trails member j - 1 by one K | V hand-over; the last layer's is exposed
            lat = 0.0
            for c in range(B):
                enc = max(meas[kind(m)][0] for m in plan.team[c])
                pre = max(max(0.0, meas[kind(m)][1] - meas[kind(m)][0]) for m in (plan.team[c] if plan.sp[c] else plan.team[c][:1]))
                lat = max(lat, enc + (tok_ms if len(plan.team[c]) > 1 else 0.0) + pre + (sp_lag if plan.sp[c] else 0.0))
            thr = max(v[1] for v in meas.values()) + tok_ms + sp_lag
            shares = [{"ranks_of_this_kind": sum(1 for q in range(N) if kind(q) == k), "frames": list(k[0]),
                       "prefill": [{"member": j, "team_size": kk, "sequence_parallel": bool(spf)} for j, kk, spf in k[1]],
                       "enc_ms": round(v[0], 3), "step_ms": round(v[1], 3)} for k, v in sorted(meas.items())]
            per_n[str(N) + ("_" + variant if variant else "")] = {"plan": plan.describe(), "shares": shares, "token_exchange_ms_modelled": round(tok_ms, 3), "kv_lag_ms_modelled": round(sp_lag, 3),
                             "throughput_ms": round(thr, 3), "throughput_speedup": round(ms1 / thr, 3),
                             "latency_ms": round(lat, 3), "latency_speedup": round(ms1 / lat, 3),
                             "projected_ms": round(thr, 3), "projected_speedup": round(ms1 / thr, 3),
                             "sum_of_shares_over_1gpu": round(sum(meas[kind(q)][1] for q in range(N)) / ms1, 3)}
        # ---- full-size numerics of the sequence-parallel path ON THIS GPU: the two members of clip 0's team at N = 8 played one after another through
        # a real mailbox (token sub-blocks both ways, K | V rows and the loss forward) -> their logits rows against the 1-GPU run's rows of clip 0
        sp_check = None
        plan8 = parallel.TeamPlan(B, T, 8)
        if plan8.sp[0]:
            sp_check = {"ranks": plan8.team[0], "note": "clip 0's team at N = 8 played on this GPU through a real mailbox; logits rows of every member against the 1-GPU run's rows "
                                                        "of clip 0.  In the timed dtype the two runs differ by that dtype's rounding (fewer rows pick other tiles / K-splits: the same order "
                                                        "as its parity error against the reference); the split verify mode shows the computation is the same"}
            for mode in ([args.dtype] if args.dry_cpu else [args.dtype, "bf16x3"]):
                runtime.set_compute_dtype(mode)
                sm.set_frame_parallel(0, 1)
                ref_lg = model(samples=samples).logits[0].float()
                outs = parallel.play_ranks(sm, lambda: model(samples=samples), plan8.team[0], 8, sp=True, balance="latency")
                diffs, agree, rows = [], [], []
                for r in plan8.team[0]:
                    s0, s1 = outs[r].sp_rows
                    lg = outs[r].logits[0].float()
                    n = min(s1, ref_lg.shape[0]) - s0
                    diffs.append(float((lg[:n] - ref_lg[s0:s0 + n]).abs().max().item()))
                    agree.append(float((lg[:n].argmax(-1) == ref_lg[s0:s0 + n].argmax(-1)).float().mean().item()))
                    rows.append([s0, s1])
                sp_check[mode] = {"rows": rows, "logits_max_abs_diff_vs_1gpu": [round(d, 6) for d in diffs], "top1_agreement_vs_1gpu": [round(a, 4) for a in agree],
                                  "logits_abs_max": round(float(ref_lg.abs().max().item()), 3)}
                del outs, ref_lg
            runtime.set_compute_dtype(args.dtype)
    finally:
        sm.set_frame_parallel(0, 1, sp=True, balance="latency")
    R = mconf["residual_size"]
    res = {"config": "c3", "workload": f"BASELINE configs[2]: B={B} clips x T={T} frames, text-conditioned Q-Former, residual pooling R={R}, strong scaling",
           "sequence_parallel_check": sp_check,
           "status": "UNMEASURED on a multi-GPU node — measured shares of ONE GPU + a modelled wire",
           "method": "measured on ONE GPU: the whole batch, then each kind of rank of the TeamPlan alone (its frames' encode; its share of its clip's prefill, "
                     "sequence-parallel inside the clip's team; receives are no-ops); throughput_ms = slowest rank's step + exchange, latency_ms = critical path of one batch",
           "wire_model": f"point-to-point over the pair's direct xGMI link: {XGMI_LINK_GBS_PER_DIR} GB/s per direction x 0.7 + 30 us per transfer (no ring: ncclSend / ncclRecv)",
           "steps_1gpu": steps1, "steps_per_share": stepsN, "ms_per_step_1gpu": round(ms1, 3), "n": per_n,
           "sum_of_shares_note": "sum_of_shares_over_1gpu > 1 = work lost to the smaller per-rank batches (GEMM tile quantisation at M = frames x 257, "
                                 "the prefill's GEMMs at M = S / team size)"}
    del model
    return res


def sync_local(dry):
    if not dry:
        torch.cuda.synchronize()


def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher: start the N ranks (one process per GPU) and forward rank 0's line."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    rc = 0
    deadline = time.time() + 3600
    for p in procs:
        try:
            rc = p.wait(timeout=max(1.0, deadline - time.time())) or rc
        except subprocess.TimeoutExpired:
            p.kill()
            rc = rc or 124
    if rc:
        for p in procs:   # a rank died: do not leave its peers waiting in a collective
            if p.poll() is None:
                p.kill()
    return rc


def run_rank(args):
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    args.gpus = world
    dry = args.dry_cpu
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if dry:
        device = torch.device("cpu")
        if world > 1:
            dist.init_process_group(backend="gloo")
    else:
        torch.cuda.set_device(local_rank)
        device = torch.device("cuda", local_rank)
        if world > 1:
            dist.init_process_group(backend="nccl", device_id=device)
    torch.set_grad_enabled(False)

    import contextlib
    backend = contextlib.nullcontext()
    if dry:   # TEST-ONLY contract backend (tests/_cpu_backend.py): checks the orchestration, measures nothing
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import _cpu_backend
        backend = _cpu_backend.installed()
        args.dtype = "fp32"
        args.no_roofline = args.no_cpu_baseline = True
    with backend:
        _run(args, world, rank, device, dry)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def _run(args, world, rank, device, dry):
    from stllm_amd import hip, runtime
    runtime.set_compute_dtype(args.dtype)
    conf = CONFIGS[args.config]
    T = args.frames if args.frames else conf["frames"]
    if conf["model"].get("residual_size", 0) > T:   # --frames override (debugging / dry runs): keep R <= T
        conf = dict(conf, model=dict(conf["model"], residual_size=T))
    model = build_model(device, args, conf["model"])
    sm = model.model.stllm_model
    sm.set_frame_parallel(rank, world)
    sm.visual_encoder.frame_streams = args.vit_streams
    B = conf["clips"] if conf["clips"] else world
    text = conf["model"]["qformer_text_input"]
    samples = make_samples(B, T, device, text=text)
    R = conf["model"].get("residual_size")
    Lvis = (R if conf["model"]["video_input"] == "residual" else T) * 32
    mask = None
    if conf["model"].get("use_mask"):   # the dynamic mask, drawn ONCE as the reference draws it and injected: every step times the same gather tables
        mask = draw_mask(Lvis, B)
        samples["mask"] = mask

    # clips in flight: also on every rank of an N > 1 run as long as the step has no exchange inside (c2 weak scaling: one whole clip per rank, teams of one) —
    # the per-N values the driver divides must be measured the same way at every N; a step with a token exchange / sequence-parallel prefill keeps one stream
    exchange_in_step = bool(world > 1 and sm.vit_model == "eva_clip_g" and sm._team_plan(B, T).exchange_needed())
    n_streams = max(1, args.streams) if (not dry and not exchange_in_step) else 1
    streams = [torch.cuda.Stream(device=device) for _ in range(n_streams)] if n_streams > 1 else []
    step_no = [0]

    def step():
        if not streams:
            return model(samples=samples)
        st = streams[step_no[0] % n_streams]
        step_no[0] += 1
        with torch.cuda.stream(st):
            return model(samples=samples)

    def sync():
        if world > 1:
            dist.barrier()
        if not dry:
            torch.cuda.synchronize()

    # ---- warmup (first step also packs the weights); calibration pass finds the dominant GEMM kernel ----
    out = None
    for i in range(max(args.warmup, 1, 2 * n_streams if n_streams > 1 else 1)):
        out = step()
        if i == 0 and streams and not dry:
            torch.cuda.synchronize()   # the first step packs the weights on ITS stream: the other streams' first steps must find them complete
    sync()
    own = getattr(sm, "owned_clips", list(range(B))) if world > 1 else list(range(B))
    S_local = (out.sp_rows[1] if getattr(out, "sp_rows", None) else out.logits.shape[1]) if out.logits is not None else 0   # (sequence-parallel: the clip's length = the last member's end)
    S_un = (S_local - sm.mask_img_len + sm.img_len) if (mask is not None and out.logits is not None) else 0   # the MVM branch's second prefill
    parity = None
    if args.full and rank == 0 and out.logits is not None and world == 1 and not dry and B == (conf["clips"] or 1):
        parity = parity_vs_fixture(out.logits, float(out.loss.item()), name=f"{args.config}_full", mask=mask)
    prof = None
    cal = {}
    if not args.no_roofline:
        # calibration step on EVERY rank (it contains the all-gather collective); only rank 0 times its GEMM launches
        if rank == 0:
            prof = hip.GemmProfiler()
            prof.start_all()
        step()
        sync()
        if rank == 0:
            cal = prof.summary()
            # the timed region: HIP events around every 7th launch of the dominant symbol (an odd period: its two alternating shapes are both
            # sampled); events around ALL of its 78 launches per step slowed the step they measure by 2 %
            prof.start_target(max(cal, key=lambda k: cal[k]["total_ms"]), sampled=True)
    # ---- timed region: EXACTLY K steps between barrier + synchronize ---------------------------------
    # The K steps run as up to 3 blocks with a device synchronisation (no barrier) between them: the blocks' own times show the spread
    # inside the run (clock ramps, a throttling box); ms_per_step is still the whole bracket, block boundaries included.
    nb = 3 if args.steps >= 6 else 1
    bsz = [args.steps // nb + (1 if i < args.steps % nb else 0) for i in range(nb)]
    tele = Telemetry(device.index or 0).start() if (args.full and rank == 0 and not dry) else None
    block_ms = []
    sync()
    t0 = time.perf_counter()
    for bi, nsteps in enumerate(bsz):
        tb = time.perf_counter()
        for _ in range(nsteps):
            out = step()
        if bi + 1 < nb:
            sync_local(dry)
            block_ms.append((time.perf_counter() - tb) / nsteps * 1e3)
    sync()
    dt_s = time.perf_counter() - t0
    block_ms.append((time.perf_counter() - tb) / bsz[-1] * 1e3)
    telemetry = tele.stop() if tele is not None else None
    target_summary = None
    if prof is not None:
        target_summary = prof.summary().get(prof.target)
        prof.stop()
    if args.dump_outputs and rank == 0:
        dump_outputs(out, args.dump_outputs)
    # ---- clips in flight (round 6): with streams > 1 the bracket above ran step k on HIP stream k % streams — every step is still one whole B = 1 pass
    # (encode + prefill + lm_head + loss), two of them share the chip: the small kernels' idle CUs, every launch's cold start and tail are covered by the
    # other clip's kernels.  With --full the SAME K-step loop on ONE stream follows (its own bracket, after the headline): the one-clip-at-a-time rate, and the bracket
    # in which the dominant kernel's own duration is sampled (an event pair around a launch that shares the chip with another stream's kernel times both).
    single_stream = None
    inflight_summary = None
    if streams and args.full:
        n1 = max(10, args.steps // 2)
        inflight_summary = target_summary
        saved, streams[:] = list(streams), []
        for _ in range(2):
            step()
        if prof is not None:
            prof.start_target(prof.target, sampled=True)
        sync()
        t1 = time.perf_counter()
        for _ in range(n1):
            out = step()
        sync()
        single_stream = {"steps": n1, "ms_per_step": round((time.perf_counter() - t1) / n1 * 1e3, 3)}
        if prof is not None:
            target_summary = prof.summary().get(prof.target)
            prof.stop()
        streams[:] = saved
    if not dry:
        if not hip.gemm_workspace_ok(device):   # a split-K exchange gave up waiting for a peer workgroup: the numbers would be meaningless
            raise RuntimeError(hip.lib().stllm_last_error().decode())
    t = torch.tensor([dt_s, float(S_local)], device=device, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dt_s, S = float(t[0].item()), int(t[1].item())
    ms_per_step = dt_s / args.steps * 1e3
    loss = float(out.loss.item()) if out.loss is not None else float("nan")
    bt = conf["model"].get("vit_model") == "eva_btadapter_g"

    plan_desc = None
    if world > 1 and sm.vit_model == "eva_clip_g":
        plan_desc = sm._team_plan(B, T)

    extra_legs = fp_leg = None
    if world == 1 and args.config == "c2" and not dry and not args.no_extra_legs and parity is not None:
        extra_legs = numerics_legs(model, samples, args, sync)
    projection = None
    if world == 1 and args.config == "c2" and not args.no_extra_legs and not args.no_projection and rank == 0:
        del model, out
        sm = None
        if not dry:
            torch.cuda.empty_cache()
        projection = frame_parallel_projection(args, device)
        out = model = None

    def _emit(fp_leg):
        from stllm_amd import parallel
        Lt = 24 if text else 0
        flop_clip = algorithmic_flops(T, S, Lt, S_unmasked=S_un, btadapter=bt)
        step_s = dt_s / args.steps
        par = "single GPU" if world == 1 else (f"clip teams over {world} ranks (stllm_amd.parallel.TeamPlan): a clip's frames encoded by its team, token sub-blocks "
                                               f"point-to-point inside the team, prefill sequence-parallel over the team")
        names = CONFIG_NAMES
        res = {"metric": f"video-tokens/sec (ViT+Qformer+LLM-prefill) at T={T}, Vicuna-7B", "value": round(B * Lvis / step_s, 2),
               "unit": "video-tokens/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": round(ms_per_step, 3), "ms_per_step_blocks": {"steps": bsz, "ms": [round(b, 3) for b in block_ms], "median": round(sorted(block_ms)[len(block_ms) // 2], 3),
                                                                                         "spread_pct": round((max(block_ms) - min(block_ms)) / min(block_ms) * 100, 2)},
               "telemetry": telemetry, "higher_is_better": True, "scaling": conf["scaling"], "vs_baseline": None,
               "dtype": args.dtype, "data": "synthetic (random 224x224 frames, random-init EVA-CLIP-g + Q-Former + Vicuna-7B, fixed token ids)",
               "config": {"workload": f"{names[args.config]}: B={B} clip(s)/step, T={T} frames, ViT {args.vit_depth} blocks + "
                                      f"Q-Former {args.qformer_layers} layers ({'text-conditioned, ' if text else ''}{conf['model']['video_input']} pooling) + "
                                      f"Llama {args.llm_layers} layers prefill S={S} + lm_head(all positions)" +
                                      (f" + MVM branch: un-masked prefill S={S_un}, mvm_decoder, cosine loss (mask {Lvis - (S_un - S)}/{Lvis} kept)" if S_un else "") +
                                      (" [BT-Adapter backbone]" if bt else "") +
                                      (f"; {n_streams} independent steps in flight (step k on HIP stream k % {n_streams}), each one whole B={B} pass" if streams else ""),
                          "name": args.config, "global_batch": B, "frames": T, "video_tokens_per_clip": Lvis, "seq_len": S, "parallelism": par},
               "frames_per_s": round(B * T / step_s, 2), "encoded_tokens_per_s": round(B * T * 32 / step_s, 1), "loss": round(loss, 5),
               "algorithmic_tflop_per_step": round(B * flop_clip / 1e12, 3),
               "end_to_end_tflops_per_gpu": round(B * flop_clip / step_s / 1e12 / world, 1)}
        if streams:
            res["clips_in_flight"] = n_streams
        if single_stream is not None:
            res["single_stream"] = dict(single_stream, value=round(B * Lvis / (single_stream["ms_per_step"] * 1e-3), 2), unit="video-tokens/s",
                                        note="the same step loop on ONE stream (one clip at a time: the latency of a clip), its own bracket right after the headline's")
        if world > 1:
            if plan_desc is not None:
                res["plan"] = plan_desc.describe()
                res["frames_per_rank"] = [sum(f1 - f0 for _, f0, f1 in plan_desc.encodes(r)) for r in range(world)]
                res["token_exchange_in_step"] = bool(plan_desc.exchange_needed())
            res["rccl_ranks"] = dist.get_world_size()
            if conf["scaling"] == "weak":
                res["scaling_note"] = ("weak scaling: one clip per GPU — every rank is a clip team of one, nothing is exchanged inside the step "
                                       "(token_exchange_in_step false); the frame-parallel strong-scaling experiment (config c3: clip teams, point-to-point "
                                       "exchange, sequence-parallel prefill) is the frame_parallel block of the --full line")
            if fp_leg is not None:
                res["frame_parallel"] = fp_leg
        if dry:
            res["data"] = "DRY RUN on CPU (gloo + tests/_cpu_backend.py): orchestration check, NOT a measurement"
        full = (args.vit_depth, args.qformer_layers, args.llm_layers, T) == (39, 12, 32, conf["frames"])
        if not full:
            res["config"]["workload"] += "  [REDUCED — not the BASELINE config; for debugging only]"
        if parity is not None:
            res["parity"] = dict(parity, dtype=args.dtype, tolerance_target="north_star: logits within 1e-2 (met by the fp32 verify leg; the 16-bit "
                                 "legs are reported with their measured gap next to the reference's own, see reference_own_gap)",
                                 reference_own_gap=REFERENCE_OWN_GAP)
            if extra_legs is not None:
                res["fp16"] = extra_legs["fp16"]
                res["parity"]["fp32_verify"] = extra_legs["fp32"]
                # the split verify mode (round 4): fp32 activations / norms / attention, every Linear as three bf16 matrix-core products of
                # split operands (stllm_hip.h STLLM_BF16X3) — the tolerance-meeting mode that is not 9.6x slower
                res["parity"]["split_verify"] = dict(extra_legs["bf16x3"], mode="bf16x3", vs_timed_dtype=round(extra_legs["bf16x3"]["ms_per_step"] / (single_stream["ms_per_step"] if single_stream else ms_per_step), 2))   # (the legs run one clip at a time: against the single-stream rate)
                # "mixed" (round 5): the split mode with the ViT blocks in fp16 — the cheapest combination of the per-stage ladder that stays under the
                # north star's 1e-2 on c2 (profiles/r04_parity_ladder.log) — c3 9.8e-3, c4 1.02e-2: AT the bar, not under it, which is why split_verify stays the reference verify mode
                res["parity"]["mixed_verify"] = dict(extra_legs["mixed"], mode="mixed: ViT fp16, Q-Former + projector + Llama + lm_head bf16x3",
                                                     vs_timed_dtype=round(extra_legs["mixed"]["ms_per_step"] / (single_stream["ms_per_step"] if single_stream else ms_per_step), 2))
        if projection is not None:
            res["frame_parallel_projection"] = projection
        if target_summary is not None:
            s = target_summary
            avg_ms = s["total_ms"] / s["launches"]
            ach = s["flops"] / (s["total_ms"] * 1e-3) / 1e12
            res["roofline"] = {"bound": "mfma", "kernel": prof.target, "achieved": round(ach, 1), "peak": MFMA_PEAK[args.dtype],
                               "unit": "TFLOP/s", "frac": round(ach / MFMA_PEAK[args.dtype], 4), "traffic": load_traffic(prof.target),
                               "launches_timed": s["launches"], "sampled_every": hip.GemmProfiler.SAMPLE_EVERY, "avg_launch_ms": round(avg_ms, 5),
                               **({"measured_in": "the single_stream bracket (the kernel alone on the chip: its own duration)",
                                   "with_clips_in_flight": {"note": "the same symbol sampled inside the headline bracket: an event pair around one launch also times the other "
                                                                    "stream's workgroups that share the chip with it",
                                                            "launches_timed": inflight_summary["launches"],
                                                            "avg_launch_ms": round(inflight_summary["total_ms"] / inflight_summary["launches"], 5),
                                                            "achieved": round(inflight_summary["flops"] / (inflight_summary["total_ms"] * 1e-3) / 1e12, 1)}}
                                  if inflight_summary is not None else {}),
                               "algorithmic_gflop_per_launch": round(s["flops"] / s["launches"] / 1e9, 2),
                               # the symbol serves more than one GEMM shape (ViT proj K = 1408 and fc2 K = 6144): each on its own
                               "per_shape": {k: {"launches": v["launches"], "avg_launch_ms": round(v["total_ms"] / v["launches"], 5),
                                                 "achieved": round(v["flops"] / (v["total_ms"] * 1e-3) / 1e12, 1),
                                                 "frac": round(v["flops"] / (v["total_ms"] * 1e-3) / 1e12 / MFMA_PEAK[args.dtype], 4)}
                                             for k, v in sorted(s["shapes"].items())},
                               # every GEMM (symbol, shape) that costs >= 1 ms per step, from the calibration step (events around EVERY launch: each launch
                               # carries ~1 us of event overhead, so these fractions read a little low against the sampled `per_shape` above)
                               "per_shape_all_ge_1ms": {f"{k} @ {shp}": {"launches": v2["launches"], "ms_per_step": round(v2["total_ms"], 3),
                                                                          "avg_launch_us": round(v2["total_ms"] / v2["launches"] * 1e3, 2),
                                                                          "achieved": round(v2["flops"] / (v2["total_ms"] * 1e-3) / 1e12, 1),
                                                                          "frac": round(v2["flops"] / (v2["total_ms"] * 1e-3) / 1e12 / MFMA_PEAK[args.dtype], 4)}
                                                        for k, v in sorted(cal.items(), key=lambda kv: -kv[1]["total_ms"])
                                                        for shp, v2 in sorted(v["shapes"].items(), key=lambda kv: -kv[1]["total_ms"]) if v2["total_ms"] >= 1.0},
                               "all_gemm_kernels_one_step": {k: {"launches": v["launches"], "ms": round(v["total_ms"], 3),
                                                                 "tflops": round(v["flops"] / max(v["total_ms"], 1e-9) / 1e9, 1)}
                                                             for k, v in sorted(cal.items(), key=lambda kv: -kv[1]["total_ms"])}}
        if not args.no_cpu_baseline and world == 1:   # reported baseline: rank 0, N=1 only
            res["cpu_baseline"] = cpu_baseline(T, S)
        print(json.dumps(res), flush=True)

    import threading
    emit_lock, emitted = threading.Lock(), [False]

    def emit(fp_leg):
        """rank 0 prints THE line (once)"""
        with emit_lock:
            if emitted[0] or rank != 0:
                return
            emitted[0] = True
        _emit(fp_leg)

    if world > 1 and args.config == "c2" and not args.no_frame_parallel:
        del model, out
        sm = None
        if not dry:
            torch.cuda.empty_cache()
        # The c3 block is the one part of this run that has NEVER executed on a multi-GPU node (RCCL point-to-point inside clip teams, kernels of two
        # processes sharing links): it must not be able to take the headline measurement — already complete at this point — down with it.  A Python
        # error becomes {"error": ...} in the line; a hang is cut by a watchdog that prints the line without the block and ends the process.
        fp_done = threading.Event()

        def watchdog():
            if not fp_done.wait(args.fp_timeout):
                emit({"error": f"the frame_parallel block did not finish within {args.fp_timeout} s (cut by bench.py's watchdog; the headline above is unaffected)"})
                sys.stdout.flush()
                os._exit(0)
        threading.Thread(target=watchdog, daemon=True).start()
        try:
            fp_leg = frame_parallel_leg(args, world, rank, device, dry, sync)
        except Exception as ex:   # noqa: BLE001 — reported, not raised: see above (peers still inside a collective end through their own watchdogs)
            fp_leg = {"error": f"{type(ex).__name__}: {ex}"}
        fp_done.set()
        sm = None
    emit(fp_leg)



def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)     # long enough for the driver's SMI sampler to see the timed window
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--config", default="c2", choices=sorted(CONFIGS))
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32", "bf16x3", "mixed"])
    ap.add_argument("--frames", type=int, default=0, help="override the config's frames per clip (debugging)")
    ap.add_argument("--vit-depth", type=int, default=39)
    ap.add_argument("--qformer-layers", type=int, default=12)
    ap.add_argument("--llm-layers", type=int, default=32)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--vit-streams", type=int, default=1)
    ap.add_argument("--streams", type=int, default=2, help="N = 1: clips in flight — step k is enqueued on HIP stream k %% streams (default 2: two independent B = 1 steps share the chip; "
                                                            "1 = one step after the other on the current stream, also timed after the headline bracket as `single_stream`)")
    ap.add_argument("--no-extra-legs", action="store_true", help="N = 1: skip the fp16 and fp32-verify legs after the timed region")
    ap.add_argument("--no-frame-parallel", action="store_true", help="N > 1: skip the c3 frame-parallel strong-scaling block")
    ap.add_argument("--no-projection", action="store_true", help="N = 1: skip the frame_parallel_projection block (c3 and its per-rank shares on this GPU)")
    ap.add_argument("--fp-steps", type=int, default=30, help="timed steps of the c3 block on N ranks (at least 30: pipeline fill / drain < 2 % of the bracket)")
    ap.add_argument("--fp-timeout", type=float, default=300.0, help="N > 1: seconds the c3 frame_parallel block may take before the watchdog prints the line without it")
    ap.add_argument("--fp-clips", type=int, default=0, help="override the c3 block's clips per batch (debugging / dry runs: 1 clip on 2 ranks = one team of two)")
    ap.add_argument("--fp-steps-1gpu", type=int, default=3, help="timed steps of the c3 block's 1-GPU reference (rank 0 alone)")
    ap.add_argument("--dry-cpu", action="store_true", help="run the rank logic on CPU (gloo, contract backend): plumbing check only")
    ap.add_argument("--full", action="store_true", help="also run every other measurement and check (parity, roofline, telemetry, single-stream bracket, "
                                                        "numerics legs, frame-parallel blocks, CPU baseline); off: the headline only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the last timed step's outputs to DIR/<name>.npy (rank 0)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if not args.full:   # a plain run times the headline and nothing else
        args.no_roofline = args.no_cpu_baseline = args.no_extra_legs = args.no_projection = args.no_frame_parallel = True
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(spawn_ranks(args))
    run_rank(args)


if __name__ == "__main__":
    main()
