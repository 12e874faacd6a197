#!/usr/bin/env python3
"""Decode latency of the KV-cache path: prefill S=576, then one-token steps.  GPU only.
HBM floor for Vicuna-7B in bf16: 13.5 GB of weights per token / ~6.3 TB/s achievable = 2.1 ms."""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--llm-layers", type=int, default=32)
ap.add_argument("--vit-depth", type=int, default=1)
ap.add_argument("--qformer-layers", type=int, default=1)
ap.add_argument("--tokens", type=int, default=16)
ap.add_argument("--rows", type=int, default=1, help="sequences decoded together (5 = demo.py's beam search)")
ap.add_argument("--weights", choices=["16", "int8", "int4g128"], default="16",
                help="decode weights: the 16-bit pack, its int8 copy on the W8A16 kernels, or its 4-bit copy on the W4A16 kernels (runtime.set_decode_weights)")
ap.add_argument("--gemv", type=int, default=-1, help="stllm_set_option('gemm_gemv'): -1 default (M <= 8), 1 = M <= 4, 0 off")
ap.add_argument("--attn-single", type=int, default=1, help="stllm_set_option('attn_decode_single')")
ap.add_argument("--ragged", default="", help="L1,L2,...: time ragged steps at these per-row cache lengths against uniform steps with every row at max(L), alternating")
ap.add_argument("--questions", default="", help="L1,L2,...: N questions of these lengths behind one prefilled 576-token prefix — generate(batching='ragged') in one "
                                                "batch against one generate() per question (what a padded batch behind a prefix costs without the ragged cache)")
ap.add_argument("--share-prefix", action="store_true", help="with --questions or --beams: generate(share_prefix=True) against share_prefix=False (private copies), "
                                                          "alternating; tokens/s and peak memory_allocated of both")
ap.add_argument("--beams", type=int, default=0, help="with --share-prefix: one prompt of --prefix-len + 24 positions, this many beams (5 = demo.py); "
                                                    "with --generate: num_beams of one prompt; with --serve N,K: every question searches this many beams "
                                                    "(serving.Engine(num_beams=...), DESIGN.md §4.2k; see --serve)")
ap.add_argument("--generate", type=int, default=0, help="N: end-to-end generate() of N new tokens per row behind a 576-position prompt (--rows prompts, or one prompt x --beams), "
                                                       "tokens/s, and the selection step alone in us by device events, on the logits of that prompt")
ap.add_argument("--selection", choices=["torch", "device", "both"], default="both", help="with --generate: the selection mode; 'both' alternates them, 3 repeats each")
ap.add_argument("--sample", action="store_true", help="with --generate: top-p sampling (top_p 0.9, temperature 0.8) instead of greedy search")
ap.add_argument("--cases", default="", help="with --generate: several workloads in one process (one model build), e.g. g1,g5,g16,s1,s16,b5 — g / s = greedy / sampled "
                                            "rows, b = beams of one prompt; default: the one case --rows / --sample / --beams describe")
ap.add_argument("--sync-every", type=int, default=1, help="with --generate, selection 'device': generate(sync_every=K)")
ap.add_argument("--serve", default="", help="N,K: N questions behind one prefilled --prefix-len prefix through K slots of serving.Engine (continuous batching) against "
                                            "generate(batching='ragged') in waves of K; mixed answer lengths (printed), EOS disabled, useful tokens/s of both.  "
                                            "With --beams nb > 1 the run is the beam comparison instead: the Engine(num_beams=nb) in both states (and, with "
                                            "--share-base, with base=prefix as well) against generate(num_beams=nb) one question at a time and in waves of K, "
                                            "alternating, one warm-up and three runs each, and the kv_reorder_rows launch alone against the index_select "
                                            "assignment; --state is ignored there")
ap.add_argument("--state", choices=["host", "device", "both"], default="host", help="with --serve: serving.Engine(state=...); 'both' alternates the host-state and the "
                "device-state Engine in one process (one warm-up and three runs each, no waves) and times the hip.select_slots launch alone")
ap.add_argument("--share-base", action="store_true", help="with --serve: serving.Engine(base=prefix) (the slots read ONE copy of the prefix, DESIGN.md §4.2j) against "
                "the copying Engine (KVCache.load_row per admission), alternating in one process, one warm-up and three runs each, with --state host, device or both; "
                "prints peak torch.cuda.max_memory_allocated of every run as well")
ap.add_argument("--admit", default="", help="R,n: the whole admission step — R running rows behind 560 .. 1100 positions plus one admitted n-token row: "
                                            "LlamaModel.step_segments against extend(lengths=[0] * R + [n]) followed by a decode_step, alternating")
ap.add_argument("--prefix-len", type=int, default=576, help="positions of the shared prefix of --share-prefix")
args = ap.parse_args()
torch.set_grad_enabled(False)
dev = torch.device("cuda:0")
model = bench.build_model(dev, args)
lm = model.model
S = 576
from stllm_amd import hip
from stllm_amd import runtime
runtime.set_decode_weights(None if args.weights == "16" else args.weights)
hip.set_option("gemm_gemv", args.gemv)
hip.set_option("attn_decode_single", args.attn_single)


def ragged_steps(lens):
    """ms per step, ragged cache at `lens` vs uniform cache with every row at max(lens): blocks of `--tokens` steps, alternating, 5 blocks each, medians.
    Every step is undone (truncate) so that each one runs at the same lengths."""
    R, L = len(lens), max(lens)
    e = (torch.randn(R, L, 4096, device=dev) * 0.02)
    uni = lm.new_cache(R, L + 8, dev)
    lm.prefill(e, None, cache=uni)
    rag = uni.fork()
    rag.truncate(list(lens))
    if rag.lens is None:
        rag.lens = list(lens)
    tok = torch.randn(R, 1, 4096, device=dev) * 0.02

    def block(cache, keep):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.tokens):
            _, h = lm.decode_step(tok, cache)
            model.logits_from(h, R, 1)
            cache.truncate(keep)
            if isinstance(keep, list) and cache.lens is None:
                cache.lens = list(keep)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.tokens * 1e3
    for _ in range(2):
        block(uni, L), block(rag, list(lens))
    tu, tr = [], []
    for _ in range(5):
        tu.append(block(uni, L))
        tr.append(block(rag, list(lens)))
    mu, mr = sorted(tu)[2], sorted(tr)[2]
    print(f"ragged decode ({R} rows, lens {','.join(map(str, lens))}, weights {args.weights}): uniform@{L} {mu:.3f} ms/step (blocks {' '.join(f'{x:.3f}' for x in tu)}), "
          f"ragged {mr:.3f} ms/step (blocks {' '.join(f'{x:.3f}' for x in tr)}), ragged - uniform {mr - mu:+.3f} ms = {(mr - mu) / len(lm.layers) * 1e3:+.1f} us/layer")


def questions_e2e(lens):
    """tokens/s of N questions behind one prefilled prefix: one ragged batch vs one generate() per question; eos disabled so that both emit N x tokens ids"""
    N, P = len(lens), 576
    video = torch.randn(1, P, 4096, device=dev) * 0.02
    prefix = lm.new_cache(1, P, dev)
    lm.prefill(video, None, cache=prefix)
    qs = [torch.randn(n, 4096, device=dev) * 0.02 for n in lens]
    emb = torch.zeros(N, max(lens), 4096, device=dev)
    mask = torch.zeros(N, max(lens), dtype=torch.long)
    for i, q in enumerate(qs):
        emb[i, :lens[i]] = q
        mask[i, :lens[i]] = 1
    kw = dict(max_new_tokens=args.tokens, eos_token_id=None, prefix_cache=prefix)

    def one_batch():
        return model.generate(inputs_embeds=emb, attention_mask=mask, batching="ragged", **kw)

    def per_question():
        return [model.generate(inputs_embeds=q[None], **kw) for q in qs]
    res = {}
    for name, f in (("ragged", one_batch), ("per-question", per_question)) * 3:   # alternating; the first round warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        res.setdefault(name, []).append(time.perf_counter() - t0)
    for name, ts in res.items():
        t = min(ts[1:])
        print(f"{N} questions (lens {','.join(map(str, lens))}) behind a {P}-token prefix, {args.tokens} new tokens each [{name}]: {t * 1e3:.1f} ms "
              f"= {N * args.tokens / t:.1f} tok/s (runs {' '.join(f'{x * 1e3:.1f}' for x in ts)})")


def share_prefix_e2e(lens, beams):
    """generate() with share_prefix off / on, alternating, 3 runs each (the first warms up): N questions of `lens` behind one prefilled prefix in one ragged
    batch, or (beams) one whole prompt with that many beams — there the prompt's own cache is the base.  eos disabled: both emit the same number of ids."""
    P = args.prefix_len
    video = torch.randn(1, P, 4096, device=dev) * 0.02
    if beams:
        kw = dict(inputs_embeds=torch.cat([video, torch.randn(1, 24, 4096, device=dev) * 0.02], dim=1), num_beams=beams)
        what, n_tok = f"{beams} beams behind {P + 24} prompt positions", args.tokens
    else:
        prefix = lm.new_cache(1, P, dev)
        lm.prefill(video, None, cache=prefix)
        N = len(lens)
        emb = torch.zeros(N, max(lens), 4096, device=dev)
        mask = torch.zeros(N, max(lens), dtype=torch.long)
        for i, n in enumerate(lens):
            emb[i, :n] = torch.randn(n, 4096, device=dev) * 0.02
            mask[i, :n] = 1
        kw = dict(inputs_embeds=emb, attention_mask=mask, batching="ragged", prefix_cache=prefix)
        what, n_tok = f"{N} questions (lens {','.join(map(str, lens))}) behind a {P}-token prefix", N * args.tokens
    res, peak = {}, {}
    for share in (False, True) * 3:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        m0 = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        model.generate(max_new_tokens=args.tokens, eos_token_id=None, share_prefix=share, **kw)
        torch.cuda.synchronize()
        res.setdefault(share, []).append(time.perf_counter() - t0)
        peak[share] = torch.cuda.max_memory_allocated() - m0
    for share, ts in res.items():
        t = min(ts[1:])
        print(f"{what}, {args.tokens} new tokens, weights {args.weights} [share_prefix={share}]: {t * 1e3:.1f} ms = {n_tok / t:.1f} tok/s "
              f"(runs {' '.join(f'{x * 1e3:.1f}' for x in ts)}), peak memory above the model + prefix {peak[share] / 1e6:.0f} MB", flush=True)


def generate_e2e(n_new, R, nb, sample):
    """generate() end to end with torch / device selection, alternating, 3 repeats each behind one warm-up each; EOS disabled so that every run emits the
    same number of ids; repetition penalty 1.5 as Chat.answer forces it.  Then the selection step alone on this prompt's first logits: the torch chain
    generate() runs today against the kernel, 50 launches each between two device events."""
    from stllm_amd import generation as G
    B = 1 if nb else R
    emb = torch.randn(B, S, 4096, device=dev) * 0.02
    kw = dict(inputs_embeds=emb, max_new_tokens=n_new, eos_token_id=None, repetition_penalty=1.5, num_beams=max(nb, 1))
    if sample:
        kw.update(do_sample=True, top_p=0.9, temperature=0.8)
    modes = ["torch", "device"] if args.selection == "both" else [args.selection]
    what = f"{nb} beams" if nb else f"{R} rows, {'sample' if sample else 'greedy'}"
    res = {}
    for rep in range(4):
        for mode in modes:
            extra = dict(selection=mode, sync_every=args.sync_every) if mode == "device" else {}
            gen = torch.Generator(device=dev).manual_seed(rep) if sample else None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = model.generate(generator=gen, **kw, **extra)
            torch.cuda.synchronize()
            res.setdefault(mode, []).append(time.perf_counter() - t0)
            assert out.shape[1] == n_new
    rows = B * max(nb, 1)
    for mode, ts in res.items():
        t = sorted(ts[1:])[1]
        print(f"generate ({what}, weights {args.weights}, {n_new} new tokens, selection {mode}{f', sync_every {args.sync_every}' if mode == 'device' else ''}): "
              f"median {t * 1e3:.1f} ms = {t / n_new * 1e3:.3f} ms/token = {B * n_new / t:.1f} tok/s (runs {' '.join(f'{x * 1e3:.1f}' for x in ts[1:])}; warm-up {ts[0] * 1e3:.1f})", flush=True)
    # the selection step alone, same logits for both: a padded-row view as logits_from returns it, 40 previous ids
    _, h16 = lm.prefill(emb, None, cache=lm.new_cache(B, S, dev))
    logits = model.logits_from(h16.view(B, S, -1)[:, -1].contiguous(), B, 1)[:, 0]
    if nb:
        logits = logits.repeat_interleave(nb, dim=0)
    V = logits.shape[1]
    prev = torch.randint(0, V, (rows, 64), device=dev, dtype=torch.int32)
    ids, n_prev = prev[:, :40].long(), 40
    bs = torch.linspace(0, -3, rows, device=dev)
    out, u = torch.empty(rows, dtype=torch.int32, device=dev), torch.rand(rows, device=dev)

    def torch_chain():
        if nb:
            lp = G._process_logits(logits.log_softmax(dim=-1), ids, n_prev, 1.5, 0, 2)
            return torch.topk((lp + bs[:, None]).view(B, nb * V), 2 * nb, dim=1, largest=True, sorted=True)
        sc = G._process_logits(logits, ids, n_prev, 1.5, 0, 2)
        if sample:
            return torch.multinomial(G._warp_logits(sc, 0.8, 0.9).softmax(dim=-1), num_samples=1)
        return sc.argmax(dim=-1)

    def kernel():
        if nb:
            return hip.beam_candidates(logits, bs, 2 * nb, prev=prev, n_prev=n_prev, penalty=1.5, eos_id=2)
        return hip.select_tokens(logits, out, prev=prev, n_prev=n_prev, penalty=1.5, eos_id=2, sample=sample, temperature=0.8, top_p=0.9, u=u)
    for name, f in (("torch chain", torch_chain), ("kernel", kernel)):
        us = []
        for _ in range(3):
            for _ in range(5):
                f()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(50):
                f()
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) / 50 * 1e3)
        print(f"selection step alone ({what}, V {V}, n_prev {n_prev}) [{name}]: {sorted(us)[1]:.1f} us (blocks {' '.join(f'{x:.1f}' for x in us)})", flush=True)


SERVE_LENGTHS = [16, 96, 32, 64, 24, 128, 48, 8]   # answer lengths of --serve, cycled over the N questions


def serve_e2e(N, K):
    """useful tokens/s: Engine (a slot is refilled the step after its answer ends) vs waves of K questions, each wave one ragged generate() that lasts as long as
    its longest answer (what the rows that finished earlier cost while they are fed pad tokens).  Alternating, 3 runs each, the first warms up."""
    from stllm_amd import serving
    P = args.prefix_len
    video = torch.randn(1, P, 4096, device=dev) * 0.02
    prefix = lm.new_cache(1, P, dev)
    lm.prefill(video, None, cache=prefix)
    qlens = [9 + (5 * i) % 17 for i in range(N)]
    alens = [SERVE_LENGTHS[i % len(SERVE_LENGTHS)] for i in range(N)]
    qs = [torch.randn(n, 4096, device=dev) * 0.02 for n in qlens]

    def engine(state=args.state, share=False):
        eng = serving.Engine(model, K, P + max(qlens) + max(alens), eos_token_id=None, repetition_penalty=1.5, **({"state": state} if state != "host" else {}),
                             **({"base": prefix} if share else {}))
        for q, n in zip(qs, alens):
            eng.submit(q, prefix=prefix, max_new_tokens=n)
        out = eng.run()
        assert sorted(ids.numel() for _, ids in out) == sorted(alens)
        return eng.steps

    def waves():
        for w in range(0, N, K):
            rows, n_new = qs[w:w + K], max(alens[w:w + K])
            emb = torch.zeros(len(rows), max(q.shape[0] for q in rows), 4096, device=dev)
            mask = torch.zeros(emb.shape[:2], dtype=torch.long)
            for i, q in enumerate(rows):
                emb[i, :q.shape[0]] = q
                mask[i, :q.shape[0]] = 1
            model.generate(inputs_embeds=emb, attention_mask=mask, batching="ragged", prefix_cache=prefix, max_new_tokens=n_new, eos_token_id=None,
                           repetition_penalty=1.5)
    if args.share_base:
        return serve_share_base(N, K, P, alens, engine)
    if args.state == "both":
        return serve_states(N, K, P, alens, engine)
    res, steps = {}, None
    for name, f in (("engine", engine), ("waves", waves)) * 3:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        res.setdefault(name, []).append(time.perf_counter() - t0)
        steps = r if name == "engine" else steps
    wave_steps = sum(max(alens[w:w + K]) for w in range(0, N, K))
    for name, ts in res.items():
        t = min(ts[1:])
        extra = f"{steps['segments']} admission + {steps['decode']} decode steps" if name == "engine" else f"{wave_steps} decode steps in {-(-N // K)} waves"
        print(f"{N} questions over {K} slots behind a {P}-token prefix, answers {','.join(map(str, alens))} ({sum(alens)} tokens), weights {args.weights} [{name}]: "
              f"{t * 1e3:.1f} ms = {sum(alens) / t:.1f} useful tok/s, {extra} (runs {' '.join(f'{x * 1e3:.1f}' for x in ts)})", flush=True)


def serve_beams(N, K, nb):
    """--serve N,K --beams nb: §4.2h's workload with nb beams per question.  Alternating in one process, one warm-up and three runs each:
    (a) serving.Engine(num_beams=nb) in both states (with --share-base also Engine(base=prefix)), (b) generate(num_beams=nb) one question at a time,
    (c) generate(num_beams=nb, batching="ragged") in waves of K questions.  Then the re-order kernel alone against the index_select assignment of
    _CacheStepper.advance: nb rows, --llm-layers layer buffers, spans of 16 and 256 positions, device events around blocks of 20 re-orders."""
    from stllm_amd import serving
    P = args.prefix_len
    video = torch.randn(1, P, 4096, device=dev) * 0.02
    prefix = lm.new_cache(1, P, dev)
    lm.prefill(video, None, cache=prefix)
    qlens = [9 + (5 * i) % 17 for i in range(N)]
    alens = [SERVE_LENGTHS[i % len(SERVE_LENGTHS)] for i in range(N)]
    qs = [torch.randn(n, 4096, device=dev) * 0.02 for n in qlens]
    kw = dict(eos_token_id=None, repetition_penalty=1.5, num_beams=nb)
    steps = {}

    def engine(state, share):
        eng = serving.Engine(model, K, P + max(qlens) + max(alens), state=state, **({"base": prefix} if share else {}), **kw)
        for q, n in zip(qs, alens):
            eng.submit(q, prefix=prefix, max_new_tokens=n)
        out = eng.run()
        assert sorted(ids.numel() for _, ids in out) == sorted(alens)
        steps[(state, share)] = dict(eng.steps)

    def one_at_a_time():
        for q, n in zip(qs, alens):
            model.generate(inputs_embeds=q[None], prefix_cache=prefix, max_new_tokens=n, **kw)

    def waves():
        for w in range(0, N, K):
            rows, n_new = qs[w:w + K], max(alens[w:w + K])
            emb = torch.zeros(len(rows), max(q.shape[0] for q in rows), 4096, device=dev)
            mask = torch.zeros(emb.shape[:2], dtype=torch.long)
            for i, q in enumerate(rows):
                emb[i, :q.shape[0]] = q
                mask[i, :q.shape[0]] = 1
            model.generate(inputs_embeds=emb, attention_mask=mask, batching="ragged", prefix_cache=prefix, max_new_tokens=n_new, **kw)
    runs = [(f"engine state={st} {'base=prefix' if sh else 'copies'}", (lambda st=st, sh=sh: engine(st, sh)))
            for st in ("host", "device") for sh in ((False, True) if args.share_base else (False,))]
    runs += [(f"generate(num_beams={nb}) one question at a time", one_at_a_time), (f"generate(num_beams={nb}) in waves of {K}", waves)]
    res = {}
    for name, f in runs * 4:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        res.setdefault(name, []).append(time.perf_counter() - t0)
    for name, ts in res.items():
        t = sorted(ts[1:])[1]
        print(f"{N} questions x {nb} beams over {K} slots ({K * nb} rows) behind a {P}-token prefix, answers {','.join(map(str, alens))} ({sum(alens)} tokens), "
              f"weights {args.weights} [{name}]: median {t * 1e3:.1f} ms = {sum(alens) / t:.1f} useful tok/s (warm-up {ts[0] * 1e3:.1f}, runs "
              f"{' '.join(f'{x * 1e3:.1f}' for x in ts[1:])})", flush=True)
    print("engine steps:", {f"{st} {'base' if sh else 'copies'}": s for (st, sh), s in steps.items()}, flush=True)
    # the re-order alone: one request's nb rows, a cycle (every row moves), all layer buffers
    L = args.llm_layers
    for span in (16, 256):
        cap = 64 + span
        bufs = [torch.randn(nb, cap, 3 * 4096, device=dev).to(torch.bfloat16) for _ in range(L)]
        perm = [(i + 1) % nb for i in range(nb)]
        src, idx = torch.tensor(perm, dtype=torch.int32, device=dev), torch.tensor(perm, device=dev)
        lo, hi = torch.tensor([64], dtype=torch.int32, device=dev), torch.tensor([cap], dtype=torch.int32, device=dev)

        def kernel():
            for b in bufs:
                hip.kv_reorder_rows(b, src, lo, hi, nb=nb, max_span=span)

        def index_select():
            for b in bufs:
                b[:, :cap] = b[:, :cap].index_select(0, idx)
        us = {}
        for name, f in (("kv_reorder_rows", kernel), ("index_select assignment", index_select)) * 3:
            f()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                f()
            e1.record()
            e1.synchronize()
            us.setdefault(name, []).append(e0.elapsed_time(e1) / 20 * 1e3)
        for name, v in us.items():
            print(f"re-order alone, {nb} rows, {L} layers, bf16, span {span} of {cap} positions [{name}]: {sorted(v)[1]:.1f} us per re-order of all layers "
                  f"(blocks {' '.join(f'{x:.1f}' for x in v)})", flush=True)


def serve_share_base(N, K, P, alens, engine):
    """the copying Engine against Engine(base=prefix) on the same requests, per state: alternating, one warm-up and three runs each; wall time, useful tokens/s,
    step counts and the peak of torch.cuda.max_memory_allocated over each run (the model, the prefix and the requests are allocated before and count in both)"""
    states = ("host", "device") if args.state == "both" else (args.state,)
    res, steps, peak = {}, {}, {}
    for key in [(st, sh) for st in states for sh in (False, True)] * 4:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        steps[key] = engine(key[0], share=key[1])
        torch.cuda.synchronize()
        res.setdefault(key, []).append(time.perf_counter() - t0)
        peak[key] = max(peak.get(key, 0), torch.cuda.max_memory_allocated())
    print(f"allocated before any Engine (model, prefix, requests): {torch.cuda.memory_allocated() / 2 ** 20:.0f} MiB", flush=True)
    for (st, sh), ts in res.items():
        t = sorted(ts[1:])[1]
        print(f"{N} questions over {K} slots behind a {P}-token prefix, answers {','.join(map(str, alens))} ({sum(alens)} tokens), weights {args.weights} "
              f"[engine state={st} {'base=prefix' if sh else 'copies'}]: median {t * 1e3:.1f} ms = {sum(alens) / t:.1f} useful tok/s, "
              f"{steps[(st, sh)]['segments']} admission + {steps[(st, sh)]['decode']} decode steps, peak allocated {peak[(st, sh)] / 2 ** 20:.0f} MiB "
              f"(warm-up {ts[0] * 1e3:.1f}, runs {' '.join(f'{x * 1e3:.1f}' for x in ts[1:])})", flush=True)


def serve_states(N, K, P, alens, engine):
    """the host-state against the device-state Engine on the same requests: alternating, one warm-up and three runs each; then the select_slots launch alone
    (K slots, a 32000-column row each, 64 ids of history, repetition penalty 1.5) in 3 blocks of 50 launches between events"""
    res, steps = {}, {}
    for state in ("host", "device") * 4:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps[state] = engine(state)
        torch.cuda.synchronize()
        res.setdefault(state, []).append(time.perf_counter() - t0)
    for state, ts in res.items():
        t = sorted(ts[1:])[1]
        print(f"{N} questions over {K} slots behind a {P}-token prefix, answers {','.join(map(str, alens))} ({sum(alens)} tokens), weights {args.weights} "
              f"[engine state={state}]: median {t * 1e3:.1f} ms = {sum(alens) / t:.1f} useful tok/s, {steps[state]['segments']} admission + "
              f"{steps[state]['decode']} decode steps (warm-up {ts[0] * 1e3:.1f}, runs {' '.join(f'{x * 1e3:.1f}' for x in ts[1:])})", flush=True)
    V, n_gen = 32000, 64
    logits = torch.randn(K, V, device=dev) * 4
    src = torch.arange(K, dtype=torch.int32, device=dev)
    ids = torch.randint(0, V, (K, max(alens)), device=dev).to(torch.int32)
    state0 = torch.tensor([[1, n_gen, 10 ** 6, 0]] * K, dtype=torch.int32, device=dev)
    us = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st = state0.clone()
        e0.record()
        for _ in range(50):
            hip.select_slots(logits, src, st, ids, penalty=1.5)
            st[:, 1] = n_gen                       # (one tiny fill per launch keeps every launch at the same history length)
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) / 50 * 1e3)
    print(f"select_slots launch alone (greedy, {K} slots, V {V}, n_gen {n_gen}, + one 4-byte-per-slot fill): {sorted(us)[1]:.1f} us "
          f"(blocks {' '.join(f'{x:.1f}' for x in us)})", flush=True)


def admit_step(R, n):
    """ms of one admission step, alternating blocks of --tokens steps, 5 blocks each, medians; every step is undone (truncate)"""
    lens = [560 + (540 * i) // max(R - 1, 1) for i in range(R)]
    L = max(lens) + n + 8
    c = lm.new_cache(R + 1, L, dev)
    lm.prefill(torch.randn(R + 1, max(lens), 4096, device=dev) * 0.02, None, cache=c)
    keep = lens + [0]
    c.truncate(keep)
    tok = torch.randn(R, 4096, device=dev) * 0.02
    new = torch.randn(n, 4096, device=dev) * 0.02
    packed = torch.cat([tok, new])
    pad = torch.zeros(R + 1, n, 4096, device=dev)
    pad[R] = new
    tok16 = torch.randn(R + 1, 1, 4096, device=dev) * 0.02

    def seg():
        _, h = lm.step_segments(packed, c, [(r, 1) for r in range(R)] + [(R, n)])
        model.logits_from(h, R + 1, 1)
        c.truncate(keep)

    def parent():
        lm.extend(pad, c, lengths=[0] * R + [n])
        _, h = lm.decode_step(tok16, c)
        model.logits_from(h, R + 1, 1)
        c.truncate(keep)

    def block(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.tokens):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.tokens * 1e3
    for _ in range(2):
        block(seg), block(parent)
    ts, tp = [], []
    for _ in range(5):
        ts.append(block(seg))
        tp.append(block(parent))
    print(f"admission step ({R} running rows behind {lens[0]} .. {lens[-1]} positions + one {n}-token row): step_segments {sorted(ts)[2]:.3f} ms "
          f"(blocks {' '.join(f'{x:.3f}' for x in ts)}), extend(n_b = 0 for the running rows) + decode_step {sorted(tp)[2]:.3f} ms (blocks {' '.join(f'{x:.3f}' for x in tp)})"
          f" — the parent pair also decodes the admitted row's first token", flush=True)


if args.serve and args.beams:
    serve_beams(*[int(x) for x in args.serve.split(",")], args.beams)
    sys.exit(0)
if args.serve:
    serve_e2e(*[int(x) for x in args.serve.split(",")])
    sys.exit(0)
if args.admit:
    admit_step(*[int(x) for x in args.admit.split(",")])
    sys.exit(0)
if args.generate:
    cases = args.cases.split(",") if args.cases else [f"b{args.beams}" if args.beams else f"{'s' if args.sample else 'g'}{args.rows}"]
    for c in cases:
        generate_e2e(args.generate, 1 if c[0] == "b" else int(c[1:]), int(c[1:]) if c[0] == "b" else 0, c[0] == "s")
    sys.exit(0)
if args.share_prefix:
    share_prefix_e2e([int(x) for x in args.questions.split(",")] if args.questions else [], args.beams)
    sys.exit(0)
if args.ragged:
    ragged_steps([int(x) for x in args.ragged.split(",")])
    sys.exit(0)
if args.questions:
    questions_e2e([int(x) for x in args.questions.split(",")])
    sys.exit(0)
R = args.rows
emb = (torch.randn(1, S, 4096, device=dev) * 0.02).expand(R, S, 4096).contiguous()
cache = lm.new_cache(R, S + args.tokens + 8, dev)
hidden, h16 = lm.prefill(emb, None, cache=cache)
tok = torch.randn(R, 1, 4096, device=dev) * 0.02
for _ in range(3):
    lm.decode_step(tok, cache)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(args.tokens):
    _, h = lm.decode_step(tok, cache)
    logits = model.logits_from(h, R, 1)
torch.cuda.synchronize()
ms = (time.perf_counter() - t0) / args.tokens * 1e3
# bytes per weight of the decoder layers: 2 | 1 (+ a scale per row: negligible) | 0.5 + one fp32 scale per 128 weights; more than 16 rows stream the 16-bit weights
bpw = {"16": 2.0, "int8": 1.0, "int4g128": 0.5 + 4.0 / 128}[args.weights] if R <= 16 else 2.0
wbytes = sum(p.numel() for n, p in lm.named_parameters() if "layers" in n) * bpw + 32000 * 4096 * 2
wtag = "" if args.weights == "16" else f", weights {args.weights}"
print(f"decode ({R} rows{wtag}, gemm_gemv {args.gemv}, attn_single {args.attn_single}, fuse_norm_rows {os.environ.get('STLLM_DECODE_FUSE_ROWS', '2')}): {ms:.2f} ms/step ({1e3 / ms:.1f} tok/s), weights streamed per token {wbytes / 1e9:.2f} GB => {wbytes / ms / 1e9:.2f} TB/s")
