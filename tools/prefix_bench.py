"""Time per question on a video that is already uploaded, with and without a prefix KV cache (LlamaModel.extend) — one process, one GPU, synthetic
7B-size Llama weights, greedy decoding of a fixed number of tokens (no EOS), HIP-event / wall timings alternating between the three paths:

  (a) whole prompt   generate(inputs_embeds = video | question): prefill of Nv + Q positions on every question (the path Chat.answer always took)
  (b) prefix         generate(inputs_embeds = question, prefix_cache = video prefix): fork of the prefix + ONE extend pass over the Q positions
  (c) per-token      the prefix forked, the question appended by forward(past_key_values=...): one decode_step per question token

"first token" = until the logits of the last prompt position exist; "answer" = first token + max_new_tokens - 1 decode steps (host bookkeeping included).
Device clock / power over the whole timed region come from bench.py's Telemetry.

    python tools/prefix_bench.py [--layers 32] [--nv 512 2048] [--question 40] [--new 16] [--rounds 5] [--mode bf16]

--follow-up [--rows 4]: a follow-up round of N conversations in one ragged batch (Chat.follow_up's generate call) against re-prefilling every row's whole
history — N rows whose histories (video of --nv[0] tokens + earlier turns) have different lengths, a next turn of a different length per row:
  (a) re-prefill   generate(inputs_embeds = history | turn of every row, batching="ragged"): one ragged prefill of everything, on every turn
  (b) follow-up    generate(inputs_embeds = turn of every row, prefix_cache = the rows' ragged history cache, batching="ragged"): fork + ONE ragged extend
and the fork() copy of (b) on its own.
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--nv", type=int, nargs="+", default=[512, 2048])
    ap.add_argument("--question", type=int, default=40)
    ap.add_argument("--new", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--mode", default="bf16")
    ap.add_argument("--share-prefix", action="store_true", help="add (d): first token / answer with the prefix SHARED (KVCache.share, generate(share_prefix=True)) "
                                                                "instead of forked: no copy of the prefix rows, the shared-prefix attention kernels")
    ap.add_argument("--follow-up", action="store_true", help="time a follow-up round of --rows conversations against re-prefilling every row's whole history")
    ap.add_argument("--rows", type=int, default=4)
    a = ap.parse_args()
    import stllm_amd  # noqa: F401
    import bench
    from stllm_amd import runtime, synth
    from stllm_amd.models.st_llm import STLLMForCausalLM, StllmConfig
    torch.set_grad_enabled(False)
    runtime.set_compute_dtype(a.mode)
    m = STLLMForCausalLM(StllmConfig(num_hidden_layers=a.layers, max_position_embeddings=4096), device="cuda")
    synth.fill_module_(m, 0, "")
    lm = m.model
    Q, N = a.question, a.new
    q_emb = synth.normal_(torch.empty((1, Q, 4096), device="cuda"), "bench.question", 0, 0.05)
    kw = dict(max_new_tokens=N, num_beams=1, do_sample=False, eos_token_id=None)
    tele = bench.Telemetry(0).start()
    if a.follow_up:
        follow_up(a, m, kw, wall)
        print(f"\ntelemetry: {tele.stop()}")
        return
    rows = []
    for nv in a.nv:
        v_emb = synth.normal_(torch.empty((1, nv, 4096), device="cuda"), f"bench.video{nv}", 0, 0.05)
        whole = torch.cat([v_emb, q_emb], dim=1)
        prefix = lm.new_cache(1, nv, "cuda")
        t_prefill_video = wall(lambda: lm.prefill(v_emb, None, cache=prefix))

        def first_a():
            c = lm.new_cache(1, nv + Q + N, "cuda")
            _, h = lm.prefill(whole, None, cache=c)
            return m.logits_from(h.view(1, nv + Q, -1)[:, -1].contiguous(), 1, 1)

        def first_b():
            c = prefix.fork(max_len=nv + Q + N)
            _, h = lm.extend(q_emb, c)
            return m.logits_from(h.view(1, Q, -1)[:, -1].contiguous(), 1, 1)

        def first_c():
            c = prefix.fork(max_len=nv + Q + N)
            o = lm(inputs_embeds=q_emb, past_key_values=c)
            return m.logits_from(o._h16, 1, 1)

        ans_a = lambda: m.generate(inputs_embeds=whole, **kw)
        ans_b = lambda: m.generate(inputs_embeds=q_emb, prefix_cache=prefix, **kw)
        fns = dict(first_a=first_a, first_b=first_b, first_c=first_c, ans_a=ans_a, ans_b=ans_b)
        if a.share_prefix:
            def first_d():
                c = prefix.share(max_new=Q + N)
                _, h = lm.extend(q_emb, c)
                return m.logits_from(h.view(1, Q, -1)[:, -1].contiguous(), 1, 1)
            fns.update(first_d=first_d, ans_d=lambda: m.generate(inputs_embeds=q_emb, prefix_cache=prefix, share_prefix=True, **kw))
            fns["ans_d"]()
        ids_a, ids_b = ans_a(), ans_b()                       # warm-up of every path (packing, workspaces, allocator) + a sanity line
        first_c()
        same = int((ids_a == ids_b).sum())
        t = {k: [] for k in fns}
        for _ in range(a.rounds):                              # alternating: a, b, c, a, b, c, ...
            for k, fn in fns.items():
                t[k].append(wall(fn))
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        best = {k: min(v) for k, v in t.items()}
        rows.append((nv, t_prefill_video, med, best, same))
        print(f"[prefix_bench] Nv={nv} Q={Q} new={N}: " + "  ".join(f"{k} {med[k]:.2f} ms (best {best[k]:.2f})" for k in fns) +
              f"  | prefix ids == whole-prompt ids on {same}/{N} tokens (bf16: summation order differs)", flush=True)
    telemetry = tele.stop()
    props = torch.cuda.get_device_properties(0)
    print(f"\n# Prefix KV cache — {props.name}, {a.layers} layers, {a.mode}, question {Q} tokens, {N} new tokens, greedy, median of {a.rounds} alternating rounds "
          f"(best in brackets), wall clock around a synchronised call\n")
    print("| Nv | first token: whole prompt (a) | prefix + extend (b) | prefix + per-token loop (c) | answer: whole prompt (a) | prefix (b) | per-token (c), derived | one-off video prefill |")
    print("|---|---|---|---|---|---|---|---|")
    for nv, tv, med, best, same in rows:
        derived = med["first_c"] + (med["ans_a"] - med["first_a"])
        print(f"| {nv} | {med['first_a']:.2f} ({best['first_a']:.2f}) | {med['first_b']:.2f} ({best['first_b']:.2f}) | {med['first_c']:.2f} ({best['first_c']:.2f}) | "
              f"{med['ans_a']:.2f} ({best['ans_a']:.2f}) | {med['ans_b']:.2f} ({best['ans_b']:.2f}) | {derived:.2f} | {tv:.2f} |")
    print(f"\ntelemetry: {telemetry}")
    print("(c) answer = its first-token time + the decode steps of (a): the decode loop behind the first token is the same code for all three.")


def follow_up(a, m, kw, wall):
    from stllm_amd import synth
    lm = m.model
    B, nv, N = a.rows, a.nv[0], a.new
    hist = [nv + (60, 95, 130, 75, 110, 66, 142, 88)[b % 8] for b in range(B)]       # video + question + first answer, per row
    turn = [(12, 30, 8, 21, 40, 16, 9, 27)[b % 8] for b in range(B)]
    emb = synth.normal_(torch.empty((B, max(h + t for h, t in zip(hist, turn)), 4096), device="cuda"), "bench.dialogue", 0, 0.05)

    def padded(spans):
        L = max(n for _, n in spans)
        x = torch.zeros((B, L, 4096), device="cuda")
        for b, (first, n) in enumerate(spans):
            x[b, :n] = emb[b, first:first + n]
        return x, (torch.arange(L)[None, :] < torch.tensor([n for _, n in spans])[:, None]).long()   # (the mask stays on the host: no D2H read per call)
    h_emb, h_mask = padded([(0, h) for h in hist])
    cache = lm.new_cache(B, max(hist), "cuda")
    lm.prefill(h_emb, h_mask, cache=cache)                                            # the state a Dialogue holds between turns: a ragged cache
    assert cache.lens == hist
    w_emb, w_mask = padded([(0, h + t) for h, t in zip(hist, turn)])
    t_emb, t_mask = padded(list(zip(hist, turn)))
    room = max(hist) + max(turn) + N
    fns = dict(reprefill=lambda: m.generate(inputs_embeds=w_emb, attention_mask=w_mask, batching="ragged", **kw),
               follow_up=lambda: m.generate(inputs_embeds=t_emb, attention_mask=t_mask, prefix_cache=cache, batching="ragged", **kw),
               fork=lambda: cache.fork(max_len=room),
               extend=lambda: lm.extend(t_emb, cache.fork(max_len=room), lengths=turn))
    ids_a, ids_b = fns["reprefill"](), fns["follow_up"]()                             # warm-up of every path + a sanity line
    fns["extend"]()
    same = int((ids_a == ids_b).sum())
    t = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            t[k].append(wall(fn))
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    best = {k: min(v) for k, v in t.items()}
    gb = sum(hist) * 2 * 4096 * 2 * a.layers / 1e9
    print(f"[prefix_bench --follow-up] {a.layers} layers, {a.mode}, rows={B} history={hist} turn={turn} new={N}: " +
          "  ".join(f"{k} {med[k]:.2f} ms (best {best[k]:.2f})" for k in fns) +
          f"  | fork copies {gb:.2f} GB of live K / V (whole [q | k | v] rows: x 1.5)  | follow-up ids == re-prefill ids on {same}/{ids_a.numel()} tokens", flush=True)


if __name__ == "__main__":
    main()
