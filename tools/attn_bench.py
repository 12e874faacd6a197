#!/usr/bin/env python3
"""Micro-benchmark of the attention shapes on the hot path (config 2).  GPU only."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from stllm_amd import hip

CASES = [("vit", 16, 16, 257, 257, 88, False, 39), ("llama", 1, 32, 576, 576, 128, True, 32), ("llama_b4", 4, 32, 576, 576, 128, True, 32),
         ("qf_self", 16, 12, 32, 32, 64, False, 12), ("qf_cross", 16, 12, 32, 257, 64, False, 6)]
if "--probe" in sys.argv:   # how does the Llama prefill kernel's time scale with the keys a workgroup walks / the workgroups in flight?  (non-causal: every workgroup alike)
    CASES += [("nc_k128", 1, 32, 576, 128, 128, False, 0), ("nc_k256", 1, 32, 576, 256, 128, False, 0), ("nc_k288", 1, 32, 576, 288, 128, False, 0),
              ("nc_k576", 1, 32, 576, 576, 128, False, 0), ("nc_k288_h51", 1, 51, 576, 288, 128, False, 0), ("nc_k288_h64", 1, 64, 576, 288, 128, False, 0),
              ("c_s288", 1, 32, 288, 288, 128, True, 0), ("c_s288_h64", 1, 64, 288, 288, 128, True, 0)]
AUDIT = "--audit" in sys.argv   # the Llama prefill kernel's work split (query tiles per workgroup x waves per query tile) forced through option attn_dma = 10 nw + ks
if AUDIT:
    CASES = [(f"llama_S{S}_B{B}", B, 32, S, S, 128, True, 32) for B, S in ((1, 178), (1, 296), (1, 400), (1, 528), (1, 576), (1, 700), (1, 1088), (4, 576), (2, 576), (16, 576))]
if "--ragged" in sys.argv:
    # one-token decode attention over a ragged KV cache (B = 8, mixed lengths up to ~1100, and one case beyond the single-pass limit): the ragged kernels against
    # the uniform decode kernels with EVERY row at the maximum length, and the append scatter; same buffers, alternating, a captured graph of 20 calls per timing.
    def timed_g(fn, rounds=5):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(20):
                fn()
        g.replay(); torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        best = float("inf")
        for _ in range(rounds):
            s.record(); g.replay(); e.record(); torch.cuda.synchronize()
            best = min(best, s.elapsed_time(e) / 20 * 1e3)
        return best
    H, D = 32, 128
    for lens in ([1100, 640, 333, 1021, 87, 590, 12, 845], [580] * 8, [2040, 700, 1500, 90], [601, 580, 577, 590, 600]):
        B, L = len(lens), max(lens)
        ML = L + 8
        dt = torch.bfloat16
        buf = torch.randn(B * ML, 3 * H * D, device="cuda").to(dt)
        row = torch.randn(B, 3 * H * D, device="cuda").to(dt)
        st = (ML * 3 * H * D, 3 * H * D)
        kv_len = torch.tensor(lens, dtype=torch.int32).cuda()
        pos = torch.tensor([n - 1 for n in lens], dtype=torch.int32).cuda()
        out = torch.empty(B, H * D, device="cuda", dtype=dt)
        kw = dict(B=B, H=H, Sq=1, Skv=L, D=D, scale=D ** -0.5, q_strides=(3 * H * D, 3 * H * D), k_strides=st, v_strides=st, out=out)
        uni = lambda: hip.attention(row[:, :H * D], buf[:, H * D:2 * H * D], buf[:, 2 * H * D:], **kw)
        rag = lambda: hip.attention(row[:, :H * D], buf[:, H * D:2 * H * D], buf[:, 2 * H * D:], kv_len=kv_len, **kw)
        app = lambda: hip.kv_append_rows(row, buf.view(B, ML, 3 * H * D), pos)
        res = {}
        for rnd in range(2):
            for name, f in (("uniform", uni), ("ragged", rag), ("append", app)):
                res.setdefault(name, []).append(timed_g(f))
        rag()
        kern = hip.lib().stllm_last_kernel().decode()
        print(f"decode attention B={B} lens={','.join(map(str, lens))}: uniform@{L} {min(res['uniform']):6.1f} us ({res['uniform'][0]:.1f} {res['uniform'][1]:.1f})  "
              f"ragged {min(res['ragged']):6.1f} us ({res['ragged'][0]:.1f} {res['ragged'][1]:.1f})  kv_append_rows {min(res['append']):5.1f} us ({res['append'][0]:.1f} {res['append'][1]:.1f})"
              f"  keys read {sum(lens)} vs {B * L}  -> {kern}", flush=True)
    sys.exit(0)
if "--shared" in sys.argv:
    # --shared R,P[,sfx] (repeatable): the one-token decode attention of R rows that share one P-key prefix and own sfx keys each (default 64).
    #   shared : hip.attention_shared — the prefix is read once for the R rows (dedicated prefix workgroups + suffix workgroups, then the merge);
    #   copies : the ragged decode attention on R private copies of prefix + suffix (what fork() gives), P + sfx keys per row;
    #   split  : the existing key-split tile kernel + its merge over the PREFIX ONLY, as a non-causal problem with R query rows (what the dedicated prefix
    #            workgroups replace; no suffix, no second merge: a lower bound of a composed decode path).
    # Same process, alternating, every timing a captured graph of 20 calls; best of 5 replays, both rounds printed.
    def timed_s(fn, rounds=5):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(20):
                fn()
        g.replay(); torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        best = float("inf")
        for _ in range(rounds):
            s.record(); g.replay(); e.record(); torch.cuda.synchronize()
            best = min(best, s.elapsed_time(e) / 20 * 1e3)
        return best
    H, D, dt = 32, 128, torch.bfloat16
    W = 3 * H * D
    for spec in [sys.argv[i + 1] for i, a in enumerate(sys.argv) if a == "--shared"]:
        R, P, sfx = (list(map(int, spec.split(","))) + [64])[:3]
        MLp, MLs, MLc = P + 8, sfx + 8, P + sfx + 8
        pre = torch.randn(MLp, W, device="cuda").to(dt)
        suf = torch.randn(R * MLs, W, device="cuda").to(dt)
        cop = torch.randn(R * MLc, W, device="cuda").to(dt)
        row = torch.randn(R, W, device="cuda").to(dt)
        out = torch.empty(R, H * D, device="cuda", dtype=dt)
        sl = torch.full((R,), sfx, dtype=torch.int32).cuda()
        kl = torch.full((R,), P + sfx, dtype=torch.int32).cuda()
        shared = lambda: hip.attention_shared(row[:, :H * D], pre[:, H * D:2 * H * D], pre[:, 2 * H * D:], suf[:, H * D:2 * H * D], suf[:, 2 * H * D:], B=R, G=1, H=H,
                                              Sq=1, P=P, D=D, scale=D ** -0.5, max_sfx=sfx, sfx_len=sl, q_strides=(W, W), kp_strides=(MLp * W, W),
                                              ks_strides=(MLs * W, W), out=out)
        copies = lambda: hip.attention(row[:, :H * D], cop[:, H * D:2 * H * D], cop[:, 2 * H * D:], B=R, H=H, Sq=1, Skv=P + sfx, D=D, scale=D ** -0.5, kv_len=kl,
                                       q_strides=(W, W), k_strides=(MLc * W, W), v_strides=(MLc * W, W), out=out)
        split = lambda: hip.attention(row[:, :H * D], pre[:, H * D:2 * H * D], pre[:, 2 * H * D:], B=1, H=H, Sq=R, Skv=P, D=D, scale=D ** -0.5, causal=False,
                                      q_strides=(R * W, W), k_strides=(MLp * W, W), v_strides=(MLp * W, W), q_off=1, out=out)
        res = {}
        hip.set_option("attn_ksplit", 1)
        try:
            for rnd in range(3):
                for name, f in (("shared", shared), ("copies", copies), ("split", split)):
                    res.setdefault(name, []).append(timed_s(f))
        finally:
            hip.set_option("attn_ksplit", -1)
        fmt = lambda n: f"{min(res[n]):6.1f} us (" + " ".join(f"{x:.1f}" for x in res[n]) + ")"
        print(f"shared-prefix decode attention R={R:3d} P={P:5d} sfx={sfx:4d}: shared {fmt('shared')}  copies {fmt('copies')}  prefix-only key-split+merge {fmt('split')}"
              f"  K/V bytes shared {(P + R * sfx) * 2 * H * D * 2 / 1e6:.1f} MB vs copies {R * (P + sfx) * 2 * H * D * 2 / 1e6:.1f} MB", flush=True)
    sys.exit(0)
if "--ragged-suffix" in sys.argv:
    # --ragged-suffix P1,P2,...:n1,n2,... (repeatable): a block of n_b new rows behind P_b cached positions per batch row (LlamaModel.extend on a ragged cache).
    #   ragged  : hip.attention_offset_ragged with the key split forced on (1), forced off (0) and by the rule (auto), padded to Sq = max(n);
    #   per-row : what the parent commit has — one stllm_attention_offset call per row with n_b > 0 (B = 1, q_off = P_b, default dispatch), len(rows) launches (pairs);
    #   steps   : ... or max(n) one-token ragged decode-attention steps over all rows (kv_len = P_b + min(t + 1, n_b)).
    # Same process and buffers, alternating, every timing a captured graph of 20 calls; best of 5 replays, every round printed.
    def timed_r(fn, rounds=5):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(20):
                fn()
        g.replay(); torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        best = float("inf")
        for _ in range(rounds):
            s.record(); g.replay(); e.record(); torch.cuda.synchronize()
            best = min(best, s.elapsed_time(e) / 20 * 1e3)
        return best
    H, D, dt = 32, 128, torch.bfloat16
    HD, W = H * D, 3 * H * D
    for spec in [sys.argv[i + 1] for i, a in enumerate(sys.argv) if a == "--ragged-suffix"]:
        Ps, ns = (list(map(int, part.split(","))) for part in spec.split(":"))
        assert len(Ps) == len(ns)
        B, S, max_kv = len(Ps), max(ns), max(p + n for p, n in zip(Ps, ns))
        ML = max_kv + 8
        buf = torch.randn(B * ML, W, device="cuda").to(dt)
        dense = torch.randn(B * S, W, device="cuda").to(dt)
        st = (ML * W, W)
        out = torch.empty(B * S, HD, device="cuda", dtype=dt)
        q_off = torch.tensor(Ps, dtype=torch.int32).cuda()
        kv_len = torch.tensor([p + n for p, n in zip(Ps, ns)], dtype=torch.int32).cuda()
        step_len = [torch.tensor([p + min(t + 1, n) for p, n in zip(Ps, ns)], dtype=torch.int32).cuda() for t in range(S)]
        ragged = lambda: hip.attention_offset_ragged(dense[:, :HD], buf[:, HD:2 * HD], buf[:, 2 * HD:], q_off, kv_len, B=B, H=H, Sq=S, max_kv=max_kv, D=D,
                                                     scale=D ** -0.5, out=out, q_strides=(S * W, W), k_strides=st, v_strides=st)

        def per_row():
            for b, (p, n) in enumerate(zip(Ps, ns)):
                if n:
                    hip.attention(dense[b * S:, :HD], buf[b * ML:, HD:2 * HD], buf[b * ML:, 2 * HD:], B=1, H=H, Sq=n, Skv=p + n, D=D, scale=D ** -0.5, causal=True,
                                  q_strides=(S * W, W), k_strides=st, v_strides=st, q_off=p, out=out[b * S:b * S + n])

        def steps():
            for t in range(S):
                hip.attention(dense[t:, :HD], buf[:, HD:2 * HD], buf[:, 2 * HD:], B=B, H=H, Sq=1, Skv=max_kv, D=D, scale=D ** -0.5, kv_len=step_len[t],
                              q_strides=(S * W, W), k_strides=st, v_strides=st, out=out[:B])
        res = {}
        try:
            for rnd in range(2):
                for name, opt, f in (("split", 1, ragged), ("tile", 0, ragged), ("auto", -1, ragged), ("per-row", -1, per_row), ("steps", -1, steps)):
                    hip.set_option("attn_ksplit", opt)
                    res.setdefault(name, []).append(timed_r(f))
        finally:
            hip.set_option("attn_ksplit", -1)
        ragged()
        auto = hip.lib().stllm_last_kernel().decode()
        fmt = lambda n: f"{min(res[n]):7.1f} us (" + " ".join(f"{x:.1f}" for x in res[n]) + ")"
        print(f"ragged suffix B={B} P={','.join(map(str, Ps))} n={','.join(map(str, ns))}: key-split {fmt('split')}  tile {fmt('tile')}  auto {fmt('auto')} -> {auto}"
              f"  | parent: per-row offset calls {fmt('per-row')}  {S} decode steps {fmt('steps')}", flush=True)
    sys.exit(0)
if "--segments-shared" in sys.argv:
    # --segments-shared P (repeatable; default 576 and 2048): the packed admission step of serving.Engine(base=) at the shape of --segments' default case — 15
    # one-token segments plus one 40-token segment, every segment behind the SAME P prefix keys.  The suffix offsets are those the default case has behind a
    # 576-token prefix (totals 560 .. 1100; the one-token segments that would sit in front of position 576 are placed at 576: an empty suffix), the 40-token
    # segment sits behind 4 suffix positions (total 580); a larger P keeps the offsets.
    #   shared : hip.attention_segments_shared — prefix pass over ONE copy of the prefix (T query rows, full tiles), suffix pass per segment, merge;
    #   copies : hip.attention_segments on R private copies of prefix + suffix (what KVCache.load_row gives), by the dispatch rule (auto) and with the key
    #            split forced on.
    # Same process, alternating, every timing a captured graph of 20 calls; best of 5 replays, every round printed.
    def timed_h(fn, rounds=5):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(20):
                fn()
        g.replay(); torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        best = float("inf")
        for _ in range(rounds):
            s.record(); g.replay(); e.record(); torch.cuda.synchronize()
            best = min(best, s.elapsed_time(e) / 20 * 1e3)
        return best
    H, D, dt = 32, 128, torch.bfloat16
    HD, W = H * D, 3 * H * D
    Pl = [int(sys.argv[i + 1]) for i, a in enumerate(sys.argv) if a == "--segments-shared" and i + 1 < len(sys.argv) and sys.argv[i + 1].isdigit()]
    offs = [max(0, 560 + (540 * i) // 14 - 576) for i in range(15)] + [4]
    ns = [1] * 15 + [40]
    for P in Pl or [576, 2048]:
        R, S, T, max_sfx = len(ns), max(ns), sum(ns), max(o + n for o, n in zip(offs, ns))
        MLp, MLs, MLc = P + 8, max_sfx + 8, P + max_sfx + 8
        pre = torch.randn(MLp, W, device="cuda").to(dt)
        suf = torch.randn(R * MLs, W, device="cuda").to(dt)
        cop = torch.randn(R * MLc, W, device="cuda").to(dt)
        packed = torch.randn(T, W, device="cuda").to(dt)
        out = torch.empty(T, HD, device="cuda", dtype=dt)
        i32 = lambda x: torch.tensor(x, dtype=torch.int32).cuda()
        row0 = [sum(ns[:r]) for r in range(R)]
        slot, row0_t, sfx_off, sfx_len = i32(list(range(R))), i32(row0), i32(offs), i32([o + n for o, n in zip(offs, ns)])
        q_off, kv_len = i32([P + o for o in offs]), i32([P + o + n for o, n in zip(offs, ns)])
        shared = lambda: hip.attention_segments_shared(packed[:, :HD], pre[:, HD:2 * HD], pre[:, 2 * HD:], suf[:, HD:2 * HD], suf[:, 2 * HD:], slot, row0_t, sfx_off,
                                                       sfx_len, H=H, D=D, T=T, P=P, n_slots=R, max_n=S, max_sfx=max_sfx, scale=D ** -0.5, out=out,
                                                       kp_strides=(MLp * W, W), ks_strides=(MLs * W, W))
        copies = lambda: hip.attention_segments(packed[:, :HD], cop[:, HD:2 * HD], cop[:, 2 * HD:], slot, row0_t, q_off, kv_len, H=H, D=D, T=T, n_slots=R, max_n=S,
                                                max_kv=P + max_sfx, scale=D ** -0.5, out=out, k_strides=(MLc * W, W), v_strides=(MLc * W, W))
        res = {}
        try:
            for rnd in range(3):
                for name, opt, f in (("shared", -1, shared), ("copies", -1, copies), ("copies-split", 1, copies)):
                    hip.set_option("attn_ksplit", opt)
                    res.setdefault(name, []).append(timed_h(f))
        finally:
            hip.set_option("attn_ksplit", -1)
        copies()
        auto = hip.lib().stllm_last_kernel().decode()
        fmt = lambda n: f"{min(res[n]):7.1f} us (" + " ".join(f"{x:.1f}" for x in res[n]) + ")"
        print(f"segments on a shared base R={R} T={T} P={P} sfx_off={','.join(map(str, offs))} n={','.join(map(str, ns))}: shared {fmt('shared')}  "
              f"attention_segments on copies: auto {fmt('copies')} -> {auto}, key split forced {fmt('copies-split')}"
              f"  K/V bytes shared {(P + sum(o + n for o, n in zip(offs, ns))) * 2 * HD * 2 / 1e6:.1f} MB vs copies {sum(P + o + n for o, n in zip(offs, ns)) * 2 * HD * 2 / 1e6:.1f} MB",
              flush=True)
    sys.exit(0)
if "--segments" in sys.argv:
    # --segments [P1,P2,...:n1,n2,...] (repeatable; default: 15 one-token segments behind 560 .. 1100 positions plus one 40-token segment behind 580): the packed
    # admission step of serving.Engine — segment r appends n_r rows behind P_r cached positions of its own slot.
    #   segments : hip.attention_segments on the packed [T, 3 H D] scratch, key split forced on (1), forced off (0) and by the rule (auto);
    #   padded   : what the parent commit has — hip.attention_offset_ragged on the padded R x max(n) layout (auto) ...
    #   dec+off  : ... or the ragged decode attention for the one-token rows plus one stllm_attention_offset call per longer row.
    # Same process and buffers, alternating, every timing a captured graph of 20 calls; best of 5 replays, every round printed.
    def timed_q(fn, rounds=5):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(20):
                fn()
        g.replay(); torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        best = float("inf")
        for _ in range(rounds):
            s.record(); g.replay(); e.record(); torch.cuda.synchronize()
            best = min(best, s.elapsed_time(e) / 20 * 1e3)
        return best
    H, D, dt = 32, 128, torch.bfloat16
    HD, W = H * D, 3 * H * D
    specs = [sys.argv[i + 1] for i, a in enumerate(sys.argv) if a == "--segments" and i + 1 < len(sys.argv) and ":" in sys.argv[i + 1]]
    default = ",".join(str(560 + (540 * i) // 14) for i in range(15)) + ",580:" + ",".join(["1"] * 15) + ",40"
    for spec in specs or [default]:
        Ps, ns = (list(map(int, part.split(","))) for part in spec.split(":"))
        assert len(Ps) == len(ns) and min(ns) >= 1
        R, S, T, max_kv = len(Ps), max(ns), sum(ns), max(p + n for p, n in zip(Ps, ns))
        ML = max_kv + 8
        buf = torch.randn(R * ML, W, device="cuda").to(dt)
        packed = torch.randn(T, W, device="cuda").to(dt)
        padded = torch.randn(R * S, W, device="cuda").to(dt)
        st = (ML * W, W)
        out, out_p = torch.empty(T, HD, device="cuda", dtype=dt), torch.empty(R * S, HD, device="cuda", dtype=dt)
        i32 = lambda x: torch.tensor(x, dtype=torch.int32).cuda()
        row0 = [sum(ns[:r]) for r in range(R)]
        slot, row0_t, q_off, kv_len = i32(list(range(R))), i32(row0), i32(Ps), i32([p + n for p, n in zip(Ps, ns)])
        ones = [r for r in range(R) if ns[r] == 1]
        dec_len = i32([Ps[r] + 1 for r in ones]) if ones else None
        seg = lambda: hip.attention_segments(packed[:, :HD], buf[:, HD:2 * HD], buf[:, 2 * HD:], slot, row0_t, q_off, kv_len, H=H, D=D, T=T, n_slots=R, max_n=S,
                                             max_kv=max_kv, scale=D ** -0.5, out=out, k_strides=st, v_strides=st)
        pad = lambda: hip.attention_offset_ragged(padded[:, :HD], buf[:, HD:2 * HD], buf[:, 2 * HD:], q_off, kv_len, B=R, H=H, Sq=S, max_kv=max_kv, D=D,
                                                  scale=D ** -0.5, out=out_p, q_strides=(S * W, W), k_strides=st, v_strides=st)

        def dec_off():   # (the one-token rows are taken as the first len(ones) cache rows: the same keys are walked)
            if ones:
                hip.attention(packed[:, :HD], buf[:, HD:2 * HD], buf[:, 2 * HD:], B=len(ones), H=H, Sq=1, Skv=max(Ps[r] + 1 for r in ones), D=D, scale=D ** -0.5,
                              kv_len=dec_len, q_strides=(W, W), k_strides=st, v_strides=st, out=out[:len(ones)])
            for r in range(R):
                if ns[r] > 1:
                    hip.attention(packed[row0[r]:, :HD], buf[r * ML:, HD:2 * HD], buf[r * ML:, 2 * HD:], B=1, H=H, Sq=ns[r], Skv=Ps[r] + ns[r], D=D, scale=D ** -0.5,
                                  causal=True, q_strides=(ns[r] * W, W), k_strides=st, v_strides=st, q_off=Ps[r], out=out[row0[r]:row0[r] + ns[r]])
        res = {}
        try:
            for rnd in range(2):
                for name, opt, f in (("split", 1, seg), ("tile", 0, seg), ("auto", -1, seg), ("padded", -1, pad), ("dec+off", -1, dec_off)):
                    hip.set_option("attn_ksplit", opt)
                    res.setdefault(name, []).append(timed_q(f))
        finally:
            hip.set_option("attn_ksplit", -1)
        seg()
        auto = hip.lib().stllm_last_kernel().decode()
        fmt = lambda n: f"{min(res[n]):7.1f} us (" + " ".join(f"{x:.1f}" for x in res[n]) + ")"
        print(f"segments R={R} T={T} P={','.join(map(str, Ps))} n={','.join(map(str, ns))}: key-split {fmt('split')}  tile {fmt('tile')}  auto {fmt('auto')} -> {auto}"
              f"  | parent: padded {R}x{S} ragged {fmt('padded')}  decode + offset calls {fmt('dec+off')}", flush=True)
    sys.exit(0)
if "--suffix" in sys.argv:
    # LlamaModel.extend's shape: Sq new rows behind q_off cached ones, operands addressed inside one fused cache buffer as the model passes them.
    # The offset tile kernel (attn_ksplit = 0) and the key-split pair (1) on the same buffers, same process, alternating; "auto" is the dispatch rule.
    # Every timing replays a captured graph of 20 calls, so that launch gaps on the host do not hide a difference of a few microseconds.
    def timed(fn, rounds=5):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(20):
                fn()
        g.replay(); torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        best = float("inf")
        for _ in range(rounds):
            s.record(); g.replay(); e.record(); torch.cuda.synchronize()
            best = min(best, s.elapsed_time(e) / 20 * 1e3)
        return best
    shapes = [(B, Sq, off) for B in (1,) for Sq in (8, 40, 96) for off in (512, 1024, 2048)] + [(1, 40, 128), (1, 40, 256), (1, 200, 1024), (1, 320, 2048), (5, 40, 1024)]
    for dt in (torch.bfloat16,) + ((torch.float16,) if "--fp16" in sys.argv else ()):
        for B, Sq, off in shapes:
            H, D, Skv = 32, 128, off + Sq
            ML = Skv + 8
            buf = torch.randn(B * ML, 3 * H * D, device="cuda").to(dt)
            st = (ML * 3 * H * D, 3 * H * D)
            out = torch.empty(B * Sq, H * D, device="cuda", dtype=dt)
            call = lambda: hip.attention(buf[off:, :H * D], buf[:, H * D:2 * H * D], buf[:, 2 * H * D:], B=B, H=H, Sq=Sq, Skv=Skv, D=D, scale=D ** -0.5, causal=True,
                                         q_strides=st, k_strides=st, v_strides=st, q_off=off, out=out)
            res = {}
            for rnd in range(2):                      # tile, split, tile, split: alternating
                for opt in (0, 1):
                    hip.set_option("attn_ksplit", opt)
                    res.setdefault(opt, []).append(timed(call))
            hip.set_option("attn_ksplit", -1)
            call()
            auto = hip.lib().stllm_last_kernel().decode()
            t, k = min(res[0]), min(res[1])
            print(f"suffix {str(dt)[6:]:9s} B={B} Sq={Sq:4d} q_off={off:5d}  tile {t:7.1f} us ({res[0][0]:.1f} {res[0][1]:.1f})  key-split {k:7.1f} us ({res[1][0]:.1f} {res[1][1]:.1f})"
                  f"  ratio {t / k:5.2f}  auto -> {auto}", flush=True)
    sys.exit(0)
for name, B, H, Sq, Skv, D, causal, per_clip in CASES:
    dt = torch.bfloat16
    if Sq == Skv:
        buf = torch.randn(B * Sq, 3 * H * D, device="cuda").to(dt)
        q, k, v = buf[:, :H * D], buf[:, H * D:2 * H * D], buf[:, 2 * H * D:]
    else:
        q = torch.randn(B * Sq, H * D, device="cuda").to(dt)
        kv = torch.randn(B * Skv, 2 * H * D, device="cuda").to(dt)
        k, v = kv[:, :H * D], kv[:, H * D:]
    out = hip.attention(q, k, v, B=B, H=H, Sq=Sq, Skv=Skv, D=D, scale=D ** -0.5, causal=causal)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(20):
        hip.attention(q, k, v, B=B, H=H, Sq=Sq, Skv=Skv, D=D, scale=D ** -0.5, causal=causal, out=out)
    e.record(); torch.cuda.synchronize()
    ms = s.elapsed_time(e) / 20
    fl = 4.0 * B * H * Sq * Skv * D * (0.5 if causal else 1.0)
    print(f"{name:9s} B={B:3d} H={H:3d} Sq={Sq:4d} Skv={Skv:4d} D={D:4d} {ms * 1e3:8.1f} us  {fl / ms / 1e9:7.1f} TF   x{per_clip} = {ms * per_clip:.3f} ms")
    if AUDIT:
        rows = []
        for cfg in (121, 81, 61, 41, 62, 42, 32, 22, 34, 24, 14):
            hip.set_option("attn_dma", cfg)
            try:
                for _ in range(3): hip.attention(q, k, v, B=B, H=H, Sq=Sq, Skv=Skv, D=D, scale=D ** -0.5, causal=causal, out=out)
                s.record()
                for _ in range(20): hip.attention(q, k, v, B=B, H=H, Sq=Sq, Skv=Skv, D=D, scale=D ** -0.5, causal=causal, out=out)
                e.record(); torch.cuda.synchronize()
                rows.append((s.elapsed_time(e) / 20 * 1e3, cfg))
            except Exception as ex:   # noqa: BLE001
                rows.append((float("inf"), cfg))
            finally:
                hip.set_option("attn_dma", 1)
        rows.sort()
        print("      " + "  ".join(f"{c // 10}x{c % 10}: {us:.1f}" for us, c in rows[:6]) + (f"   <-- {ms * 1e3 - rows[0][0]:.1f} us faster than the automatic choice" if rows[0][0] < 0.97 * ms * 1e3 else ""))
