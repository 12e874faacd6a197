"""Call trace of the Llama decoder-layer host paths (models/llama.py) on the CPU contract backend (tests/_cpu_backend.py).

    python tests/golden/make_layer_trace.py      -> tests/golden/llama_layer_trace.json

The committed file was written by this script at the commit BEFORE the six copies of the layer body became one; tests/test_llama_layer_trace_cpu.py
replays record() on the code as it is and requires the same traces.  Only public entry points are driven: prefill, extend, decode_step and
sp_layer_part(carr=None).  An entry is [function, positional arguments, keywords] of one call into `hip`, in call order.  Scalars are kept as they are
(floats as "<float>"), a tensor as "buffer+element offset[shape]/[strides]:dtype" plus the contents of a small integer table; the buffer is x (the
residual), cache[l] / base[l] (a layer's KV buffer), scratch, qkv (sequence-parallel), w[l].key / q[l].key.q|scale (packed / quantised weights),
cos[S] / sin[S], norm, table (an uploaded integer table) or "temporary".  No pointers, no floating-point values: the trace is the same on any machine.
"""
import contextlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "llama_layer_trace.json")
TRACED = ["gemm", "gemv_w8", "gemv_q4", "rmsnorm", "attention", "attention_decode_ragged", "attention_shared", "kv_append_rows", "gather_rows", "lora_down",
          "h2d", "llama_layer_array", "llama_lora_array", "llama_layers", "llama_layers_extend", "llama_layer_sp"]
CFG = dict(num_hidden_layers=2, hidden_size=256, intermediate_size=512, num_attention_heads=2, vocab_size=64)
D = CFG["hidden_size"]
H2D_CASES = {"uniform": "decode_b3", "ragged": "decode_ragged_b3", "shared": "decode_shared_ragged"}   # the three cache shapes of a decode step


class Tracer:
    def __init__(self):
        self.entries, self.keep, self.ids, self.hints = [], [], {}, {}

    def sid(self, t):
        self.keep.append(t)   # alive until the case ends: no storage address is used twice
        return self.ids.setdefault(t.untyped_storage().data_ptr(), len(self.ids))

    def hint(self, t, name):
        if isinstance(t, torch.Tensor):
            self.hints.setdefault(self.sid(t), name)

    def desc(self, v):
        if v is None or isinstance(v, (bool, int, str)):
            return v
        if isinstance(v, float):
            return "<float>"
        if isinstance(v, torch.dtype):
            return str(v)
        if isinstance(v, torch.Tensor):
            d = {"sid": self.sid(v), "view": f"+{v.storage_offset()}{list(v.shape)}/{list(v.stride())}:{str(v.dtype)[6:]}"}
            if v.dtype in (torch.int32, torch.int64) and v.numel() <= 64:
                d["view"] += "=" + str(v.tolist())
            return d
        if isinstance(v, (tuple, list)):
            return "<layers>" if v and isinstance(v[0], dict) else [self.desc(e) for e in v]
        return f"<{type(v).__name__}>"

    def call(self, fn, a, k):
        if fn == "rmsnorm" or fn.startswith("llama_layer") and fn != "llama_layer_array":
            self.hint(a[0], "x")
        self.hint(k.get("resid"), "x")
        if k.get("a_norm") is not None:
            self.hint(k["a_norm"][0], "x")
        if fn == "kv_append_rows":
            self.hint(a[0], "scratch")
        if fn == "h2d":
            self.hint(a[0], "table")   # (on the CPU the upload returns its argument)
        self.entries.append([fn, [self.desc(v) for v in a], {n: self.desc(v) for n, v in sorted(k.items())}])

    def resolve(self, known):
        """the entries with every tensor's buffer named: `known` [(tensor, name)] first, then the role a buffer was seen in, else "temporary" """
        names = dict(self.hints)
        for t, name in known:
            key = t.untyped_storage().data_ptr()
            if key in self.ids:
                names[self.ids[key]] = name

        def fin(v):
            if isinstance(v, dict) and "sid" in v:
                return names.get(v["sid"], "temporary") + v["view"]
            if isinstance(v, dict):
                return {n: fin(e) for n, e in v.items()}
            return [fin(e) for e in v] if isinstance(v, list) else v
        return [fin(e) for e in self.entries]


ACTIVE = []   # the Tracer of the case that is being recorded, if any


@contextlib.contextmanager
def wrapped():
    """inside the backend's installed(): every call into `hip` that the layer paths make goes through the active Tracer first"""
    from stllm_amd import hip
    saved = {n: getattr(hip, n) for n in TRACED}

    def wrap(name, f):
        def g(*a, **k):
            if ACTIVE:
                ACTIVE[-1].call(name, a, k)
            k.pop("w_frag", None)   # recorded; the contract backend's gemm has no fragment-major operand
            return f(*a, **k)
        return g
    try:
        for n, f in saved.items():
            setattr(hip, n, wrap(n, f))
        yield
    finally:
        for n, f in saved.items():
            setattr(hip, n, f)


def known(lm, cache=None, extra=()):
    """[(tensor, name)] of the buffers a case can meet, in the current compute dtype / decode-weights mode"""
    from stllm_amd import runtime
    out = list(extra) + [(lm.norm.weight, "norm")]
    for (S, _), (cos, sin) in lm._rope.items():
        out += [(cos, f"cos[{S}]"), (sin, f"sin[{S}]")]
    for li, pk in enumerate(lm.pack(runtime.compute_dtype())):
        out += [(t, f"w[{li}].{key}") for key, t in pk.items() if isinstance(t, torch.Tensor)]
    mode = runtime.decode_weights()
    if mode is not None:
        for li, qw in enumerate(lm.pack_w8() if mode == "int8" else lm.pack_q4()):
            for key, (q, scale) in qw.items():
                out += [(q, f"q[{li}].{key}.q"), (scale, f"q[{li}].{key}.scale")]
    if cache is not None:
        out += [(t, f"cache[{li}]") for li, t in enumerate(cache.qkv)]
        if cache.base is not None:
            out += [(t, f"base[{li}]") for li, t in enumerate(cache.base.qkv)]
    return out


def model(lora=False):
    from stllm_amd import synth
    from stllm_amd.models import lora as lora_mod
    from stllm_amd.models.llama import LlamaConfig, LlamaModel
    lm = LlamaModel(LlamaConfig(**CFG), device="cpu")
    synth.fill_module_(lm, 0, "")
    if lora:   # active adapters with a non-zero B: the K-extended QKV weight and qkv_operand
        lm.add_lora(8)
        for li, layer in enumerate(lm.layers):
            for j, mod in enumerate(lora_mod.adapters_of(layer)):
                mod.B.copy_(synth.normal_(torch.empty(tuple(mod.B.shape)), f"trace.B{li}.{j}", 0, 0.05))
    return lm


def plant_frags(lm):
    """stand-ins for the fragment-major weight copies, which pack() makes on the GPU only: which calls pass w_frag= is part of the trace"""
    from stllm_amd import runtime
    for pk in lm.pack(runtime.compute_dtype()):
        pk["wqkv_frag"], pk["wgu_frag"] = torch.zeros(1), torch.zeros(1)


def emb(name, B, S):
    from stllm_amd import synth
    return synth.normal_(torch.empty((B, S, D)), "trace." + name, 0, 0.05)


def mask_of(lens, S):
    return (torch.arange(S)[None, :] < torch.tensor(lens)[:, None]).long()


def record():
    """{case: [entry, ...]} for every case; the set-up of a case (the prefill in front of a decode step, ...) is not traced"""
    import _cpu_backend as CB
    from stllm_amd import runtime
    from stllm_amd.models import llama
    out = {}

    def run(name, lm, fn, cache=None, extra=()):
        tr = Tracer()
        ACTIVE.append(tr)
        try:
            fn()
        finally:
            ACTIVE.pop()
        out[name] = tr.resolve(known(lm, cache, extra))

    def prefilled(lm, B, S, room, lens=None):
        c = lm.new_cache(B, S + room, "cpu")
        lm.prefill(emb("pre", B, S), None if lens is None else mask_of(lens, S), cache=c)
        return c

    def shared(lm, lengths=None):   # 2 rows behind one base row of 4 positions, 2 more positions (or `lengths`) already appended
        c = prefilled(lm, 1, 4, 2).share(rows=2, max_new=8)
        lm.extend(emb("sfx", 2, 2), c, lengths=lengths)
        return c

    def decode(name, lm, B, cache=None, lens=None):
        c = prefilled(lm, B, 5, 5, lens) if cache is None else cache
        run(name, lm, lambda: lm.decode_step(emb("tok", B, 1), c), c)

    with CB.installed(), wrapped(), torch.no_grad(), runtime.use_decode_weights(None):
        lm, lml = model(), model(lora=True)
        with runtime.use_dtype("bf16"):
            plant_frags(lm)
            run("prefill", lm, lambda: lm.prefill(emb("pre", 2, 5), None))
            c = lm.new_cache(2, 9, "cpu")
            run("prefill_cache", lm, lambda: lm.prefill(emb("pre", 2, 5), None, cache=c), c)
            c = lm.new_cache(2, 9, "cpu")
            run("prefill_cache_padded", lm, lambda: lm.prefill(emb("pre", 2, 5), mask_of([5, 3], 5), cache=c), c)
            c = lm.new_cache(2, 9, "cpu")
            old, llama.STACK_ENTRY = llama.STACK_ENTRY, False
            try:
                run("prefill_cache_per_op", lm, lambda: lm.prefill(emb("pre", 2, 5), None, cache=c), c)
            finally:
                llama.STACK_ENTRY = old
            c = prefilled(lm, 2, 4, 8)
            run("extend", lm, lambda: lm.extend(emb("ext", 2, 3), c), c)
            c = prefilled(lm, 2, 4, 8)
            run("extend_lengths", lm, lambda: lm.extend(emb("ext", 2, 3), c, lengths=[3, 2]), c)
            c = shared(lm)
            run("extend_shared", lm, lambda: lm.extend(emb("ext", 2, 3), c), c)
            c = shared(lm)
            run("extend_shared_lengths", lm, lambda: lm.extend(emb("ext", 2, 3), c, lengths=[3, 1]), c)
            decode("decode_b1", lm, 1)
            decode("decode_b3", lm, 3)
            decode("decode_ragged_b3", lm, 3, lens=[5, 3, 4])
            decode("decode_shared_uniform", lm, 2, cache=shared(lm))
            decode("decode_shared_ragged", lm, 2, cache=shared(lm, lengths=[2, 1]))
            for mode, tag in (("int8", "int8"), ("int4g128", "int4")):
                with runtime.use_decode_weights(mode):
                    decode(f"decode_{tag}_b1", lm, 1)
                    decode(f"decode_{tag}_b3", lm, 3)
            with runtime.use_decode_weights("int8"):
                decode("decode_int8_b17", lm, 17)   # more than 16 rows: the 16-bit step
            decode("decode_lora_b1", lml, 1)
            s0, s1 = 3, 8
            cos, sin = lm.rope(s1, "cpu")
            for part in (0, 1):
                x, qkv = emb("sp.x", 1, s1 - s0)[0].clone(), torch.zeros((s1, 3 * D), dtype=torch.bfloat16)
                run(f"sp_part{part}", lm, lambda: lm.sp_layer_part(part, x, lm.pack(torch.bfloat16), 1, qkv, s0, s1, cos[s0:s1], sin[s0:s1], torch.bfloat16, None),
                    extra=[(qkv, "qkv"), (x, "x")])
        with runtime.use_dtype("fp32"):
            plant_frags(lm)
            decode("decode_fp32_b1", lm, 1)
    return out


def h2d_counts(cases):
    """hip.h2d uploads of one decode step in each of the three cache shapes"""
    return {shape: sum(e[0] == "h2d" for e in cases[name]) for shape, name in H2D_CASES.items()}


def dumps(cases):
    body = ",\n".join(f' {json.dumps(name)}: [\n' + ",\n".join("  " + json.dumps(e, separators=(",", ":")) for e in entries) + "\n ]"
                      for name, entries in cases.items())
    return '{"h2d_per_decode_step": ' + json.dumps(h2d_counts(cases)) + ',\n"cases": {\n' + body + "\n}}\n"


if __name__ == "__main__":
    tests = os.path.dirname(HERE)
    for p in (os.path.dirname(tests), tests):
        if p not in sys.path:
            sys.path.insert(0, p)
    cases = record()
    with open(OUT, "w") as f:
        f.write(dumps(cases))
    print(f"{OUT}: {len(cases)} cases, {sum(len(e) for e in cases.values())} calls, h2d per decode step {h2d_counts(cases)}")
