"""Call trace of the generate host path (generation.py, STLLMForCausalLM.generate, Chat.answer / answer_many) on the CPU contract backend
(tests/_cpu_backend.py), fp32.

    python tests/golden/make_generate_trace.py      -> tests/golden/generate_trace.json

The committed file was written by this script at the commit BEFORE the prompt-cache setup of generation._CacheStepper became one sequence and the
generate() options one object; tests/test_generate_trace_cpu.py replays record() on the code as it is and requires the same traces.  An entry is one call
of LlamaModel.prefill / extend / decode_step or of logits_from, in call order: [method, shape of the embeddings (logits_from: of the hidden rows),
`lengths` (prefill: the row sums of the mask) or None, the cache as it is when the call is made: {batch, max_len, len, lens, base: None | [base.batch,
base.len]} or None].  A case ends with ["result", shape of the returned ids]; where the combination raises, the case is ["raises", exception type, message] alone.
No floats, no pointers, no token ids.  The model is the small one of tests/test_ragged_cpu.py; every case generates 3 tokens.
"""
import contextlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "generate_trace.json")
NEW = 3
LENS = [6, 4, 6]            # the mixed-length batch of the batching= cases
QUESTIONS = [[21, 22, 23], [400, 17, 9000, 5, 77], [9]]


def cache_desc(c):
    if c is None:
        return None
    return {"batch": c.batch, "max_len": c.max_len, "len": c.len, "lens": None if c.lens is None else list(c.lens),
            "base": None if c.base is None else [c.base.batch, c.base.len]}


@contextlib.contextmanager
def wrapped(model, entries):
    """every call of the four methods on `model` (an STLLMForCausalLM) and its LlamaModel appends to `entries` first"""
    lm = model.model

    def prefill(emb, attention_mask=None, cache=None):
        entries.append(["prefill", list(emb.shape), None if attention_mask is None else attention_mask.sum(dim=1).tolist(), cache_desc(cache)])
        return type(lm).prefill(lm, emb, attention_mask, cache=cache)

    def extend(emb, cache, lengths=None):
        entries.append(["extend", list(emb.shape), None if lengths is None else [int(n) for n in lengths], cache_desc(cache)])
        return type(lm).extend(lm, emb, cache, lengths=lengths)

    def decode_step(x_new, cache):
        entries.append(["decode_step", list(x_new.shape), None, cache_desc(cache)])
        return type(lm).decode_step(lm, x_new, cache)

    def logits_from(h16, B, S):
        entries.append(["logits_from", list(h16.shape), [B, S], None])
        return type(model).logits_from(model, h16, B, S)
    try:
        lm.prefill, lm.extend, lm.decode_step, model.logits_from = prefill, extend, decode_step, logits_from
        yield
    finally:
        del lm.prefill, lm.extend, lm.decode_step, model.logits_from


def padded(prompts, side):
    S = max(p.shape[0] for p in prompts)
    emb = torch.zeros(len(prompts), S, prompts[0].shape[1])
    mask = torch.zeros(len(prompts), S, dtype=torch.long)
    for i, p in enumerate(prompts):
        sl = slice(0, p.shape[0]) if side == "right" else slice(S - p.shape[0], S)
        emb[i, sl], mask[i, sl] = p, 1
    return emb, mask


def record(model=None):
    """{case: [entry, ...]}.  model: test_ragged_cpu._build(CFG) with the lm_head spread by 6, when the caller has one already"""
    import _cpu_backend as CB
    import _select_ref as R
    from _util import T
    from test_ragged_cpu import CFG, _build
    from stllm_amd import generation, runtime
    from stllm_amd.conversation import Chat
    out = {}
    with torch.no_grad(), CB.installed(), CB._patched({"select_tokens": R.select_tokens, "beam_candidates": R.beam_candidates}), runtime.use_dtype("fp32"), \
            runtime.use_decode_weights(None):
        if model is None:
            model = _build(CFG)
            model.lm_head.weight.mul_(6.0)   # as the fixture of tests/test_ragged_cpu.py
        lm = model.model

        def run(name, fn):
            entries = []
            with wrapped(model, entries):
                try:
                    res = fn()
                    res = res[0] if isinstance(res, tuple) else res
                    entries.append(["result", [len(res)] if isinstance(res, list) else list(res.shape)])
                except Exception as e:   # a combination that raises: its type and message are the record, instead of the calls made before it
                    entries[:] = [["raises", type(e).__name__, str(e)]]
            out[name] = entries

        emb = T("gtrace.emb", (2, 6, 4096), 0.05)
        prefixes = {"none": None}
        for key, rows in (("per_row", 2), ("one_row", 1)):
            prefixes[key] = lm.new_cache(rows, 5, "cpu")
            lm.prefill(T("gtrace.prefix", (rows, 5, 4096), 0.05), None, cache=prefixes[key])
        for pkey, prefix in prefixes.items():
            for lkey, lengths in (("uniform", None), ("lengths", [6, 4])):
                for nb in (1, 3):
                    for share in (False, True):
                        run(f"stepper/prefix={pkey}/{lkey}/beams={nb}/share={share}",
                            lambda: generation.generate(model, emb, max_new_tokens=NEW, num_beams=nb, prefix=prefix, lengths=lengths, share_prefix=share))
        run("use_cache=False", lambda: generation.generate(model, emb, max_new_tokens=NEW, use_cache=False))
        run("use_cache=False/beams=3", lambda: generation.generate(model, emb, max_new_tokens=NEW, use_cache=False, num_beams=3))
        run("device/greedy", lambda: generation.generate(model, emb, max_new_tokens=NEW, selection="device"))
        prompts = [T(f"gtrace.prompt{i}", (n, 4096), 0.05) for i, n in enumerate(LENS)]
        for side in ("right", "left"):
            e, m = padded(prompts, side)
            for batching in ("groups", "ragged"):
                for nb in (1, 3):
                    run(f"batching={batching}/{side}/beams={nb}",
                        lambda: model.generate(inputs_embeds=e, attention_mask=m, max_new_tokens=NEW, num_beams=nb, batching=batching))
        chat = Chat(model, device="cpu")
        img_list = []
        chat.upload_video(T("input.frames2", (2, 3, 224, 224)).view(6, 224, 224), None, img_list)
        nv = img_list[0].shape[1]
        run("chat/prefill_video", lambda: chat.prefill_video(img_list).cache.qkv)
        vp = chat.prefill_video(img_list)
        for pkey, pf in (("none", None), ("video", vp)):
            for nb in (1, 3):
                run(f"chat/answer/prefix={pkey}/beams={nb}", lambda: chat.answer(img_list, QUESTIONS[1], max_new_tokens=NEW, num_beams=nb, prefix=pf)[1])
                run(f"chat/answer_many/prefix={pkey}/beams={nb}", lambda: chat.answer_many(img_list, QUESTIONS, max_new_tokens=NEW, num_beams=nb, prefix=pf))
            # the truncation rule cuts into the video: the whole-prompt path, prefix or not
            run(f"chat/answer/prefix={pkey}/truncated", lambda: chat.answer(img_list, QUESTIONS[1], max_new_tokens=NEW, max_length=nv + 2 + NEW, prefix=pf)[1])
            run(f"chat/answer_many/prefix={pkey}/truncated", lambda: chat.answer_many(img_list, QUESTIONS, max_new_tokens=NEW, max_length=nv + 2 + NEW, prefix=pf))
        run("chat/answer_many/prefix=video/share", lambda: chat.answer_many(img_list, QUESTIONS, max_new_tokens=NEW, num_beams=3, prefix=vp, share_prefix=True))
    return out


def dumps(cases):
    body = ",\n".join(f' {json.dumps(name)}: [\n' + ",\n".join("  " + json.dumps(e, separators=(",", ":")) for e in entries) + "\n ]"
                      for name, entries in cases.items())
    return '{"cases": {\n' + body + "\n}}\n"


if __name__ == "__main__":
    tests = os.path.dirname(HERE)
    for p in (os.path.dirname(tests), tests):
        if p not in sys.path:
            sys.path.insert(0, p)
    cases = record()
    with open(OUT, "w") as f:
        f.write(dumps(cases))
    print(f"{OUT}: {len(cases)} cases, {sum(len(e) - 1 for e in cases.values())} calls")
