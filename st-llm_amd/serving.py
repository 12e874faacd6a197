"""Continuous batching: a fixed set of KV-cache slots, requests admitted into free slots while the others keep decoding.

`generate()` fixes its batch when it starts: a row that finished is fed pad tokens until the slowest row is done, and a new prompt waits for the whole
batch.  The Engine owns one KVCache of `slots` rows instead.  Every step it frees the slots of finished requests, admits queued requests into free slots
(FIFO) and runs ONE pass of the decoder:

  * a step WITH admissions is LlamaModel.step_segments: the step's tokens packed as [T, D] — one token for every running request, the whole remaining
    prompt of every admitted one — on hip.kv_append_segments / hip.attention_segments.  No pad rows; running rows do not stall.
  * a step WITHOUT admissions is LlamaModel.decode_step on the slot cache, the GEMV path that a fixed batch takes (quantised decode weights included).
    Free slots ride along as don't-care rows; their length is put back to 0 afterwards.

Selection is per request, with generate()'s own processors (generation._process_logits / _warp_logits) on that request's ids and step count: a request
generates the ids that generate() gives for it alone (greedy; sampling with its own generator).

Not served (they raise): beams, selection="device" (stllm_select_tokens takes one step index for all rows), share_prefix / caches with a base,
return_cache.  No paged blocks, no preemption: a request must fit `max_len` positions when it is submitted and keeps its slot until it finishes."""
import collections

import torch

from . import generation


class _Request:
    __slots__ = ("handle", "emb", "prefix", "max_new", "generator", "slot", "ids", "pending")

    def __init__(self, handle, emb, prefix, max_new, generator):
        self.handle, self.emb, self.prefix, self.max_new, self.generator = handle, emb, prefix, max_new, generator
        self.slot, self.pending = None, None
        self.ids = torch.zeros((1, 0), dtype=torch.long, device=emb.device)   # on the device of the logits, as generate() keeps them


class Engine:
    """Engine(lm_wrapper, slots, max_len, **options): `lm_wrapper` is what generate() runs on (`.model` a LlamaModel, `.logits_from`), `options` are
    generate()'s sampling and stopping options (generation.Options); num_beams == 1, use_cache and selection == "torch" only."""

    def __init__(self, lm_wrapper, slots, max_len, device=None, **options):
        o = generation.Options(**options)
        if o.num_beams != 1:
            raise NotImplementedError("serving.Engine: beams are not served (num_beams == 1)")
        if o.selection != "torch":
            raise NotImplementedError("serving.Engine: selection='device' is not served (stllm_select_tokens takes one step index for all rows)")
        if not o.use_cache:
            raise ValueError("serving.Engine: needs use_cache (the slots ARE the KV cache)")
        if o.share_prefix or o.return_cache or o.return_lengths:
            raise NotImplementedError("serving.Engine: share_prefix / return_cache / return_lengths are generate()'s")
        self.o = o._replace(stop_sequences=list(o.stop_sequences) if o.stop_sequences else None)
        self.m, self.lm = lm_wrapper, lm_wrapper.model
        self.device = torch.device(device) if device is not None else self.lm.embed_tokens.weight.device
        assert slots >= 1 and max_len >= 2
        self.cache = self.lm.new_cache(slots, max_len, self.device)
        self.cache.set_lens([0] * slots)
        self.queue = collections.deque()
        self.running = {}                 # slot -> _Request
        self.done_slots = []              # slots whose request finished in the last step: released at the start of the next one
        self.free = list(range(slots))
        self.handles = 0
        self.steps = collections.Counter()   # "segments" / "decode": the passes run so far

    # ---- requests ------------------------------------------------------------------------------------------------------------------------------
    def submit(self, inputs_embeds, prefix=None, max_new_tokens=None, generator=None):
        """queue a request: inputs_embeds [S, D] (S >= 1), the prompt — or, with `prefix` (a one-row uniform KVCache without a base, e.g.
        Chat.prefill_video(...).cache, only ever read), what follows the prefix's positions.  generator: the request's own torch.Generator for do_sample
        (default: the Engine's `generator` option).  Raises if prefix + prompt + max_new_tokens does not fit a slot.  Returns the handle."""
        max_new = self.o.max_new_tokens if max_new_tokens is None else int(max_new_tokens)
        assert inputs_embeds.dim() == 2 and inputs_embeds.shape[0] >= 1 and max_new >= 1
        P = 0
        if prefix is not None:
            if prefix.base is not None or prefix.lens is not None or prefix.batch != 1:
                raise NotImplementedError("serving.Engine.submit(prefix=): a one-row uniform KVCache without a base")
            P = prefix.len
        need = P + inputs_embeds.shape[0] + max_new - 1      # the last generated token is never fed
        if need > self.cache.max_len:
            raise ValueError(f"serving.Engine.submit: the request needs {need} positions (prefix + prompt + max_new_tokens - 1), a slot holds {self.cache.max_len}")
        self.handles += 1
        self.queue.append(_Request(self.handles, inputs_embeds.float().to(self.device), prefix, max_new, generator if generator is not None else self.o.generator))
        return self.handles

    def idle(self):
        return not self.queue and not self.running

    # ---- one step ------------------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self):
        """release, admit, one decoder pass, one selected token per request in a slot.  Returns [(handle, ids)] of the requests that finished in this
        step: ids is the 1-D LongTensor generate() returns for that request alone."""
        for s in self.done_slots:
            self.cache.release(s)
            self.free.append(s)
        self.done_slots = []
        self.free.sort()
        admitted = []
        while self.queue and self.free:
            r = self.queue.popleft()
            r.slot = self.free.pop(0)
            if r.prefix is not None:
                self.cache.load_row(r.slot, r.prefix)
            admitted.append(r)
        if not admitted and not self.running:
            return []
        running = [self.running[s] for s in sorted(self.running)]
        if admitted:
            parts, segments = [], []
            if running:
                parts.append(self.lm.embed_tokens(torch.tensor([[r.pending] for r in running]))[:, 0].float().to(self.device))
                segments += [(r.slot, 1) for r in running]
            for r in admitted:
                parts.append(r.emb)
                segments.append((r.slot, r.emb.shape[0]))
                self.running[r.slot] = r
                r.emb = None
            _, h16 = self.lm.step_segments(torch.cat(parts) if len(parts) > 1 else parts[0], self.cache, segments)
            served = running + admitted
            logits = self.m.logits_from(h16, len(served), 1)[:, 0].float()
            self.steps["segments"] += 1
        else:
            K = self.cache.batch
            toks = [self.o.pad_token_id] * K
            for r in running:
                toks[r.slot] = r.pending
            _, h16 = self.lm.decode_step(self.lm.embed_tokens(torch.tensor(toks).view(K, 1)).float().to(self.device), self.cache)
            for s in self.free:               # the free slots rode along: whatever they appended is don't-care
                self.cache.release(s)
            logits = self.m.logits_from(h16, K, 1)[:, 0].float()[[r.slot for r in running]]
            served = running
            self.steps["decode"] += 1
        finished = []
        for i, r in enumerate(served):
            if self._select(r, logits[i:i + 1]):
                finished.append((r.handle, r.ids[0].clone()))
                del self.running[r.slot]
                self.done_slots.append(r.slot)
        if finished and self.device.type == "cuda":
            from . import hip
            hip.gemm_workspace_check(self.device, wait=True)   # as generation._finish: no id leaves behind a timed-out split-K exchange
        return finished

    def _select(self, r, logits):
        """generation._generate_torch's step for ONE request: its own ids, its own step count.  True when the request is finished."""
        o = self.o
        scores = generation._process_logits(logits, r.ids, r.ids.shape[1], o.repetition_penalty, o.min_length, o.eos_token_id)
        if o.do_sample:
            probs = generation._warp_logits(scores, o.temperature, o.top_p).softmax(dim=-1)
            nxt = torch.multinomial(probs, num_samples=1, generator=r.generator).squeeze(1)
        else:
            nxt = scores.argmax(dim=-1)
        r.ids = torch.cat([r.ids, nxt[:, None]], dim=-1)
        r.pending = int(nxt)
        done = o.eos_token_id is not None and r.pending == o.eos_token_id
        done = done or bool(o.stop_sequences and generation._ends_in_stop(r.ids, o.stop_sequences)[0])
        return done or generation._stop(o.stopping_criteria, r.ids, scores) or r.ids.shape[1] >= r.max_new

    def run(self):
        """step until the queue and the slots are empty: [(handle, ids)] in the order the requests finished"""
        out = []
        while not self.idle():
            out += self.step()
        for s in self.done_slots:
            self.cache.release(s)
            self.free.append(s)
        self.done_slots = []
        return out
