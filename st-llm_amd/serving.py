"""Continuous batching: a fixed set of KV-cache slots, requests admitted into free slots while the others keep decoding.

`generate()` fixes its batch when it starts: a row that finished is fed pad tokens until the slowest row is done, and a new prompt waits for the whole
batch.  The Engine owns one KVCache of `slots` rows instead.  Every step it frees the slots of finished requests, admits queued requests into free slots
(FIFO) and runs ONE pass of the decoder:

  * a step WITH admissions is LlamaModel.step_segments: the step's tokens packed as [T, D] — one token for every running request, the whole remaining
    prompt of every admitted one — on hip.kv_append_segments / hip.attention_segments.  No pad rows; running rows do not stall.
  * a step WITHOUT admissions is LlamaModel.decode_step on the slot cache, the GEMV path that a fixed batch takes (quantised decode weights included).
    Free slots ride along as don't-care rows; their length is put back to 0 (with a base: to the base's length) afterwards.

Selection is per request, with generate()'s own processors (generation._process_logits / _warp_logits) on that request's ids and step count: a request
generates the ids that generate() gives for it alone (greedy; sampling with its own generator).

Engine(state="device") keeps that per-request state on the device instead: a [slots, 4] table (live, n_gen, max_new, pending), the
generated ids [slots, max_new] and the stop sequences.  ONE hip.select_slots launch behind the pass selects for every served slot with its own step count,
appends the token and settles whether the request is finished; the next step's embeddings are gathered from the table's `pending` column.  The host reads
the table once per step, and a request's ids once, when it finishes.  A request generates the ids of generate(selection="device") for it alone.

Engine(base=prefix) serves many questions about ONE prefilled video without copying it: the slot cache is prefix.share(rows=slots, ...), every
slot holds only the positions behind the prefix, an admission copies nothing, a step with admissions runs hip.attention_segments_shared (the prefix's K / V read
once for all packed rows) and a step without runs decode_step's shared-prefix attention.  A released or idle slot sits at the prefix's length, not at 0.

Engine(num_beams=nb) serves beam search: `slots` keeps meaning concurrent requests, the cache has slots * nb rows and the request in slot g
owns rows [g * nb, (g + 1) * nb).  A prompt is admitted as ONE segment into row g * nb; hip.kv_reorder_rows (one call per layer and step for all running
requests, none when every table is the identity) fans its K / V out to the sibling rows and later lets the rows follow the chosen beams, moving only the
positions behind the prompt; generation._BeamRequest is generate()'s beam scorer per request, fed by the torch candidates (state="host") or by ONE
hip.beam_candidates_rows launch and one read of its candidate buffer (state="device").  A request returns the ids of generate(num_beams=nb) for it alone.

Not served (they raise): do_sample with beams, selection="device" among the options (the device path of the Engine is state="device"), generate()'s share_prefix option,
return_cache, a `prefix` with a base of its own, more than one base per Engine (submit(prefix=) other than the Engine's base); with state="device" also
stopping_criteria (Python callables need the ids on the host) and sync_every != 1.  No paged blocks, no preemption: a request must fit `max_len` positions
when it is submitted and keeps its slot until it finishes."""
import collections

import torch

from . import generation


class _Request:
    __slots__ = ("handle", "emb", "prefix", "max_new", "generator", "slot", "ids", "pending", "beam", "index", "prompt_end")

    def __init__(self, handle, emb, prefix, max_new, generator):
        self.handle, self.emb, self.prefix, self.max_new, self.generator = handle, emb, prefix, max_new, generator
        self.slot, self.pending = None, None
        # num_beams > 1: the scorer state (generation._BeamRequest); `pending` is then the list of the beams' next tokens and `index` the beam each of
        # them continues (None: the admission step, whose beams all continue the prompt's one row); prompt_end: the prompt's end in the slot buffers
        self.beam, self.index, self.prompt_end = None, None, 0
        self.ids = torch.zeros((1, 0), dtype=torch.long, device=emb.device)   # on the device of the logits, as generate() keeps them


class Engine:
    """Engine(lm_wrapper, slots, max_len, **options): `lm_wrapper` is what generate() runs on (`.model` a LlamaModel, `.logits_from`), `options` are
    generate()'s sampling and stopping options (generation.Options); use_cache and selection == "torch" only.
    num_beams > 1: every request searches num_beams beams in slots * num_beams cache rows (module docstring; do_sample raises, as in generate()).
    state: "host" (default) selects per request on the host with generate()'s processors; "device" keeps the per-request selection state on the device
    and selects for all slots in one hip.select_slots launch (see the module docstring).
    base: a one-row uniform KVCache without a base of its own (Chat.prefill_video(...).cache) that EVERY request sits behind; it is held by reference and only
    read.  max_len keeps counting total positions (the base's included)."""

    def __init__(self, lm_wrapper, slots, max_len, device=None, state="host", base=None, **options):
        o = generation.Options(**options)
        if state not in ("host", "device"):
            raise ValueError(f"serving.Engine: state must be 'host' or 'device', got {state!r}")
        nb = self.nb = int(o.num_beams)
        assert nb >= 1
        if nb > 1 and o.do_sample:
            raise NotImplementedError("serving.Engine(num_beams > 1, do_sample=True): beam-sample is not served (generate() has none either); sample with "
                                      "num_beams=1, or search the beams with do_sample=False")
        if o.selection != "torch":
            raise NotImplementedError("serving.Engine: selection='device' is generate()'s fixed-batch path (stllm_select_tokens takes one step index for all "
                                      "rows); the Engine selects on the device with Engine(..., state='device')")
        if not o.use_cache:
            raise ValueError("serving.Engine: needs use_cache (the slots ARE the KV cache)")
        if o.share_prefix or o.return_cache or o.return_lengths:
            raise NotImplementedError("serving.Engine: share_prefix / return_cache / return_lengths are generate()'s")
        self.o = o._replace(stop_sequences=list(o.stop_sequences) if o.stop_sequences else None)
        self.m, self.lm = lm_wrapper, lm_wrapper.model
        self.device = torch.device(device) if device is not None else self.lm.embed_tokens.weight.device
        assert slots >= 1 and max_len >= 2
        if nb > 1:
            from . import hip
            if not hip.beam_rows_available(self.device):
                raise NotImplementedError("serving.Engine(num_beams > 1) needs hip.kv_reorder_rows / hip.beam_candidates_rows, which this backend does not "
                                          f"provide for {self.device}; generate(num_beams=...) serves one request at a time")
            if nb > 16:
                raise NotImplementedError(f"serving.Engine(num_beams={nb}): stllm_kv_reorder_rows holds the rows of a request in registers, 16 at the most")
        self.base = base
        rows = slots * nb                     # the request in slot g owns the cache rows [g * nb, (g + 1) * nb): its beams
        if base is not None:
            if base.base is not None or base.lens is not None or base.batch != 1:
                raise NotImplementedError("serving.Engine(base=): a one-row uniform KVCache without a base")
            if max_len <= base.len:
                raise ValueError(f"serving.Engine(base=): max_len {max_len} counts total positions and the base holds {base.len}")
            assert base.qkv[0].device == self.device, "serving.Engine(base=): the base lives on the Engine's device"
            self.cache = base.share(rows=rows, max_new=max_len - base.len)    # every row at the base's length; nothing is copied
        else:
            self.cache = self.lm.new_cache(rows, max_len, self.device)
            self.cache.set_lens([0] * rows)
        self.queue = collections.deque()
        self.running = {}                 # slot -> _Request
        self.done_slots = []              # slots whose request finished in the last step: released at the start of the next one
        self.free = list(range(slots))
        self.handles = 0
        self.steps = collections.Counter()   # "segments" / "decode": the passes run so far
        self.state = state
        if nb > 1:
            self._init_beams()
        elif state == "device":
            self._init_device_state(slots)

    # ---- requests ------------------------------------------------------------------------------------------------------------------------------
    def submit(self, inputs_embeds, prefix=None, max_new_tokens=None, generator=None):
        """queue a request: inputs_embeds [S, D] (S >= 1), the prompt — or, with `prefix` (a one-row uniform KVCache without a base, e.g.
        Chat.prefill_video(...).cache, only ever read), what follows the prefix's positions.  generator: the request's own torch.Generator for do_sample
        (default: the Engine's `generator` option).  Raises if prefix + prompt + max_new_tokens does not fit a slot.  Returns the handle.
        An Engine with a base: every request sits behind the base; `prefix` is None or that same object, anything else raises ValueError."""
        max_new = self.o.max_new_tokens if max_new_tokens is None else int(max_new_tokens)
        assert inputs_embeds.dim() == 2 and inputs_embeds.shape[0] >= 1 and max_new >= 1
        P = 0
        if self.base is not None:
            if prefix is not None and prefix is not self.base:
                raise ValueError("serving.Engine(base=).submit(prefix=): one base per Engine — every request sits behind the Engine's base, so prefix is "
                                 "None or that same cache")
            P, prefix = self.base.len, None      # nothing to load at admission: the slot reads the base
        elif prefix is not None:
            if prefix.base is not None or prefix.lens is not None or prefix.batch != 1:
                raise NotImplementedError("serving.Engine.submit(prefix=): a one-row uniform KVCache without a base")
            P = prefix.len
        if self.nb > 1 and self.state == "device":
            # the history table [rows, longest budget so far] shares the LDS with a logits row in every hip.beam_candidates_rows launch: a budget that
            # does not fit is refused here, not by a launch in the middle of run() with other requests in flight
            from . import hip
            if not hip.beam_rows_fit(self.m.vocab_size, max(self.ld_hist, max_new)):
                raise ValueError(f"serving.Engine(state='device').submit: max_new_tokens={max_new} ids of history and the {self.m.vocab_size} logits of a row "
                                 f"do not fit the {hip.SEL_LDS_BYTES} bytes of LDS that hip.beam_candidates_rows may take; use state='host'")
        need = P + inputs_embeds.shape[0] + max_new - 1      # the last generated token is never fed
        if need > self.cache.max_len:
            raise ValueError(f"serving.Engine.submit: the request needs {need} positions (prefix + prompt + max_new_tokens - 1), a slot holds {self.cache.max_len}")
        if self.nb > 1:
            # the history table of the device state is built on the host and uploaded whole every step ([rows, ld_hist] int32: a few KiB at the budgets
            # served; an incremental table on the device would be select_slots' way, and is not built)
            self.ld_hist = max(self.ld_hist, max_new)
        elif self.state == "device" and max_new > self.d_ids.shape[1]:   # a longer budget than any so far: widen the id table (a device copy, no read)
            ids = torch.zeros((self.d_ids.shape[0], max_new), dtype=torch.int32, device=self.device)
            ids[:, :self.d_ids.shape[1]] = self.d_ids
            self.d_ids = ids
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
        if self.nb > 1:
            return self._step_beams()
        if self.state == "device":
            return self._step_device()
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
        self._release_done()
        return out

    # ---- state="device" ------------------------------------------------------------------------------------------------------------------------
    def _init_device_state(self, slots):
        from . import hip
        o = self.o
        if o.stopping_criteria is not None:
            raise NotImplementedError("serving.Engine(state='device'): stopping_criteria are Python callables on host ids; use stop_sequences, or state='host'")
        if int(o.sync_every) != 1:
            raise NotImplementedError("serving.Engine(state='device'): sync_every != 1 is not served (the state table is read every step)")
        dev = self.device
        self.d_state = torch.zeros((slots, 4), dtype=torch.int32, device=dev)     # (live, n_gen, max_new, pending) per slot
        self.d_state[:, 3] = o.pad_token_id
        self.d_ids = torch.zeros((slots, max(1, int(o.max_new_tokens))), dtype=torch.int32, device=dev)
        self.d_pending = torch.empty(slots, dtype=torch.int32, device=dev)        # the gather's index operand: a dense copy of the pending column
        self.d_u = torch.zeros(slots, dtype=torch.float32, device=dev)
        self.d_stops = self.d_stop_len = None
        stops = [s.reshape(-1).tolist() for s in (o.stop_sequences or []) if s.numel()]
        if stops:
            table = torch.zeros((len(stops), max(len(s) for s in stops)), dtype=torch.int32)
            for j, s in enumerate(stops):
                table[j, :len(s)] = torch.tensor(s, dtype=torch.int32)
            self.d_stops = table.to(dev)
            self.d_stop_len = torch.tensor([len(s) for s in stops], dtype=torch.int32).to(dev)
        self._h2d = lambda rows: hip.h2d(torch.tensor(rows, dtype=torch.int32), dev)   # a small int32 table, uploaded without stalling the host

    def _release_done(self):
        for s in self.done_slots:
            for row in range(s * self.nb, (s + 1) * self.nb):
                self.cache.release(row)
            self.free.append(s)
            if self.state == "device" and self.nb == 1:   # the slot's row: dead, and what it feeds while it rides along is pad (an upload, never a read)
                self.d_state[s].copy_(self._h2d([0, 0, 0, self.o.pad_token_id]))
        self.done_slots = []

    def _read_state(self):
        """the ONE device-to-host transfer of a state="device" step: the [slots, 4] table as lists"""
        return self.d_state.tolist()

    def _step_device(self):
        """step() with the selection state on the device: release, admit, one decoder pass fed from the table's `pending` column, ONE hip.select_slots launch,
        one read of the table"""
        from . import hip
        o, K, dev = self.o, self.cache.batch, self.device
        self._release_done()
        self.free.sort()
        admitted = []
        while self.queue and self.free:
            r = self.queue.popleft()
            r.slot = self.free.pop(0)
            if r.prefix is not None:
                self.cache.load_row(r.slot, r.prefix)
            self.d_state[r.slot].copy_(self._h2d([1, 0, r.max_new, o.pad_token_id]))
            admitted.append(r)
        if not admitted and not self.running:
            return []
        running = [self.running[s] for s in sorted(self.running)]
        table = self.lm.embed_tokens.weight
        src = [-1] * K                            # slot -> its row of this step's logits
        if admitted:
            parts, segments = [], []
            if running:
                pending = torch.index_select(self.d_state[:, 3], 0, self._h2d([r.slot for r in running]))
                parts.append(hip.gather_rows(table, pending.to(table.device)).to(dev))
                segments += [(r.slot, 1) for r in running]
            for r in admitted:
                parts.append(r.emb)
                segments.append((r.slot, r.emb.shape[0]))
                self.running[r.slot] = r
                r.emb = None
            _, h16 = self.lm.step_segments(torch.cat(parts) if len(parts) > 1 else parts[0], self.cache, segments)
            served = running + admitted
            logits = self.m.logits_from(h16, len(served), 1)[:, 0]
            for i, r in enumerate(served):
                src[r.slot] = i
            self.steps["segments"] += 1
        else:
            self.d_pending.copy_(self.d_state[:, 3])
            _, h16 = self.lm.decode_step(hip.gather_rows(table, self.d_pending.to(table.device)).to(dev).view(K, 1, -1), self.cache)
            for s in self.free:                   # the free slots rode along: whatever they appended is don't-care
                self.cache.release(s)
            logits = self.m.logits_from(h16, K, 1)[:, 0]
            served = running
            for r in served:
                src[r.slot] = r.slot
            self.steps["decode"] += 1
        if o.do_sample:                           # one draw per served request from ITS generator: the stream generate(selection="device") consumes for it alone
            draws = [torch.rand(1, generator=r.generator, device=r.generator.device if r.generator is not None else dev) for r in served]
            if all(d.device.type == "cpu" for d in draws):
                u = torch.zeros(K)
                u[torch.tensor([r.slot for r in served])] = torch.cat(draws)
                self.d_u.copy_(hip.h2d(u, dev))   # one upload per step
            else:
                for r, d in zip(served, draws):
                    self.d_u[r.slot:r.slot + 1].copy_(d)
        hip.select_slots(logits, self._h2d(src), self.d_state, self.d_ids, penalty=o.repetition_penalty, min_length=o.min_length, eos_id=o.eos_token_id,
                         pad_id=o.pad_token_id, sample=o.do_sample, temperature=o.temperature, top_p=o.top_p, u=self.d_u if o.do_sample else None,
                         stops=self.d_stops, stop_len=self.d_stop_len)
        state = self._read_state()
        finished = []
        for r in served:
            live, n_gen = state[r.slot][0], state[r.slot][1]
            if not live:
                finished.append((r.handle, self.d_ids[r.slot, :n_gen].long()))
                del self.running[r.slot]
                self.done_slots.append(r.slot)
        if finished and dev.type == "cuda":
            hip.gemm_workspace_check(dev, wait=True)   # as generation._finish: no id leaves behind a timed-out split-K exchange
        return finished

    # ---- num_beams > 1 ---------------------------------------------------------------------------------------------------------
    def _init_beams(self):
        o = self.o
        if self.state == "device":
            if o.stopping_criteria is not None:
                raise NotImplementedError("serving.Engine(state='device'): stopping_criteria are Python callables on host ids; use stop_sequences, or state='host'")
            if int(o.sync_every) != 1:
                raise NotImplementedError("serving.Engine(state='device'): sync_every != 1 is not served (the candidates are read every step)")
        self.ld_hist = max(1, int(o.max_new_tokens))   # columns of the history table that state="device" uploads: the longest budget so far

    def _embed(self, toks):
        """the embedding rows f32 [len(toks), D] of a host list of token ids, on the Engine's device: the lookup of the step() / _step_device() in use"""
        if self.state == "device":
            from . import hip
            table = self.lm.embed_tokens.weight
            return hip.gather_rows(table, hip.h2d(torch.tensor(toks, dtype=torch.int32), self.device).to(table.device)).to(self.device)
        return self.lm.embed_tokens(torch.tensor(toks).view(-1, 1))[:, 0].float().to(self.device)

    def _read_candidates(self, buf):
        """the ONE device-to-host transfer of a state="device" beam step: the [2, rows, 2 * num_beams] candidate buffer (scores as fp32 bits | tokens)"""
        return buf.cpu()

    def _step_beams(self):
        """step() with num_beams > 1.  The request in slot g owns the cache rows [g * nb, (g + 1) * nb), one per beam.  Release and admit as step() does
        (the prompt is ONE segment into row g * nb); ONE hip.kv_reorder_rows call per layer lets every running request's rows follow the beams chosen in
        its last step (the first one: a fan-out of the prompt's positions from row g * nb; later ones: the positions behind the prompt only; none at all
        when every table is the identity); one decoder pass (a running request feeds num_beams one-token rows); then generate()'s beam scorer per request
        (generation._BeamRequest) — on the torch candidates of the request's rows (state="host"), or on ONE hip.beam_candidates_rows launch for all
        served requests and one read of its candidate buffer (state="device")."""
        from . import hip
        o, nb, dev, cache = self.o, self.nb, self.device, self.cache
        K, P, on_device = cache.batch, cache.base_len, self.state == "device"
        self._release_done()
        self.free.sort()
        running = [self.running[s] for s in sorted(self.running)]
        admitted = []
        while self.queue and self.free:
            r = self.queue.popleft()
            r.slot = self.free.pop(0)
            if r.prefix is not None:
                cache.load_row(r.slot * nb, r.prefix)
            r.beam = generation._BeamRequest(o, r.max_new, torch.device("cpu") if on_device else dev)
            admitted.append(r)
        if not admitted and not running:
            return []

        def tab(v):
            return hip.h2d(torch.tensor(v, dtype=torch.int32), dev)
        # the re-order: the host knows every table; positions are local to the slot buffers (behind the base, when there is one)
        lens = cache.row_lens()
        src, lo, hi = list(range(K)), [0] * (K // nb), [0] * (K // nb)
        for r in running:
            g0 = r.slot * nb
            n = lens[g0] - P
            if r.index is None:                       # first step behind the admission: the siblings get the prompt's K / V, and their length
                r.prompt_end = n
                src[g0:g0 + nb], lo[r.slot], hi[r.slot] = [g0] * nb, 0, n
                lens[g0:g0 + nb] = [lens[g0]] * nb
            elif r.index != list(range(nb)):          # the first prompt_end positions are the same in all rows and never move again
                src[g0:g0 + nb], lo[r.slot], hi[r.slot] = [g0 + i for i in r.index], r.prompt_end, n
        span = max(h - l for l, h in zip(lo, hi))
        if span > 0:
            src_t, lo_t, hi_t = tab(src), tab(lo), tab(hi)
            for buf in cache.qkv:
                hip.kv_reorder_rows(buf, src_t, lo_t, hi_t, nb=nb, max_span=span)
            self.steps["reorder"] += 1
        cache.set_lens(lens)
        # one decoder pass; rows_of[i]: the logits rows of served request i's beams
        if admitted:
            parts, segments = [], []
            if running:
                parts.append(self._embed([t for r in running for t in r.pending]))
                segments += [(r.slot * nb + j, 1) for r in running for j in range(nb)]
            for r in admitted:
                parts.append(r.emb)
                segments.append((r.slot * nb, r.emb.shape[0]))
                self.running[r.slot] = r
                r.emb = None
            _, h16 = self.lm.step_segments(torch.cat(parts) if len(parts) > 1 else parts[0], cache, segments)
            logits = self.m.logits_from(h16, len(segments), 1)[:, 0]
            rows_of = [list(range(i * nb, (i + 1) * nb)) for i in range(len(running))] + [[len(running) * nb + j] * nb for j in range(len(admitted))]
            self.steps["segments"] += 1
        else:
            toks = [o.pad_token_id] * K
            for r in running:
                toks[r.slot * nb:(r.slot + 1) * nb] = r.pending
            _, h16 = self.lm.decode_step(self._embed(toks).view(K, 1, -1), cache)
            for s in self.free:                       # the free groups rode along: whatever they appended is don't-care
                for row in range(s * nb, (s + 1) * nb):
                    cache.release(row)
            logits = self.m.logits_from(h16, K, 1)[:, 0]
            rows_of = [list(range(r.slot * nb, (r.slot + 1) * nb)) for r in running]
            self.steps["decode"] += 1
        served = running + admitted
        V = logits.shape[-1]
        if on_device:
            k = 2 * nb
            if k > min(32, V):
                raise ValueError(f"serving.Engine(state='device'): 2 * num_beams = {k} candidates per beam exceed min(32, vocabulary {V})")
            src_l, n_prev = [-1] * K, [0] * K
            scores, hist = torch.zeros(K, dtype=torch.float32), torch.zeros((K, self.ld_hist), dtype=torch.int32)
            for r, rows in zip(served, rows_of):
                g0, n = r.slot * nb, r.beam.ids.shape[1]
                src_l[g0:g0 + nb], n_prev[g0:g0 + nb] = rows, [n] * nb
                scores[g0:g0 + nb], hist[g0:g0 + nb, :n] = r.beam.beam_scores, r.beam.ids
            buf = torch.empty((2, K, k), dtype=torch.int32, device=dev)   # scores (as fp32 bits) and tokens side by side: one copy back
            hip.beam_candidates_rows(logits, tab(src_l), hip.h2d(scores, dev), k, prev=hip.h2d(hist, dev), n_prev=tab(n_prev), penalty=o.repetition_penalty,
                                     min_length=o.min_length, eos_id=o.eos_token_id, cand_score=buf[0].view(torch.float32), cand_token=buf[1])
            host = self._read_candidates(buf)
            cand_s, cand_t = host[0].view(torch.float32), host[1]
        finished = []
        for i, (r, rows) in enumerate(zip(served, rows_of)):
            g0 = r.slot * nb
            if on_device:
                cs, ct, cb = r.beam.merge(cand_s[g0:g0 + nb].reshape(-1), cand_t[g0:g0 + nb].reshape(-1), nb, V)
            else:
                cs, ct, cb = r.beam.candidates(logits[torch.tensor(rows, device=logits.device)].float())
            tokens, index = r.beam.process(cs, ct, cb)
            if r.beam.finished:
                finished.append((r.handle, r.beam.finalize().to(dev)))
                del self.running[r.slot]
                self.done_slots.append(r.slot)
            else:
                r.pending, r.index = tokens, (None if i >= len(running) else index)
        if finished and dev.type == "cuda":
            hip.gemm_workspace_check(dev, wait=True)   # as generation._finish: no id leaves behind a timed-out split-K exchange
        return finished
