"""Token generation on the KV cache: what `Chat.answer` asks of `llama_model.generate(...)` in the reference
(stllm/conversation/conversation.py:231-243: inputs_embeds, max_new_tokens, stopping_criteria, num_beams, do_sample,
min_length, top_p, repetition_penalty, length_penalty, temperature; demo.py:58-66 runs it with num_beams=5, do_sample=False).

The reference delegates to HuggingFace transformers == 4.28.0 (requirement.txt), which is not part of /root/reference; this
module restates the published algorithm of `GenerationMixin.greedy_search / sample / beam_search` + `BeamSearchScorer` for
the argument subset above (one return sequence, no beam groups):

  * logits processors, in HF's order: RepetitionPenaltyLogitsProcessor, MinLengthLogitsProcessor; sampling adds the warpers
    TemperatureLogitsWarper, TopPLogitsWarper;
  * greedy / sampling: finished rows emit `pad_token_id`; stop when every row has emitted EOS, a stopping criterion fires, or
    `max_new_tokens` tokens exist;
  * beam search: scores are log-softmax + running beam score, top 2*num_beams candidates per step, candidates ending in EOS
    become hypotheses (score = sum_logprobs / len ** length_penalty, only if ranked inside the first num_beams), the rest
    refill the beams; a batch row is done when num_beams hypotheses exist and the best running score cannot beat the worst
    of them (early_stopping=False heuristic: best_sum_logprobs / cur_len ** length_penalty); `finalize` adds the open beams
    and returns the best hypothesis followed by EOS when it ended early;
  * the KV cache is re-ordered by `beam_idx` after every step (`LlamaForCausalLM._reorder_cache`, spec
    modeling_llama_mem.py:747-752) — here one index_select per layer on the fused QKV cache rows that are in use.

Ragged batches (`lengths=`: per-row prompt lengths of a right-padded `inputs_embeds`): ONE prefill fills a ragged KV cache (KVCache.lens), the first logits
come from row lengths[b] - 1 of each prompt, beams inherit their prompt's length, and every step appends token b at its own position — each row generates
exactly as its unpadded prompt would alone.  `stop_sequences` finishes rows one by one (the reference's StoppingCriteriaSub looks at row 0 only and stops
the whole batch, which is wrong for more than one prompt).

With `inputs_embeds` and no `input_ids` the sequences HF scores start empty, so every length below counts generated tokens
only.  The prompt is prefilled ONCE and its cache rows are replicated to the beams (HF prefills num_beams identical copies).
"""
import collections

import torch


class _BeamHypotheses:
    """transformers 4.28 generation/beam_search.py BeamHypotheses (early_stopping=False)."""

    def __init__(self, num_beams, length_penalty):
        self.num_beams, self.length_penalty = num_beams, length_penalty
        self.beams = []
        self.worst_score = 1e9

    def __len__(self):
        return len(self.beams)

    def add(self, hyp, sum_logprobs):
        score = sum_logprobs / (hyp.shape[-1] ** self.length_penalty)
        if len(self) < self.num_beams or score > self.worst_score:
            self.beams.append((score, hyp))
            if len(self) > self.num_beams:
                sorted_scores = sorted([(s, idx) for idx, (s, _) in enumerate(self.beams)])
                del self.beams[sorted_scores[0][1]]
                self.worst_score = sorted_scores[1][0]
            else:
                self.worst_score = min(score, self.worst_score)

    def is_done(self, best_sum_logprobs, cur_len):
        if len(self) < self.num_beams:
            return False
        return self.worst_score >= best_sum_logprobs / cur_len ** self.length_penalty


def _process_logits(scores, ids, cur_len, repetition_penalty, min_length, eos_token_id):
    """RepetitionPenaltyLogitsProcessor then MinLengthLogitsProcessor (HF order), on [rows, vocab] fp32 scores."""
    if repetition_penalty != 1.0 and ids.shape[1] > 0:
        s = torch.gather(scores, 1, ids)
        s = torch.where(s < 0, s * repetition_penalty, s / repetition_penalty)
        scores = scores.scatter(1, ids, s)
    if eos_token_id is not None and cur_len < min_length:
        scores = scores.clone()
        scores[:, eos_token_id] = -float("inf")
    return scores


def _warp_logits(scores, temperature, top_p):
    """TemperatureLogitsWarper then TopPLogitsWarper (min_tokens_to_keep = 1)."""
    if temperature != 1.0:
        scores = scores / temperature
    if top_p is not None and top_p < 1.0:
        sorted_logits, sorted_indices = torch.sort(scores, descending=False)
        cumulative = sorted_logits.softmax(dim=-1).cumsum(dim=-1)
        remove = cumulative <= (1 - top_p)
        remove[..., -1:] = False
        scores = scores.masked_fill(remove.scatter(1, sorted_indices, remove), -float("inf"))
    return scores


def _stop(stopping_criteria, ids, scores):
    return stopping_criteria is not None and any(bool(sc(ids, scores)) for sc in stopping_criteria)


def _ends_in_stop(ids, stop_sequences):
    """bool [rows]: the row's ids end in one of the stop sequences (1-D id tensors)"""
    hit = torch.zeros(ids.shape[0], dtype=torch.bool, device=ids.device)
    for seq in stop_sequences:
        n = seq.numel()
        if 0 < n <= ids.shape[1]:
            hit |= (ids[:, -n:] == seq.to(ids.device).view(1, n)).all(dim=1)
    return hit


# the sampling and stopping options of generate() (see its docstring) and their defaults, stated once: every public entry builds one Options from its keywords
_DEFAULTS = dict(max_new_tokens=16, num_beams=1, do_sample=False, min_length=0, top_p=1.0, temperature=1.0, repetition_penalty=1.0, length_penalty=1.0,
                 stopping_criteria=None, eos_token_id=2, pad_token_id=0, use_cache=True, generator=None, stop_sequences=None, return_lengths=False,
                 share_prefix=False, selection="torch", sync_every=1, return_cache=False)
Options = collections.namedtuple("Options", list(_DEFAULTS), defaults=list(_DEFAULTS.values()))
# generate(return_cache=True): what a later turn continues from.  cache: the working KV cache, truncated per row to the positions whose K / V certainly belong
# to the row's own tokens — prompt_len_b + n_gen_b - 1 (a finished row was fed pads meanwhile: dropped); pending: LongTensor [B] on the CPU, every row's
# last generated id, which has not been fed yet — the first token of the row's next prompt
Continuation = collections.namedtuple("Continuation", "cache pending")


class _CacheStepper:
    """next-token logits from the model: prefill once, then one decode step per token; rows can be re-ordered (beams)."""

    def __init__(self, lm_wrapper, inputs_embeds, opts, prefix=None, lengths=None):
        """prefix: a KVCache holding the prompts' first positions (a prefilled video; one row per prompt, or with `lengths` one row shared by all), left
        as it was: the work happens on a fork (a copy per row) or, share_prefix, on a cache that reads it where it is (KVCache.share).  A prefix whose rows
        have different lengths (prefix.lens set: one row per prompt, the rows of an earlier ragged batch) is forked and extended by LlamaModel.extend's
        ragged path; it cannot be shared.
        lengths: row b of the right-padded `inputs_embeds` holds lengths[b] tokens -> a ragged cache; the beams of a prompt inherit its length."""
        self.m, self.lm = lm_wrapper, lm_wrapper.model
        self.use_cache, self.rep = opts.use_cache, opts.num_beams      # rep: beams per prompt
        share, room = opts.share_prefix, opts.max_new_tokens
        emb = inputs_embeds.float()
        B, S, _ = emb.shape
        if share and not self.use_cache:
            raise ValueError("generate(share_prefix=True) needs use_cache: what is shared is the KV cache of the prompt's first positions")
        if lengths is not None:
            if not self.use_cache:
                raise ValueError("generate(lengths=...): ragged batches need use_cache")
            lengths = [int(n) for n in lengths]
            assert len(lengths) == B and all(1 <= n <= S for n in lengths)
            if prefix is not None and prefix.batch not in (1, B):
                raise ValueError("generate(prefix=..., lengths=...): the prefix holds one row shared by every prompt, or one row per prompt")
            if share and prefix is None and self.rep > 1:
                raise NotImplementedError("generate(share_prefix=True, lengths=...) with beams needs prefix=: a ragged prompt cache cannot be a shared base")
        elif prefix is not None and (not self.use_cache or prefix.batch != B):
            raise ValueError("generate(prefix=...): needs use_cache and one prefix row per prompt")
        if prefix is not None and prefix.lens is not None and (share or prefix.batch != B):
            raise NotImplementedError("generate(prefix=<a cache whose rows have different lengths>): one prefix row per prompt, share_prefix off "
                                      "(ragged rows cannot be a shared base)")

        def per_beam(t):                          # row b -> rows [b * rep, (b + 1) * rep)
            return t.repeat_interleave(self.rep, dim=0) if self.rep > 1 else t
        if not self.use_cache:
            self.emb = per_beam(emb)
            self.logits = self.m.forward(samples=None, inputs_embeds=self.emb).logits[:, -1].float()
            return
        # the cache of the B prompt rows, with room for the prompt and the new tokens ...
        if prefix is None:
            cache = self.lm.new_cache(B, S + room, emb.device)
        elif share:
            cache = prefix.share(rows=B, max_new=S + room)
        else:
            cache = prefix.fork(rows=B, max_len=prefix.len + S + room)
        # ... filled in ONE pass: behind the prefix, or from position 0 (a right-padded mask makes the cache ragged)
        if prefix is not None:
            _, h16 = self.lm.extend(emb, cache, lengths=lengths)
        else:
            mask = None if lengths is None else (torch.arange(S)[None, :] < torch.tensor(lengths)[:, None]).long()
            _, h16 = self.lm.prefill(emb, mask, cache=cache)
        # the first logits are those of every prompt's LAST real token
        h16 = h16.view(B, S, -1)
        last = h16[:, -1] if lengths is None else h16[torch.arange(B), torch.tensor(lengths) - 1]
        logits = self.m.logits_from(last.contiguous(), B, 1)[:, 0]
        if self.rep > 1:
            # the beams of a prompt: copies of its cache row (fork), or, share_prefix, readers of ONE base — the prefix when there is one (the rows
            # behind it are copied per beam), else the prompt's own cache, never replicated; max_new counts the positions behind that base
            cache = cache.share(rows=B * self.rep, max_new=cache.max_len - (cache.base_len or cache.len)) if share else cache.fork(rows=B * self.rep)
        self.cache, self.logits = cache, per_beam(logits).float()

    def advance(self, next_tokens, beam_idx=None, on_device=False):
        """append `next_tokens` [rows] (after re-ordering the rows by `beam_idx`) and compute the next logits.
        on_device: `next_tokens` is a contiguous int32 tensor on the device and stays there — the embedding rows are gathered by it directly"""
        if on_device:
            from . import hip
            tok = hip.gather_rows(self.lm.embed_tokens.weight, next_tokens).view(next_tokens.numel(), 1, -1)
        else:
            tok = self.lm.embed_tokens(next_tokens.view(-1, 1).cpu())
        if self.use_cache:
            if beam_idx is not None and not torch.equal(beam_idx.cpu(), torch.arange(beam_idx.numel())):
                n = self.cache.len - self.cache.base_len   # a shared base is common to the beams of a prompt: only the positions behind it move
                idx = beam_idx.to(self.cache.qkv[0].device)
                for buf in self.cache.qkv:        # _reorder_cache: past.index_select(0, beam_idx), only the rows in use
                    buf[:, :n] = buf[:, :n].index_select(0, idx)
                if self.cache.lens is not None:   # ragged: n = max(lens); the lengths travel with their rows (beams stay inside their prompt)
                    self.cache.lens = [self.cache.lens[i] for i in beam_idx.tolist()]
            _, h16 = self.lm.decode_step(tok, self.cache)
            self.logits = self.m.logits_from(h16, next_tokens.numel(), 1)[:, 0].float()
        else:
            if beam_idx is not None:
                self.emb = self.emb.index_select(0, beam_idx.to(self.emb.device))
            self.emb = torch.cat([self.emb, tok.to(self.emb.device)], dim=1)
            self.logits = self.m.forward(samples=None, inputs_embeds=self.emb).logits[:, -1].float()


@torch.no_grad()
def generate(lm_wrapper, inputs_embeds, max_new_tokens=16, num_beams=1, do_sample=False, min_length=0, top_p=1.0,
             temperature=1.0, repetition_penalty=1.0, length_penalty=1.0, stopping_criteria=None, eos_token_id=2,
             pad_token_id=0, use_cache=True, generator=None, prefix=None, lengths=None, stop_sequences=None, return_lengths=False,
             share_prefix=False, selection="torch", sync_every=1, return_cache=False):
    """Returns the generated ids [B, n] (the prompt has no ids), HF semantics as described in the module docstring.
    prefix: a KVCache that already holds the first positions of every prompt (LlamaModel.prefill(cache=...) / Chat.prefill_video); `inputs_embeds` is then
    the remainder of the prompt, appended behind it in one pass (LlamaModel.extend).  The prefix is left unchanged.
    lengths: per-row token counts of a right-padded `inputs_embeds` (a ragged batch in one call; with a prefix the prefix may hold one shared row).
    stop_sequences: list of 1-D id tensors — a row whose generated ids end in one of them is finished from that step on and emits pad_token_id, like a
    row that emitted EOS (beam search: the prompt is closed when its first beam ends in one, its open beams become hypotheses).
    return_lengths: also return the number of generated tokens per row (the rest of the row is padding).
    share_prefix: the rows that have the same first positions — the questions behind one prefix row, the beams of a prompt — read ONE physical copy of them
    (KVCache.share, hip.attention_shared) instead of owning a copy each; the beam re-ordering then moves the positions behind it only.
    Same ids up to the summation order of the attention; needs use_cache.  False (default): every row owns its copy, as always.
    selection: "torch" (default) selects every token with torch operators, as always.  "device" (opt-in) selects it with the project's
    own kernels — hip.select_tokens on the logits where `logits_from` wrote them, into column t of an int32 ids buffer that stays on the device and feeds
    the next embedding lookup; beam search takes the 2 * num_beams best candidates of every beam from hip.beam_candidates, merges them per prompt on the
    host and runs the same scorer.  Greedy and beam search give the ids of "torch" (up to fp32 rounding between near-tied scores).  Sampling draws ONE
    uniform number per row and step (torch.rand(rows, generator=generator)) and inverts the kept distribution's CDF in id order, so for the same seed its
    ids DIFFER from those of torch.multinomial; the same seed reproduces them.  A vocabulary that does not fit the LDS raises.
    sync_every: "device", num_beams == 1 only — the host reads `unfinished` back every sync_every-th step instead of every step; finished rows emit
    pad_token_id meanwhile, and the result is cut where every row had finished: the same ids.  A `stopping_criteria` callable needs the ids of every
    step and forces 1.
    return_cache: additionally return a Continuation(cache, pending) as the LAST element of the result (num_beams == 1, use_cache; both selections): the
    working cache cut per row to its own tokens, and every row's last generated id, not fed yet.  A later generate(prefix=cont.cache, lengths=...) whose
    row b starts with pending[b] continues row b (Chat.follow_up)."""
    opts = Options(max_new_tokens=max_new_tokens, num_beams=num_beams, do_sample=do_sample, min_length=min_length, top_p=top_p, temperature=temperature,
                   repetition_penalty=repetition_penalty, length_penalty=length_penalty, stopping_criteria=stopping_criteria, eos_token_id=eos_token_id,
                   pad_token_id=pad_token_id, use_cache=use_cache, generator=generator, stop_sequences=stop_sequences, return_lengths=return_lengths,
                   share_prefix=share_prefix, selection=selection, sync_every=sync_every, return_cache=return_cache)
    return _generate(lm_wrapper, inputs_embeds, opts, prefix, lengths)


def _generate(lm_wrapper, inputs_embeds, opts, prefix=None, lengths=None):
    """generate() on an Options object: the three decode loops.  They stay apart — the torch loop is what the device loop is tested against — and share
    their head (_CacheStepper) and tail (_finish) only."""
    if opts.selection not in ("torch", "device"):
        raise ValueError(f"generate(selection={opts.selection!r}): 'torch' or 'device'")
    opts = opts._replace(stop_sequences=list(opts.stop_sequences) if opts.stop_sequences else None)
    if opts.return_cache and not opts.use_cache:
        raise ValueError("generate(return_cache=True) needs use_cache: what is returned is the KV cache")
    if opts.return_cache and opts.num_beams > 1:
        raise NotImplementedError("generate(return_cache=True) with beams: the rows of the working cache are beams, not prompts (num_beams == 1 only)")
    if opts.num_beams > 1:
        return _generate_beams(lm_wrapper, inputs_embeds, opts, prefix, lengths)
    loop = _generate_device if opts.selection == "device" else _generate_torch
    return loop(lm_wrapper, inputs_embeds, opts, prefix, lengths)


def _finish(ids, n_gen, opts, cont=None):
    """the common tail of the loops.  Every token was read back on the host, so the stream is idle: a timed-out split-K exchange anywhere in this
    generate() call must not come back as plausible-looking ids.  n_gen: the number of generated tokens per row, returned on request.
    cont: the Continuation of return_cache, appended to the result."""
    if ids.device.type == "cuda":
        from . import hip
        hip.gemm_workspace_check(ids.device, wait=True)
    out = (ids, n_gen) if opts.return_lengths else (ids,)
    out = out + (cont,) if opts.return_cache else out
    return out if len(out) > 1 else out[0]


def _continuation(st, ids, n_gen, steps):
    """return_cache: `steps` tokens were selected and steps - 1 of them fed, so row b holds its prompt plus steps - 1 positions, of which the first
    n_gen[b] - 1 are its own tokens (the last one it generated is pending; what a finished row was fed afterwards is padding)"""
    cache = st.cache
    have = cache.lens if cache.lens is not None else [cache.len] * cache.batch
    cache.truncate([h - steps + n for h, n in zip(have, n_gen)])
    host = ids.cpu()
    return Continuation(cache, torch.tensor([int(host[b, n - 1]) for b, n in enumerate(n_gen)], dtype=torch.long))


def _generate_torch(lm_wrapper, inputs_embeds, o, prefix, lengths):
    """greedy search / sampling with torch operators"""
    B, dev = inputs_embeds.shape[0], inputs_embeds.device
    st = _CacheStepper(lm_wrapper, inputs_embeds, o, prefix, lengths)
    ids = torch.zeros((B, 0), dtype=torch.long, device=dev)
    unfinished = torch.ones(B, dtype=torch.long, device=dev)
    n_gen = torch.zeros(B, dtype=torch.long, device=dev)
    while True:
        scores = _process_logits(st.logits.to(dev), ids, ids.shape[1], o.repetition_penalty, o.min_length, o.eos_token_id)
        if o.do_sample:
            probs = _warp_logits(scores, o.temperature, o.top_p).softmax(dim=-1)
            nxt = torch.multinomial(probs, num_samples=1, generator=o.generator).squeeze(1)
        else:
            nxt = scores.argmax(dim=-1)
        if o.eos_token_id is not None or o.stop_sequences:
            nxt = nxt * unfinished + o.pad_token_id * (1 - unfinished)
        ids = torch.cat([ids, nxt[:, None]], dim=-1)
        n_gen = n_gen + unfinished
        if o.eos_token_id is not None:
            unfinished = unfinished * (nxt != o.eos_token_id).long()
        if o.stop_sequences:
            unfinished = unfinished * (~_ends_in_stop(ids, o.stop_sequences)).long()
        if unfinished.max() == 0 or _stop(o.stopping_criteria, ids, scores) or ids.shape[1] >= o.max_new_tokens:
            break
        st.advance(nxt)
    n_host = n_gen.tolist() if o.return_lengths or o.return_cache else None
    return _finish(ids, n_host, o, _continuation(st, ids, n_host, ids.shape[1]) if o.return_cache else None)


def _generate_beams(lm_wrapper, inputs_embeds, opts, prefix, lengths):
    """beam search; selection="device" takes the candidates of every step from hip.beam_candidates, the scorer is the same"""
    if opts.do_sample:
        raise NotImplementedError("beam-sample is not used by the reference (demo: num_beams=5, do_sample=False)")
    B, dev, nb, on_device = inputs_embeds.shape[0], inputs_embeds.device, opts.num_beams, opts.selection == "device"
    max_new_tokens, min_length, repetition_penalty, length_penalty = opts.max_new_tokens, opts.min_length, opts.repetition_penalty, opts.length_penalty
    eos_token_id, pad_token_id, stop_sequences, stopping_criteria = opts.eos_token_id, opts.pad_token_id, opts.stop_sequences, opts.stopping_criteria
    st = _CacheStepper(lm_wrapper, inputs_embeds, opts, prefix, lengths)
    ids = torch.zeros((B * nb, 0), dtype=torch.long, device=dev)
    beam_scores = torch.zeros((B, nb), dtype=torch.float32, device=dev)
    beam_scores[:, 1:] = -1e9
    beam_scores = beam_scores.view(-1)
    hyps = [_BeamHypotheses(nb, length_penalty) for _ in range(B)]
    done = [False] * B
    while True:
        cur_len = ids.shape[1]
        if on_device:
            cs, ct, cb = _device_candidates(st.logits, ids, beam_scores, B, nb, repetition_penalty=repetition_penalty, suppress_eos=cur_len < min_length,
                                            eos_token_id=eos_token_id)
        else:
            logp = st.logits.to(dev).log_softmax(dim=-1)
            logp = _process_logits(logp, ids, cur_len, repetition_penalty, min_length, eos_token_id)
            V = logp.shape[-1]
            cand = (logp + beam_scores[:, None]).view(B, nb * V)
            cand_scores, cand_tokens = torch.topk(cand, 2 * nb, dim=1, largest=True, sorted=True)
            cand_beams = torch.div(cand_tokens, V, rounding_mode="floor")
            cand_tokens = cand_tokens % V
            cs, ct, cb = cand_scores.cpu(), cand_tokens.cpu(), cand_beams.cpu()
        next_scores = torch.zeros((B, nb), dtype=torch.float32, device=dev)
        next_tokens = torch.zeros((B, nb), dtype=torch.long, device=dev)
        next_index = torch.zeros((B, nb), dtype=torch.long, device=dev)
        for b in range(B):                                   # BeamSearchScorer.process
            if done[b]:
                next_scores[b] = 0
                next_tokens[b] = pad_token_id
                next_index[b] = b * nb
                continue
            k = 0
            for rank in range(2 * nb):
                tok, sc, row = int(ct[b, rank]), float(cs[b, rank]), b * nb + int(cb[b, rank])
                if eos_token_id is not None and tok == eos_token_id:
                    if rank >= nb:
                        continue
                    hyps[b].add(ids[row].clone(), sc)
                else:
                    next_scores[b, k], next_tokens[b, k], next_index[b, k] = sc, tok, row
                    k += 1
                if k == nb:
                    break
            done[b] = done[b] or hyps[b].is_done(float(cs[b].max()), cur_len)
        beam_scores = next_scores.view(-1)
        beam_idx = next_index.view(-1)
        ids = torch.cat([ids[beam_idx], next_tokens.view(-1, 1)], dim=-1)
        if stop_sequences:
            # per prompt what a stopping criterion does to a single prompt (it looks at the first row and ends the search): the open beams become hypotheses
            hit = _ends_in_stop(ids, stop_sequences).tolist()
            for b in range(B):
                if not done[b] and hit[b * nb]:
                    for j in range(nb):
                        hyps[b].add(ids[b * nb + j].clone(), float(beam_scores[b * nb + j]))
                    done[b] = True
        if all(done) or _stop(stopping_criteria, ids, None) or ids.shape[1] >= max_new_tokens:
            break
        if on_device:
            st.advance(next_tokens.view(-1).to(torch.int32), beam_idx, on_device=True)
        else:
            st.advance(next_tokens.view(-1), beam_idx)
    # BeamSearchScorer.finalize: open beams become hypotheses, best one wins, EOS appended when it ended early
    out = []
    for b in range(B):
        if not done[b]:
            for j in range(nb):
                hyps[b].add(ids[b * nb + j], float(beam_scores[b * nb + j]))
        out.append(sorted(hyps[b].beams, key=lambda x: x[0])[-1][1])
    sent_max = min(max(len(o) for o in out) + 1, max_new_tokens)
    res = torch.full((B, sent_max), pad_token_id, dtype=torch.long, device=dev)
    for b, o in enumerate(out):
        res[b, :len(o)] = o
        if len(o) < sent_max:
            res[b, len(o)] = eos_token_id
    return _finish(res, [min(len(o) + 1, sent_max) for o in out], opts)


def _device_candidates(logits, ids, beam_scores, B, nb, *, repetition_penalty, suppress_eos, eos_token_id):
    """selection="device": what `topk` over the nb * V scores of a prompt returns, from hip.beam_candidates.  Every beam row gives its k = 2 * nb best
    (score descending, token ascending); ONE device -> host copy brings the nb * k (score, token) pairs of every prompt over, and the host merges them by
    (score descending, beam * V + token ascending).  Returns CPU tensors (scores f32, tokens, beams) [B, 2 * nb]."""
    from . import hip
    rows, k, V = B * nb, 2 * nb, logits.shape[-1]
    if k > min(32, V):
        raise ValueError(f"generate(selection='device'): 2 * num_beams = {k} candidates per beam exceed min(32, vocabulary {V})")
    n_prev = ids.shape[1]
    buf = torch.empty((2, rows, k), dtype=torch.int32, device=logits.device)   # scores (as fp32 bits) and tokens side by side: one copy back
    hip.beam_candidates(logits, beam_scores.contiguous(), k, prev=ids.to(torch.int32) if n_prev else None, n_prev=n_prev, penalty=repetition_penalty,
                        suppress_eos=suppress_eos and eos_token_id is not None, eos_id=eos_token_id, cand_score=buf[0].view(torch.float32), cand_token=buf[1])
    host = buf.cpu()
    sc, tk = host[0].view(torch.float32).view(B, nb * k), host[1].view(B, nb * k)
    beam = torch.arange(nb).repeat_interleave(k)
    cs, ct, cb = (torch.empty((B, k), dtype=dt) for dt in (torch.float32, torch.long, torch.long))
    for b in range(B):
        order = sorted(range(nb * k), key=lambda i: (-float(sc[b, i]), int(beam[i]) * V + int(tk[b, i])))[:k]
        cs[b], ct[b], cb[b] = sc[b, order], tk[b, order].long(), beam[order]
    return cs, ct, cb


class _BeamRequest:
    """_generate_beams for ONE prompt, a step at a time: the state (ids, beam scores, hypotheses) and the scorer (BeamSearchScorer.process / finalize) of row b
    of its batch, for a caller whose prompts are each at their own step (serving.Engine(num_beams > 1)).  Every line is the one _generate_beams runs for
    B = 1 — _BeamHypotheses with the request's length_penalty, EOS candidates beyond rank num_beams skipped, is_done, the stop sequences, the open beams
    becoming hypotheses at max_new_tokens, EOS appended when the best hypothesis ended early — so a request gives the ids of generate() for it alone.
    device: where ids and beam scores live (the logits' device for the torch chain; the CPU when the candidates come from the device kernel, whose
    caller reads nothing else back)."""

    def __init__(self, opts, max_new_tokens, device):
        nb = self.nb = opts.num_beams
        self.o, self.max_new = opts, max_new_tokens
        self.ids = torch.zeros((nb, 0), dtype=torch.long, device=device)
        self.beam_scores = torch.zeros(nb, dtype=torch.float32, device=device)
        self.beam_scores[1:] = -1e9
        self.hyps = _BeamHypotheses(nb, opts.length_penalty)
        self.done = self.finished = False

    def candidates(self, logits):
        """the torch chain of _generate_beams' non-device branch on this request's [num_beams, V] logits rows: CPU (scores, tokens, beams) [2 * num_beams]"""
        o, nb, cur_len = self.o, self.nb, self.ids.shape[1]
        logp = logits.to(self.ids.device).log_softmax(dim=-1)
        logp = _process_logits(logp, self.ids, cur_len, o.repetition_penalty, o.min_length, o.eos_token_id)
        V = logp.shape[-1]
        cand = (logp + self.beam_scores[:, None]).view(1, nb * V)
        cand_scores, cand_tokens = torch.topk(cand, 2 * nb, dim=1, largest=True, sorted=True)
        cand_beams = torch.div(cand_tokens, V, rounding_mode="floor")
        return cand_scores[0].cpu(), (cand_tokens % V)[0].cpu(), cand_beams[0].cpu()

    @staticmethod
    def merge(scores, tokens, nb, V):
        """_device_candidates' merge for one prompt: scores f32 / tokens [nb * k] (beam-major, k = 2 * nb per beam) on the CPU -> the first k of their union
        under (score descending, beam * V + token ascending): (scores, tokens, beams) [k]"""
        k = 2 * nb
        beam = torch.arange(nb).repeat_interleave(k)
        order = sorted(range(nb * k), key=lambda i: (-float(scores[i]), int(beam[i]) * V + int(tokens[i])))[:k]
        return scores[order], tokens[order].long(), beam[order]

    def process(self, cs, ct, cb):
        """BeamSearchScorer.process on the 2 * num_beams merged candidates (CPU tensors), then the stop rules.  Returns (next tokens, beam indices): lists
        of num_beams ints, beam j continues beam index[j] with token[j]; sets `finished`."""
        o, nb, cur_len, dev = self.o, self.nb, self.ids.shape[1], self.ids.device
        eos = o.eos_token_id
        scores, tokens, index = [], [], []
        for rank in range(2 * nb):
            tok, sc, row = int(ct[rank]), float(cs[rank]), int(cb[rank])
            if eos is not None and tok == eos:
                if rank >= nb:
                    continue
                self.hyps.add(self.ids[row].clone(), sc)
            else:
                scores.append(sc); tokens.append(tok); index.append(row)
            if len(tokens) == nb:
                break
        self.done = self.hyps.is_done(float(cs.max()), cur_len)
        self.beam_scores = torch.tensor(scores, dtype=torch.float32, device=dev)
        self.ids = torch.cat([self.ids[torch.tensor(index, device=dev)], torch.tensor(tokens, device=dev).view(-1, 1)], dim=-1)
        if o.stop_sequences and not self.done and bool(_ends_in_stop(self.ids[:1], o.stop_sequences)[0]):
            for j in range(nb):
                self.hyps.add(self.ids[j].clone(), scores[j])
            self.done = True
        self.finished = self.done or _stop(o.stopping_criteria, self.ids, None) or self.ids.shape[1] >= self.max_new
        return tokens, index

    def finalize(self):
        """BeamSearchScorer.finalize: the 1-D LongTensor generate(...)[0] returns for this prompt alone"""
        o = self.o
        if not self.done:
            for j in range(self.nb):
                self.hyps.add(self.ids[j], float(self.beam_scores[j]))
        best = sorted(self.hyps.beams, key=lambda x: x[0])[-1][1]
        sent_max = min(len(best) + 1, self.max_new)
        res = torch.full((sent_max,), o.pad_token_id, dtype=torch.long, device=self.ids.device)
        res[:len(best)] = best
        if len(best) < sent_max:
            res[len(best)] = o.eos_token_id
        return res


def _generate_device(lm_wrapper, inputs_embeds, opts, prefix, lengths):
    """greedy search / sampling of generate(selection="device"): one hip.select_tokens launch per step, the ids stay on the device"""
    from . import hip
    B, dev = inputs_embeds.shape[0], inputs_embeds.device
    max_new_tokens, min_length, do_sample, generator, stopping_criteria = opts.max_new_tokens, opts.min_length, opts.do_sample, opts.generator, opts.stopping_criteria
    eos_token_id, pad_token_id, stop_sequences = opts.eos_token_id, opts.pad_token_id, opts.stop_sequences
    st = _CacheStepper(lm_wrapper, inputs_embeds, opts, prefix, lengths)
    ids = torch.full((B, max_new_tokens), pad_token_id, dtype=torch.int32, device=dev)
    track = eos_token_id is not None or bool(stop_sequences)     # rows can finish: the kernel keeps `unfinished`
    unfinished = torch.ones(B, dtype=torch.int32, device=dev)
    n_gen = torch.zeros(B, dtype=torch.int32, device=dev)
    every = 1 if stopping_criteria is not None else max(1, int(opts.sync_every))
    nxt = torch.empty(B, dtype=torch.int32, device=dev)
    u, t = None, 0
    while True:
        n_gen += unfinished
        if do_sample:
            u = torch.rand(B, generator=generator, device=generator.device if generator is not None else dev).to(dev)
        hip.select_tokens(st.logits, ids[:, t], prev=ids, n_prev=t, penalty=opts.repetition_penalty,
                          suppress_eos=eos_token_id is not None and t < min_length, eos_id=eos_token_id, pad_id=pad_token_id, sample=do_sample,
                          temperature=opts.temperature, top_p=opts.top_p, u=u, unfinished=unfinished if track else None)
        t += 1
        if stop_sequences:
            unfinished *= (~_ends_in_stop(ids[:, :t], stop_sequences)).to(torch.int32)
        if t >= max_new_tokens:
            break
        if stopping_criteria is not None and _stop(stopping_criteria, ids[:, :t].long(), None):
            break
        if track and t % every == 0 and int(unfinished.max()) == 0:
            break
        nxt.copy_(ids[:, t - 1])                                 # the gather's index operand is a dense vector: one 4 * B-byte device copy
        st.advance(nxt, on_device=True)
    n_host = n_gen.tolist()
    n = t if stopping_criteria is not None else max(n_host)      # sync_every > 1 runs past the step at which every row had finished: cut there
    return _finish(ids[:, :n].long(), n_host, opts, _continuation(st, ids, n_host, t) if opts.return_cache else None)
