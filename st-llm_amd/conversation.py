"""Tensor path of the reference's Chat wrapper (stllm/conversation/conversation.py:181-340): what
``demo.py`` drives — ``upload_video`` -> ``encode_img`` -> pooling -> prompt-embedding concat ->
``generate(inputs_embeds=...)``.  The frame transform (resize / crop / normalise, conversation.py:190-198) runs on the
GPU (processors.VideoTransform); video decoding, prompt templates and stopping criteria are
host-side text/media utilities and out of scope."""
import torch

from . import hip
from .models.st_llm import get_residual_index
from .processors import VideoTransform, is_raw_frames


class StoppingCriteriaSub:
    """conversation.py:105-116: stop as soon as the FIRST row ends in one of the stop sequences ('###' has two encodings)."""

    def __init__(self, stops=(), encounters=1):
        self.stops = list(stops)

    def __call__(self, input_ids, scores):
        for stop in self.stops:
            if torch.all((stop.to(input_ids.device) == input_ids[0][-len(stop):])).item():
                return True
        return False


class VideoPrefix:
    """the KV cache of a video's tokens (positions 0 .. n_tokens - 1), reusable across questions (Chat.prefill_video)"""

    def __init__(self, cache, n_tokens):
        self.cache, self.n_tokens = cache, n_tokens


class Dialogue:
    """N conversations in one ragged KV cache, between turns (Chat.answer_many(keep=True), Chat.follow_up).  cache: row b holds the K / V of everything row b
    has seen and said so far except its last generated id, pending[b], which the next turn feeds first (generation.Continuation).  The dialogue lives on
    TOKEN IDS: a follow-up sees exactly the ids the model generated."""

    def __init__(self, cache, pending):
        self.cache, self.pending, self.turns = cache, pending, 1


class Chat:
    def __init__(self, model, device="cuda:0"):
        self.device = device
        self.LLM = model
        # conversation.py:185-190 — the visual front-end hangs off model.model (or model.model.model under peft)
        self.model = model.model.stllm_model if hasattr(model.model, "stllm_model") else model.model.model.stllm_model
        self.transform = VideoTransform(device)   # conversation.py:190-198
        # conversation.py:199-201: '###' ends an answer
        self.stopping_criteria = [StoppingCriteriaSub(stops=[torch.tensor([835]), torch.tensor([2277, 29937])])]

    def upload_video(self, video, conv, img_list, num_frame=64, text=None):
        """conversation.py:274-299.  `video`: decoded raw frames (uint8 RGB [T,H,W,3] / list of PIL images — what the
        reference's load_video returns; transformed on the GPU by processors.VideoTransform == self.transform) or an already
        transformed frames tensor ([T*3,224,224] or [T,3,224,224], CLIP-normalised)."""
        if is_raw_frames(video):
            video = self.transform(video)
        frames = video.to(self.device)
        if frames.dim() == 3:
            bt, w, h = frames.shape
            frames = frames.view(bt // 3, 3, w, h)
        m = self.model
        video_emb, _, _ = m.encode_img(frames, text=text)  # [T,32,4096]
        if m.video_input == "mean":
            video_emb = hip.mean_t(video_emb.unsqueeze(0).contiguous())
        elif m.video_input == "all":
            video_emb = video_emb.reshape(1, -1, video_emb.shape[-1])
        elif m.video_input == "residual":
            video_emb = m.pool_video(video_emb.unsqueeze(0))[:, 0]
        img_list.append(video_emb)
        if conv is not None:
            conv.append_message(conv.roles[0], "<Video><ImageHere></Video>")
        return "Received."

    def get_context_emb_ids(self, img_list, question_ids):
        """conversation.py:322-340 (get_context_emb_sim) on token ids: cat(video_emb, embed([BOS]+question))."""
        tk = self.model.llama_tokenizer
        ids = [[tk.bos_token_id] + list(question_ids)]
        seg = self.model.embed_tokens(torch.tensor(ids))
        mixed = torch.cat((img_list[0], seg), dim=1)
        att = torch.ones(mixed.shape[:-1], dtype=torch.long, device=mixed.device)
        return mixed, att

    def get_context_emb_sim(self, conv, img_list, system=True):
        question = conv.messages[0][1].split("</Video> ")[1]
        question = (conv.system if system else "") + "###Human: " + question + " ###Assistant: "
        return self.get_context_emb_ids(img_list, self.model.llama_tokenizer.encode_ids(question, add_special_tokens=False))

    def prefill_video(self, img_list):
        """Prefill the video tokens img_list[0] ONCE: in the get_context_emb_sim layout they come first (positions 0 .. Nv - 1), so their K / V rows
        do not depend on the question.  Returns a VideoPrefix (the cache in the current compute dtype) for answer(prefix=...).
        With a text-conditioned Q-Former (upload_video(text=question)) the video tokens depend on that text: the prefix is then valid for the question
        it was encoded with only — the caller's responsibility, as img_list already is."""
        emb = img_list[0]
        lm = self.LLM.model
        cache = lm.new_cache(emb.shape[0], emb.shape[1], emb.device)
        lm.prefill(emb, None, cache=cache)
        return VideoPrefix(cache, emb.shape[1])

    def _prompts(self, img_list, questions_ids, keep, prefix):
        """conversation.py:213-253 for every question: its context embeddings [L, D], of which the last `keep` stay.  prefix = prefill_video(img_list)
        and nothing truncated: only [BOS] + question, behind the prefix's cache (a truncated prompt would cut into the cached positions: whole prompts
        then).  Returns (the embeddings per question, that cache | None)."""
        embs = [self.get_context_emb_ids(img_list, q)[0][0] for q in questions_ids]
        if prefix is not None and all(e.shape[0] <= keep for e in embs):
            assert prefix.n_tokens == img_list[0].shape[1] == prefix.cache.len
            return [e[prefix.n_tokens:] for e in embs], prefix.cache
        return [e[max(0, e.shape[0] - keep):] for e in embs], None

    def _decoded(self, tok):
        """conversation.py:246-249: drop a leading <unk> (0), then a leading <s> (1); (text, ids)"""
        for lead in (0, 1):
            if tok.numel() and int(tok[0]) == lead:
                tok = tok[1:]
        return self.model.llama_tokenizer.decode(tok.tolist()), tok.cpu().numpy()

    def answer(self, img_list, question_ids, max_new_tokens=300, num_beams=1, min_length=1, top_p=0.9,
               repetition_penalty=1.0, length_penalty=1, temperature=1.0, max_length=2000, do_sample=False,
               stopping_criteria=None, instruction=False, prefix=None, share_prefix=False, **kw):
        """conversation.py:213-253: keep the last `max_length - max_new_tokens` embeddings, generate with the reference's
        knobs (demo.py: num_beams=5, do_sample=False), drop a leading <unk> (0) / <s> (1) token.  prefix: a prefill_video(img_list) result — the
        video's K / V rows are reused and only [BOS] + question is run (same ids; see prefill_video for the text-conditioned case).  This entry point is the
        `get_context_emb_sim` path (no conv.instruction: video tokens + question), for which the reference OVERRIDES
        repetition_penalty with 1.5 (conversation.py:219-220) whatever the caller passed; instruction=True keeps the argument.
        share_prefix: the beams read one copy of the prompt's (or the video prefix's) K / V rows (generate(share_prefix=True)).
        **kw reaches generate(): selection="device" (and sync_every=K) selects the tokens with the project's own kernels (generation.generate)."""
        if not instruction:
            repetition_penalty = 1.5
        (emb,), cache = self._prompts(img_list, [question_ids], max_length - max_new_tokens, prefix)
        embs = emb[None]
        if cache is not None:
            kw = dict(kw, prefix_cache=cache)
        if stopping_criteria is None:
            stopping_criteria = self.stopping_criteria
        out = self.LLM.generate(inputs_embeds=embs, max_new_tokens=max_new_tokens, stopping_criteria=stopping_criteria,
                                num_beams=num_beams, do_sample=do_sample, min_length=min_length, top_p=top_p,
                                repetition_penalty=repetition_penalty, length_penalty=length_penalty, temperature=temperature,
                                share_prefix=share_prefix, **kw)
        hip.gemm_workspace_check(embs.device, wait=True) if embs.is_cuda else None   # generate() synchronised on every token anyway
        return self._decoded(out[0])

    def answer_many(self, img_list, questions_ids, max_new_tokens=300, num_beams=1, min_length=1, top_p=0.9,
                    repetition_penalty=1.0, length_penalty=1, temperature=1.0, max_length=2000, do_sample=False,
                    stop_sequences=None, instruction=False, prefix=None, share_prefix=False, keep=False, **kw):
        """N questions about ONE video in one ragged batch (generate(batching="ragged")): answer()'s truncation rule and its repetition_penalty = 1.5
        override per question, Chat's stop tokens as per-row stop_sequences (a row that ends in '###' is finished, the others go on).  prefix: a
        prefill_video(img_list) result — the video is prefilled once, forked to the N rows, and only [BOS] + question runs per row.  Returns one
        (text, ids) pair per question, each what answer() returns for that question alone.  share_prefix: the N rows (and their beams) read the prefilled video
        where it is instead of a fork each (generate(share_prefix=True)).  **kw reaches generate(): selection="device", sync_every=K as in answer().
        keep: return (answers, Dialogue) — the rows' KV cache stays alive for follow_up() (num_beams == 1)."""
        if not instruction:
            repetition_penalty = 1.5
        embs, cache = self._prompts(img_list, questions_ids, max_length - max_new_tokens, prefix)
        if cache is not None:
            kw = dict(kw, prefix_cache=cache)
        return self._ragged_round(embs, keep, kw, max_new_tokens=max_new_tokens, stop_sequences=stop_sequences, num_beams=num_beams, do_sample=do_sample,
                                  min_length=min_length, top_p=top_p, repetition_penalty=repetition_penalty, length_penalty=length_penalty,
                                  temperature=temperature, share_prefix=share_prefix)

    def answer_queue(self, img_list, questions_ids, slots=8, max_new_tokens=300, min_length=1, top_p=0.9, repetition_penalty=1.0, temperature=1.0,
                     max_length=2000, do_sample=False, stop_sequences=None, instruction=False, prefix=None, generators=None, share_prefix=False,
                     num_beams=1, length_penalty=1, **kw):
        """N >= 1 questions about ONE video through `slots` KV-cache slots (serving.Engine): a question whose answer ends frees its slot
        for the next one while the others keep decoding, so N may exceed `slots` and no row decodes padding.  answer_many's truncation rule, its
        repetition_penalty = 1.5 override and Chat's stop tokens as per-request stop_sequences.  prefix: a prefill_video(img_list) result — the video's K / V
        rows are copied into a slot on admission and only [BOS] + question runs.  generators: one torch.Generator per question for do_sample.  Returns one
        (text, ids) per question, in order, each what answer() returns for that question alone.  **kw reaches the Engine's options (state="device").
        num_beams > 1 (demo.py decodes with 5): every question searches num_beams beams in its slot, by answer()'s beam rules (do_sample
        raises); length_penalty as in answer().
        share_prefix=True (needs prefix=): the prefix's cache becomes the Engine's base — no slot copies the video's rows, every step reads
        them once for all slots."""
        from . import serving
        if share_prefix and prefix is None:
            raise ValueError("Chat.answer_queue(share_prefix=True) needs prefix=: the prefilled video is what the slots share")
        if not instruction:
            repetition_penalty = 1.5
        embs, cache = self._prompts(img_list, questions_ids, max_length - max_new_tokens, prefix)
        if stop_sequences is None:
            stop_sequences = self.stopping_criteria[0].stops
        P = cache.len if cache is not None else 0
        eng = serving.Engine(self.LLM, min(slots, len(embs)), P + max(e.shape[0] for e in embs) + max_new_tokens, device=embs[0].device,
                             max_new_tokens=max_new_tokens, do_sample=do_sample, min_length=min_length, top_p=top_p, repetition_penalty=repetition_penalty,
                             temperature=temperature, stop_sequences=stop_sequences, num_beams=num_beams, length_penalty=length_penalty,
                             **(dict(kw, base=cache) if share_prefix else kw))
        handles = [eng.submit(e, prefix=cache, generator=None if generators is None else generators[i]) for i, e in enumerate(embs)]
        out = dict(eng.run())
        return [self._decoded(out[h]) for h in handles]

    def _ragged_round(self, embs, keep, kw, *, stop_sequences, **knobs):
        """one generate(batching="ragged") over the right-padded prompts `embs`: (text, ids) per row, and with `keep` the Dialogue to go on from"""
        lens = torch.tensor([e.shape[0] for e in embs])
        batch = torch.nn.utils.rnn.pad_sequence(embs, batch_first=True)
        mask = (torch.arange(int(lens.max()))[None, :] < lens[:, None]).long()
        if stop_sequences is None:
            stop_sequences = self.stopping_criteria[0].stops
        out, n_out, *cont = self.LLM.generate(inputs_embeds=batch, attention_mask=mask, stop_sequences=stop_sequences, batching="ragged",
                                              return_lengths=True, return_cache=keep, **knobs, **kw)
        hip.gemm_workspace_check(batch.device, wait=True) if batch.is_cuda else None
        answers = [self._decoded(row[:n]) for row, n in zip(out, n_out)]
        return (answers, Dialogue(*cont[0])) if keep else answers

    def turn_ids(self, question, closed=True):
        """the ids of a follow-up turn: "Human: " + question + " ###Assistant: " behind a row that ended on '###' (closed), "###Human: ..." behind one
        that ended on EOS or ran out of tokens"""
        text = ("" if closed else "###") + "Human: " + question + " ###Assistant: "
        return self.model.llama_tokenizer.encode_ids(text, add_special_tokens=False)

    def follow_up(self, dialogue, turns_ids, max_new_tokens=300, num_beams=1, min_length=1, top_p=0.9, repetition_penalty=1.0, length_penalty=1, temperature=1.0,
                  do_sample=False, stop_sequences=None, instruction=False, **kw):
        """The next turn of every row of a Dialogue, in ONE ragged batch: row b's prompt is pending[b] + turns_ids[b] (turn_ids()), appended behind the
        row's own cached positions (generate(prefix_cache=dialogue.cache, batching="ragged"): LlamaModel.extend on a ragged cache) — neither the video nor
        the history is prefilled again.  Returns what answer_many returns and updates the dialogue.  The knobs are answer_many's (beams raise: generate(return_cache=True)).
        The dialogue lives on TOKEN IDS: the follow-up sees exactly the ids the model generated.  The reference re-tokenises the decoded text of the whole
        conversation on every turn (conversation.py:301-320), which need not give the same ids; what this equals is a from-scratch prefill of the
        concatenated id sequence [video, turn 1, answer 1, turn 2, ...] of every row.
        A turn that does not fit the cache gets a larger one (the working cache of every turn is a fork); past the model's position limit it is a ValueError."""
        from .models.llama import cfg_max_len
        if not instruction:
            repetition_penalty = 1.5
        cache = dialogue.cache
        assert len(turns_ids) == cache.batch
        ids = [[int(p)] + list(t) for p, t in zip(dialogue.pending.tolist(), turns_ids)]
        have = cache.lens if cache.lens is not None else [cache.len] * cache.batch
        limit = cfg_max_len(self.LLM.model.config)
        need = max(h + len(i) for h, i in zip(have, ids)) + max_new_tokens
        if need > limit:
            raise ValueError(f"Chat.follow_up: the next turn needs {need} positions (history + turn + max_new_tokens), past the model's limit of {limit} "
                             "(max_position_embeddings)")
        embs = [self.model.embed_tokens(torch.tensor([i]))[0] for i in ids]
        answers, nxt = self._ragged_round(embs, True, dict(kw, prefix_cache=cache), max_new_tokens=max_new_tokens, stop_sequences=stop_sequences,
                                          num_beams=num_beams, do_sample=do_sample, min_length=min_length, top_p=top_p, repetition_penalty=repetition_penalty,
                                          length_penalty=length_penalty, temperature=temperature)
        dialogue.cache, dialogue.pending, dialogue.turns = nxt.cache, nxt.pending, dialogue.turns + 1
        return answers
