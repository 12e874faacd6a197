"""CPU: serving.Engine(state="device") on the contract backend, fp32, the SMALL model and the vetted prompts of tests/test_segments_cpu.py,
with tests/_select_slots_ref.select_slots in place of the kernel: every request's ids equal generate() of that request alone and the host-state Engine
(greedy, with and without a prefix, an EOS mid-way, stop sequences; sampling against generate(selection="device") with the same seed); a step is one
select_slots launch and one read of the state table; what the mode does not serve raises; Chat.answer_queue(state="device")."""
import contextlib
import sys

import numpy as np
import pytest
import torch

import _cpu_backend as CB
import _poison
import _segments_case as SC
import _select_ref as R
import _select_slots_ref as SR
from _util import T, small_llama
from test_segments_cpu import VIDEO, _requests, stllm  # noqa: F401  (stllm: the chat fixture)

torch.set_grad_enabled(False)
SMALL = SC.SMALL


@contextlib.contextmanager
def _backend():
    from stllm_amd import runtime
    with SC.installed(), CB._patched({"select_slots": SR.select_slots, "select_tokens": R.select_tokens}), runtime.use_dtype("fp32"):
        yield


@contextlib.contextmanager
def _recording():
    """every hip.select_slots call of the block: its keyword arguments, and its name in CB.CALLS (next to what SC.counting() records)"""
    from stllm_amd import hip
    seen, inner = [], hip.select_slots

    def f(*a, **k):
        CB.CALLS.append("select_slots")
        seen.append(k)
        return inner(*a, **k)
    with CB._patched({"select_slots": f}):
        yield seen


@pytest.mark.parametrize("with_prefix", [False, True])
def test_device_state_gives_the_ids_of_generate_alone_and_of_the_host_engine(with_prefix):
    """5 requests of different prompt lengths and max_new_tokens over 2 slots, greedy, with the EOS id that request 1 emits mid-way; then the same with a
    stop sequence cut from a free run"""
    model = small_llama(SMALL, lm_head_spread=6.0)
    lm = model.model
    prompts = _requests()
    video = T(VIDEO[0], (VIDEO[1], 256), 0.05) if with_prefix else None
    k = dict(do_sample=False, min_length=0)
    with _backend():
        free = SC.alone(model, prompts, video, eos_token_id=None, **k)
        prefix = None
        if with_prefix:
            prefix = lm.new_cache(1, VIDEO[1], "cpu")
            lm.prefill(video[None], None, cache=prefix)
            before = [x.clone() for x in prefix.qkv]
        stop = [free[0][2:4].clone(), free[3][1:2].clone()]     # two ids of request 0's free run, one of request 3's
        for extra in (dict(eos_token_id=int(free[1][1])), dict(eos_token_id=None, stop_sequences=stop)):
            kk = dict(k, **extra)
            with SC.scored_runs() as scored:
                want = SC.alone(model, prompts, video, **kk)
            assert min(scored) >= SC.MARGIN, ("precondition: the from-scratch runs are not near a tie", min(scored))
            assert any(w.numel() < n for w, n in zip(want, SC.REQ_MAX_NEW)) and any(w.numel() == n for w, n in zip(want, SC.REQ_MAX_NEW)), "one ends early, one runs to its limit"
            host, _ = SC.serve(model, prompts, 2, 40, prefix=prefix, **kk)
            got, eng = SC.serve(model, prompts, 2, 40, prefix=prefix, state="device", **kk)
            for i, (g, h, w) in enumerate(zip(got, host, want)):
                assert g.dtype == torch.long and g.dim() == 1
                assert g.tolist() == w.tolist() and g.tolist() == h.tolist(), (extra, i, g.tolist(), h.tolist(), w.tolist())
            assert eng.steps["segments"] >= 3 and eng.steps["decode"] >= 1, eng.steps
        assert all(w.tolist() == f[:w.numel()].tolist() for w, f in zip(want, free)) and want[0].numel() < free[0].numel() and want[3].numel() == 2, \
            "the stop sequences cut the free runs"
        if with_prefix:
            assert prefix.len == VIDEO[1] and all(_poison.bits_equal(x, y) for x, y in zip(prefix.qkv, before)), "the prefix is only read"


def test_device_state_sampling_equals_generate_device_of_every_request_alone():
    """do_sample with one generator per request: the ids of generate(selection="device", generator=same seed) for that request alone — one torch.rand(1)
    per served request and step is the stream that path consumes"""
    from stllm_amd import serving
    model = small_llama(SMALL, lm_head_spread=6.0)
    prompts = _requests()
    k = dict(do_sample=True, top_p=0.9, temperature=0.8, min_length=1, eos_token_id=None, max_new_tokens=5, repetition_penalty=1.5)
    with _backend():
        want = [model.generate(inputs_embeds=p[None], generator=torch.Generator().manual_seed(7 + i), selection="device", **k)[0] for i, p in enumerate(prompts[:3])]
        eng = serving.Engine(model, 2, 40, state="device", **k)
        hs = [eng.submit(p, generator=torch.Generator().manual_seed(7 + i)) for i, p in enumerate(prompts[:3])]
        with _recording() as seen:
            got = dict(eng.run())
        assert all(kw["sample"] and kw["u"] is not None for kw in seen)
        for h, w in zip(hs, want):
            assert got[h].tolist() == w.tolist()
        assert len({tuple(w.tolist()) for w in want}) > 1


def _count_reads(monkeypatch):
    """Tensor.item / tolist / __int__ called from serving.py: (method, calling function) per call.  On the device each of them is a blocking transfer."""
    reads = []

    def counted(name, orig):
        def f(self, *a, **k):
            fr = sys._getframe(1)
            if fr.f_code.co_filename.replace("\\", "/").endswith("/serving.py"):
                reads.append((name, fr.f_code.co_name))
            return orig(self, *a, **k)
        return f
    for name in ("item", "tolist", "__int__"):
        monkeypatch.setattr(torch.Tensor, name, counted(name, getattr(torch.Tensor, name)))
    return reads


def test_a_step_is_one_select_slots_launch_and_one_read(monkeypatch):
    from stllm_amd import serving
    model = small_llama(SMALL, lm_head_spread=6.0)
    prompts = _requests()
    with _backend():
        eng = serving.Engine(model, 3, 40, state="device", do_sample=False, min_length=1, eos_token_id=None, max_new_tokens=4, repetition_penalty=1.5)
        host = serving.Engine(model, 3, 40, do_sample=False, min_length=1, eos_token_id=None, max_new_tokens=4, repetition_penalty=1.5)
        for e in (eng, host):
            e.submit(prompts[0])
            e.submit(prompts[1])
        reads = _count_reads(monkeypatch)
        table_reads = []
        monkeypatch.setattr(serving.Engine, "_read_state", (lambda f: lambda self: (table_reads.append(1), f(self))[1])(serving.Engine._read_state))
        for kind, n_of_kind in (("segments", 1), ("decode", 1), ("segments", 2)):   # two admissions; a pure decode step; an admission next to two running requests
            if n_of_kind == 2:
                eng.submit(prompts[2])
                host.submit(prompts[2])
            del reads[:], table_reads[:]
            with SC.counting() as calls, _recording() as seen:
                assert eng.step() == []
                assert calls.count("select_slots") == 1 and len(seen) == 1, calls
            assert eng.steps[kind] == n_of_kind, eng.steps
            assert reads == [("tolist", "_read_state")] and table_reads == [1], (kind, reads)
            n_running = len(eng.running)
            del reads[:]
            assert host.step() == []
            assert len(reads) >= n_running and all(fn == "_select" for _, fn in reads), (kind, reads)   # today's path: a blocking read per request
        assert eng.cache.row_lens() == host.cache.row_lens()
        a, b = dict(eng.run()), dict(host.run())
        assert sorted(a) == sorted(b) and all(a[h].tolist() == b[h].tolist() for h in a)


def test_what_device_state_does_not_serve_raises():
    from stllm_amd import serving
    model = small_llama(SMALL, lm_head_spread=6.0)

    class Never:
        def __call__(self, ids, scores):
            return False
    with _backend():
        for bad in (dict(stopping_criteria=[Never()]), dict(sync_every=4), dict(selection="device"), dict(num_beams=2)):
            with pytest.raises(NotImplementedError):
                serving.Engine(model, 2, 40, state="device", **bad)
        with pytest.raises(NotImplementedError, match="state='device'"):
            serving.Engine(model, 2, 40, selection="device")
        with pytest.raises(ValueError):
            serving.Engine(model, 2, 40, state="gpu")
        serving.Engine(model, 2, 40, stopping_criteria=[Never()])    # the host state serves criteria as before
        eng = serving.Engine(model, 2, 40, state="device", max_new_tokens=3, eos_token_id=None)
        h = eng.submit(_requests()[0], max_new_tokens=7)              # a longer budget than the table was sized for: it is widened
        assert dict(eng.run())[h].numel() == 7 and eng.cache.row_lens() == [0, 0]


@pytest.mark.parametrize("with_prefix", [True, False])
def test_chat_answer_queue_device_state_equals_answer_queue(stllm, with_prefix):  # noqa: F811
    """three questions over two slots: (text, ids) of Chat.answer_queue per question (which equals Chat.answer: tests/test_segments_cpu.py); Chat's default
    stop sequences reach the kernel's stop table"""
    from stllm_amd.conversation import Chat
    import _ragged_extend_case as RC
    frames = T("input.frames2", (2, 3, 224, 224))
    questions = RC.CHAT_QUESTIONS
    k = dict(max_new_tokens=4)
    with _backend():
        chat = Chat(stllm, device="cpu")
        img_list = []
        chat.upload_video(frames.view(6, 224, 224), None, img_list)
        prefix = chat.prefill_video(img_list) if with_prefix else None
        want = chat.answer_queue(img_list, questions, slots=2, prefix=prefix, **k)
        with _recording() as seen:
            got = chat.answer_queue(img_list, questions, slots=2, prefix=prefix, state="device", **k)
        n_stops = len([s for s in chat.stopping_criteria[0].stops if s.numel()])
        assert seen and all(kw["stops"] is not None and kw["stops"].shape[0] == n_stops and kw["stop_len"].numel() == n_stops for kw in seen)
        assert len(got) == 3
        for (t0, i0), (t1, i1) in zip(want, got):
            assert np.array_equal(i0, i1) and t0 == t1
