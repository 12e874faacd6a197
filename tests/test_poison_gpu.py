"""GPU: poisoned-allocation runs (tests/_poison.py) of the product path on the HIP kernels.  Every path runs twice clean (A, B) and once with every
torch.empty / empty_like / empty_strided / new_empty result — KV-cache buffers, attention and key-split workspaces, norm-backward scratch, dense staging
rows, LoRA row buffers, outputs — every hand-out of hip.split_workspace and every truncated cache row filled with 0xFF (P): NaN wherever a kernel or the
host reads what nobody wrote.  On the DEFINED outputs: A == B bit for bit (run-to-run determinism), P == A bit for bit, P finite, poison count > 0
(tests/_poison.py: compare).  The smallest models of the GPU suite: build_stllm at (vit_depth 1, qf_layers 2, llm_layers 2) and the 2-layer full-width
Llama of tests/test_ragged_gpu.py; prompts of 12 - 40 positions, 4 - 6 new tokens.  The host-code twin on the CPU contract backends: test_poison_cpu.py."""
import contextlib

import numpy as np
import pytest
import torch

from _poison import compare, poisoned_allocations
from _util import T
from test_poison_cpu import GEN, LENS, _gen_cases, _live, _mask, _steps, abp

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

BASE = dict(vit_model="eva_clip_g", image_size=224, num_query_token=32, max_txt_len=32, end_sym=" 2")
CFG_TEXT = dict(BASE, video_input="residual", residual_size=2, use_mask=False, mvm_decode=False, qformer_text_input=True)
CFG_MVM = dict(BASE, video_input="all", use_mask=True, mvm_decode=True, qformer_text_input=False)
CFG_MEAN = dict(BASE, video_input="mean", use_mask=False, mvm_decode=False, qformer_text_input=False)
CFG_NOQF = dict(CFG_MEAN, has_qformer=False)
CFG_PRE = dict(BASE, video_input="all", use_mask=False, mvm_decode=False, qformer_text_input=False, pre_encoding=True)
CFG_BT = dict(BASE, vit_model="eva_btadapter_g", video_input="all", use_mask=True, mvm_decode=True, qformer_text_input=True)


def _stllm(cfg, depths=(1, 2, 2)):
    from test_model_gpu import build_stllm
    return build_stllm(cfg, vit_depth=depths[0], qf_layers=depths[1], llm_layers=depths[2])


def _inputs(B, Tn, text, image=None):
    from test_host_orchestration_cpu import make_inputs
    samples, _ = make_inputs(B, Tn, text)            # ragged instruction / answer / Q-Former text rows
    samples["image"] = (samples["image"] if image is None else image).cuda()
    return samples


def _forward_run(model, samples, seed=None):
    """model(samples): the logits at the unmasked positions and the loss.  seed: the dynamic mask is drawn from numpy's global generator"""
    am = {}

    def run():
        if seed is not None:
            np.random.seed(seed)
        if "mask" not in am:
            am["mask"] = model.model.stllm_model(samples)[1].bool()      # input-determined: which positions are tokens
            if seed is not None:
                np.random.seed(seed)
        out = model(samples=samples)
        torch.cuda.synchronize()
        res = dict(logits=out.logits[am["mask"]].clone(), loss=out.loss.clone())
        if getattr(out, "loss_mvm", None) is not None:
            res["loss_mvm"] = out.loss_mvm.clone()
        return res
    return run


def _ok():
    from stllm_amd import hip
    assert hip.gemm_workspace_ok()


# ---- forward ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "fp16", "fp32"])
def test_forward_text_qformer_with_ragged_text_rows(mode):
    from stllm_amd import runtime
    model = _stllm(CFG_TEXT)
    samples = _inputs(2, 4, True)
    with runtime.use_dtype(mode):
        abp(_forward_run(model, samples), f"forward, text Q-Former, ragged text rows, {mode}")
    _ok()


@pytest.mark.parametrize("name", ["dynamic mask + MVM, T = 2", "no Q-Former", "pre-encoded features", "BT-Adapter (4, 2, 1)"])
def test_forward_other_graphs(name):
    from stllm_amd import runtime
    seed = None
    if name.startswith("dynamic"):
        model, samples, seed = _stllm(CFG_MVM), _inputs(2, 2, False), 13          # no samples["mask"]: drawn per call (the c4 graph at T = 2)
    elif name.startswith("no Q"):
        model, samples = _stllm(CFG_NOQF), _inputs(2, 2, False)
    elif name.startswith("pre"):
        model, samples = _stllm(CFG_PRE), _inputs(2, 3, False, image=T("input.features", (2, 3, 32, 768), 0.5))
    else:
        model, samples, seed = _stllm(CFG_BT, (4, 2, 1)), _inputs(2, 4, True), 13
    with runtime.use_dtype("bf16"):
        abp(_forward_run(model, samples, seed), f"forward, {name}, bf16")
    _ok()


@pytest.mark.parametrize("mode", ["bf16x3", "mixed"])
def test_forward_split_modes_exercise_the_split_workspace(mode):
    from stllm_amd import runtime
    model = _stllm(CFG_MEAN)
    samples = _inputs(2, 2, False)
    with runtime.use_dtype(mode):
        counts = abp(_forward_run(model, samples), f"forward, {mode}")
    assert counts.refills > 0, "hip.split_workspace: re-filled at every hand-out"
    _ok()


def test_two_steps_in_flight_on_two_streams():
    from stllm_amd import runtime
    model = _stllm(CFG_MEAN)
    sa = _inputs(2, 2, False)
    sb = dict(sa, image=T("input.video_b", (2, 2, 3, 224, 224)).cuda())
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()

    def run():
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            oa = model(samples=sa)
        with torch.cuda.stream(s2):
            ob = model(samples=sb)
        torch.cuda.synchronize()
        return dict(a=(oa.logits.clone(), oa.loss.clone()), b=(ob.logits.clone(), ob.loss.clone()))
    with runtime.use_dtype("bf16"):
        am = model.model.stllm_model(sa)[1].bool()
        a, b = run(), run()
        with poisoned_allocations() as counts:
            p = run()
        pick = lambda r: {k: (v[0][am], v[1]) for k, v in r.items()}
        compare(pick(a), pick(b), pick(p), counts, "two steps in flight on two streams")
    _ok()


# ---- the language model: prefill / extend / decode_step / generate -----------------------------------------------------------------------------------
def _llm(r=0):
    from test_ragged_gpu import _model
    m = _model(2, r=r)
    m.lm_head.weight.mul_(6.0)     # as tests/test_model_gpu.py::test_generate_padded_batch_on_device: the rows take different paths
    return m


@pytest.fixture(scope="module")
def llm():
    return _llm()


@pytest.fixture(scope="module")
def llm_lora():
    return _llm(r=8)


def EMB():
    return T("poison.emb4096", (4, 40, 4096), 0.05).cuda()


@contextlib.contextmanager
def _modes(dt, weights=None):
    from stllm_amd import runtime
    with contextlib.ExitStack() as st:
        st.enter_context(runtime.use_dtype(dt))
        if weights:
            st.enter_context(runtime.use_decode_weights(weights))
        yield


def _sync(x):
    torch.cuda.synchronize()
    return x


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("kind", ["uniform", "ragged, one restarted row", "shared base"])
def test_prefill_then_four_decode_steps(llm, mode, kind):
    """prefill of right-padded rows into a cache, then 4 decode_steps: the logits of every step, K and V of every cache row below its length"""
    emb, lm = EMB(), llm.model

    def run():
        if kind == "uniform":
            c = lm.new_cache(2, 24, "cuda")
            lm.prefill(emb[:2, :17], None, cache=c)
            return _sync(dict(logits=_steps(llm, c, emb[:2, 17:21]), cache=_live(c)))
        lens = [17, 12, 17, 13]
        c = lm.new_cache(4, 24, "cuda")
        h32, _ = lm.prefill(emb[:, :17] * _mask(lens, 17)[:, :, None].cuda(), _mask(lens, 17), cache=c)
        hidden = [h32[b, :n].clone() for b, n in enumerate(lens)]
        if kind == "shared base":
            base = lm.new_cache(1, 13, "cuda")
            lm.prefill(emb[:1, :13], None, cache=base)
            s = base.share(rows=4, max_new=5 + 4)
            sfx = [5, 1, 5, 3]
            _, hs = lm.extend(emb[:, 13:18], s, lengths=sfx)
            ext = [hs.view(4, 5, -1)[b, :n].clone() for b, n in enumerate(sfx)]
            return _sync(dict(hidden=hidden, extend=ext, logits=_steps(llm, s, emb[:, 20:24]), cache=_live(s), base=_live(base)))
        c.truncate([17, 0, 17, 13])                                     # row 1: a freed slot that starts over at position 0 — the 12 rows it held are
        return _sync(dict(hidden=hidden, logits=_steps(llm, c, emb[:, 17:21]), cache=_live(c)))   # undefined again (poisoned by the truncation)
    with _modes(mode):
        abp(run, f"prefill + 4 decode steps, {kind}, {mode}")
    _ok()


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_extend_behind_a_prefix(llm, mode, monkeypatch):
    """stack entry, per-op body, lengths=, shared base: the hidden rows of the live positions and the live cache rows"""
    from stllm_amd.models import llama
    emb, lm = EMB(), llm.model

    def run():
        out = {}
        for entry in (True, False):
            monkeypatch.setattr(llama, "STACK_ENTRY", entry)
            c = lm.new_cache(2, 40, "cuda")
            lm.prefill(emb[:2, :19], None, cache=c)
            h32, _ = lm.extend(emb[:2, 19:32], c)
            out[f"uniform, stack entry {entry}"] = (h32.clone(), _live(c))
        monkeypatch.setattr(llama, "STACK_ENTRY", True)
        sfx = [13, 2, 9, 1]
        c = lm.new_cache(4, 40, "cuda")
        lm.prefill(emb[:, :19], None, cache=c)
        h32, _ = lm.extend(emb[:, 19:32], c, lengths=sfx)
        out["lengths"] = ([h32[b, :n].clone() for b, n in enumerate(sfx)], _live(c), _steps(llm, c, emb[:, 32:34]))
        base = lm.new_cache(2, 19, "cuda")
        lm.prefill(emb[:2, :19], None, cache=base)
        s = base.share(rows=4, max_new=16)
        h32, _ = lm.extend(emb[:, 19:32], s, lengths=sfx)
        out["shared"] = ([h32[b, :n].clone() for b, n in enumerate(sfx)], _live(s), _live(base))
        return _sync(out)
    with _modes(mode):
        abp(run, f"extend behind a prefix, {mode}")
    _ok()


def _gen_run(model, emb, only=None, sample=False):
    def run():
        cases, prefix = _gen_cases(model, emb)
        out = {k: model.generate(**kw, **GEN) for k, kw in cases.items() if only is None or k in only}
        if sample:
            out["top-p"] = model.generate(inputs_embeds=emb[:2, :12], max_new_tokens=5, do_sample=True, top_p=0.9, min_length=1,
                                          generator=torch.Generator(device="cuda").manual_seed(7))
        out["prefix"] = [b[:, :7, b.shape[-1] // 3:].clone() for b in prefix.qkv]
        return _sync(out)
    return run


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_generate(llm, mode):
    """greedy, top-p with a seeded generator, 5 beams, a padded batch by groups, batching="ragged", prefix_cache=, share_prefix=True: the ids"""
    with _modes(mode):
        abp(_gen_run(llm, EMB(), sample=True), f"generate, {mode}")
    _ok()


@pytest.mark.parametrize("weights", ["int8", "int4g128"])
def test_generate_on_quantised_decode_weights(llm, weights):
    with _modes("bf16", weights):
        abp(_gen_run(llm, EMB(), sample=True), f"generate, {weights}")
    _ok()


def test_generate_with_active_lora_adapters(llm_lora):
    emb, lm = EMB(), llm_lora.model

    def run():
        c = lm.new_cache(2, 40, "cuda")
        h32, _ = lm.prefill(emb[:2, :19], None, cache=c)
        e32, _ = lm.extend(emb[:2, 19:25], c)
        out = dict(prefill=h32.clone(), extend=e32.clone(), steps=_steps(llm_lora, c, emb[:2, 25:29]), cache=_live(c))
        out.update(_gen_run(llm_lora, emb, only=("greedy", "5 beams", "groups", "ragged", "prefix_cache", "share_prefix, ragged questions"))())
        return out
    with _modes("bf16"):
        abp(run, "active LoRA adapters, bf16")
    _ok()


def test_chat_prefill_video_and_answer_many_share_prefix():
    from stllm_amd import runtime
    from stllm_amd.conversation import Chat
    model = _stllm(CFG_MEAN)
    model.lm_head.weight.mul_(6.0)
    frames = T("input.frames2", (2, 3, 224, 224)).view(6, 224, 224).cuda()
    questions = [[21, 22, 23], [400, 17, 9000, 5, 77], [9]]

    def run():
        chat = Chat(model, device="cuda")
        img_list = []
        chat.upload_video(frames, None, img_list)
        prefix = chat.prefill_video(img_list)
        got = chat.answer_many(img_list, questions, prefix=prefix, share_prefix=True, max_new_tokens=6, do_sample=False, num_beams=1)
        beams = chat.answer_many(img_list, questions, prefix=prefix, share_prefix=True, max_new_tokens=4, do_sample=False, num_beams=3)
        torch.cuda.synchronize()
        return dict(video=img_list[0].clone(), ids=[torch.from_numpy(i.copy()) for _, i in got], beams=[torch.from_numpy(i.copy()) for _, i in beams],
                    prefix=_live(prefix.cache))
    with runtime.use_dtype("bf16"):
        abp(run, "Chat.prefill_video + answer_many(share_prefix=True), bf16")
    _ok()


# ---- training --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_train_step(mode):
    """training.train_step on the `mvm` case of tests/test_backward_cpu.py.
    Bit-exact (A == B == P): the loss, the MVM loss and EVERY gradient — the optimizer's flat gradient buffer holds all of them after the step.
    NOT run-to-run deterministic (measured on an MI355X: A != B, first at the gradient norm; profiles/poisoned_allocations.md): the gradient norm, and
    through the clipping factor max_grad_norm / norm the masters and both AdamW moments.  Cause, by reading: sumsq_kernel (csrc/train_ops.hip) adds one
    partial sum per workgroup into a single float with atomicAdd, in the order the workgroups retire.  For these four outputs only, P is compared with A
    at the bounds of the accuracy tests of the same quantities — tests/test_optimizer_cpu.py::test_adamw_matches_torch: `abs(got_norm - want_norm) <=
    1e-5 * want_norm` and `torch.allclose(p, rp, rtol=2e-6, atol=2e-7)` for the masters; tests/test_kernels_emulated_cpu.py::test_adamw_and_sumsq (run on
    the device by tests/test_train_gpu.py): 2e-6 of the tensor's abs-max for m and v — and must be finite."""
    import test_backward_cpu as TB
    from _poison import assert_finite, bits_equal
    from stllm_amd import runtime, training
    g = TB.golden("backward")
    cfg, Tn = TB.CASES["mvm"]
    model = _stllm(dict(cfg, image_size=224, num_query_token=32, max_txt_len=32, end_sym=" 2"))
    instr, answers = TB.product_samples(g, "mvm", False)
    samples = {"image": T("input.video", (2, Tn, 3, 224, 224)).cuda(), "instruction_input": instr, "answer": answers, "mask": torch.from_numpy(g["mvm.mask"])}
    start = {k: v.detach().clone() for k, v in model.state_dict().items()}

    def run():
        model.load_state_dict(start)            # in place: the step before moved the masters; loading drops every packed copy
        opt = training.AdamW(list(training.trainable_parameters(model)), lr=1e-3, max_grad_norm=1.0)
        loss, loss_mvm, norm = training.train_step(model, samples, opt)
        torch.cuda.synchronize()
        exact = dict(loss=loss.clone(), loss_mvm=loss_mvm.clone(), grads=opt.gflat.clone())
        return exact, dict(norm=float(norm), masters=opt.flat.clone(), m=opt.m.clone(), v=opt.v.clone())
    with runtime.use_dtype(mode):
        (a, sa), (b, sb) = run(), run()
        with poisoned_allocations() as counts:
            p, sp = run()
    print(f"training.train_step, mvm, {mode}: {counts}; norm / masters / m / v: A == B {bits_equal(sa, sb)}, P == A {bits_equal(sp, sa)} "
          f"(norm A {sa['norm']!r} B {sb['norm']!r} P {sp['norm']!r})")
    compare(a, b, p, counts, f"training.train_step, mvm, {mode}: loss, gradients")
    assert_finite(sp, "P")
    assert abs(sp["norm"] - sa["norm"]) <= 1e-5 * sa["norm"]
    assert torch.allclose(sp["masters"], sa["masters"], rtol=2e-6, atol=2e-7)
    for k in ("m", "v"):
        err, scale = float((sp[k] - sa[k]).abs().max()), float(sa[k].abs().max())
        assert err <= 2e-6 * scale, (k, err, scale)
    _ok()
