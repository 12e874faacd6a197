"""GPU (-m gpu): LoRA adapters on the Llama q/v projections — the down-projection kernel, the K-extended QKV GEMM inside the prefill
(stack entry and per-op path), decode with the KV cache, merge / unmerge on the device.

peft is not available, so there is no reference fixture for this branch: every parity check feeds `W + s·B·A` (computed in fp64) as a
plain q_proj / v_proj weight to the reference-pinned CPU oracle (oracle/stllm_oracle.py).  Adapters carry NON-ZERO B (peft's zero
init would pass on a build that ignores them), and every parity check first asserts on the oracle alone that the adapters move the
compared tensor by >= 10x the tolerance it is about to use.  Tolerances: MODES of tests/test_model_gpu.py.
Each check runs in a child process with its own timeout (house style of tests/test_train_gpu.py): a fault ends that check only."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _child(args, timeout):
    r = subprocess.run([sys.executable] + args, cwd=ROOT, env=dict(os.environ), capture_output=True, text=True, timeout=timeout)
    tail = (r.stdout[-3000:] + "\n" + r.stderr[-3000:])
    assert r.returncode == 0, f"child exited with {r.returncode}:\n{tail}"
    return r.stdout


_COMMON = r'''
import sys
sys.path[:0] = ["tests", "oracle", "."]
import numpy as np, torch
torch.set_grad_enabled(False)
import stllm_oracle as O
from _util import T
from stllm_amd import hip, runtime, synth
from stllm_amd.models import llama as llama_mod
from stllm_amd.models.st_llm import STLLMForCausalLM, StllmConfig
MODES = [("fp32", 2e-4), ("fp16", 1e-2), ("bf16", 5e-2)]   # tests/test_model_gpu.py

def build(n_layers, r, alpha=32, b_std=0.0):
    m = STLLMForCausalLM(StllmConfig(num_hidden_layers=n_layers), device="cuda")
    synth.fill_module_(m, 0, "")
    m.add_lora(r, alpha)
    set_b(m, b_std)
    return m

def set_b(m, b_std):
    for i, mod in enumerate(m._lora_modules()):
        mod.B.copy_(T(f"lora.B{i}", tuple(mod.B.shape), b_std).cuda())

def merged_sd(m):
    """HF-named state dict on the CPU with q_proj / v_proj = W + s B A in fp64 (the oracle's input), and the same with the base weights"""
    base, mg = {}, {}
    for k, v in m.state_dict().items():
        if "lora_" in k:
            continue
        k2 = k.replace(".base_layer.", ".")
        base[k2] = mg[k2] = v.detach().float().cpu()
    for li, l in enumerate(m.model.layers):
        for t in ("q_proj", "v_proj"):
            mod = getattr(l.self_attn, t)
            w = mod.base_layer.weight.detach().double().cpu() + mod.scaling * (mod.B.detach().double().cpu() @ mod.A.detach().double().cpu())
            mg[f"model.layers.{li}.self_attn.{t}.weight"] = w
    return base, mg

def oracle_logits(emb, mask, sd):
    sd = {k: v.float() for k, v in sd.items()}
    h = O.llama_forward(emb, mask, sd)
    return h, O.lm_logits(h, sd)

def pick_b(m, emb, mask, tol, valid=None):
    """B's scale such that the adapters move the oracle's logits by >= 10 tol abs-max (the guard that fails on a build ignoring them)"""
    for b_std in (0.02, 0.05, 0.12, 0.3):
        set_b(m, b_std)
        base, mg = merged_sd(m)
        hb, lb = oracle_logits(emb, mask, base)
        hm, lm_ = oracle_logits(emb, mask, mg)
        v = slice(None) if valid is None else valid
        ok = all(float((a[v] - b[v]).abs().max()) >= 10 * tol * float(a[v].abs().max()) for a, b in ((hm, hb), (lm_, lb)))
        print("pick_b", b_std, float((lm_[v] - lb[v]).abs().max()), float(lm_[v].abs().max()), ok, flush=True)
        if ok:
            return hm, lm_
    raise AssertionError("no B scale moves the oracle's output by 10x the tolerance")
'''

_KERNEL = _COMMON + r'''
# tighter than MODES (2e-4 / 1e-2 / 5e-2), which a single kernel against its own rounded inputs must beat by far: bounds from the number formats.
# (stllm_lora_down offers no 2-level row indexing — its callers hold flat rows — so there is no such case.)
eps_out = {"fp32": 1e-5, "fp16": 2.0 ** -10 + 1e-5, "bf16": 2.0 ** -7 + 1e-5}   # one rounding of the output (2 ulp_half) + fp32 accumulation over K = 4096
K = 4096
for mode in ("fp32", "fp16", "bf16"):
    dt = hip.torch_dtype(mode)
    for r in (8, 16, 64):
        P = hip.lora_pad(r, dt)
        A = T(f"k.A{r}", (2 * r, K), 0.02).cuda().to(dt)
        for M in (1, 5, 16, 576, 1088, 2304):
            buf = torch.full((M, K + P), float("nan"), device="cuda", dtype=dt)     # x and t in ONE row buffer, as the model holds them
            buf[:, :K] = T(f"k.x{M}", (M, K), 1.0).cuda().to(dt)
            hip.lora_down(buf[:, :K], A, dtype=dt, out=buf[:, K:])
            t1 = buf[:, K:].clone()
            hip.lora_down(buf[:, :K], A, dtype=dt, out=buf[:, K:])
            t2 = buf[:, K:].clone()
            assert torch.equal(t1, t2), (mode, r, M, "two calls differ")
            assert bool((t1[:, 2 * r:] == 0).all()), (mode, r, M, "pad columns")
            want = buf[:, :K].double() @ A.double().t()
            err = float((t1[:, :2 * r].double() - want).abs().max()) / float(want.abs().max())
            assert err <= eps_out[mode], (mode, r, M, err)
            out2 = torch.empty((M, P), device="cuda", dtype=dt)                      # separate, dense output: same bits
            hip.lora_down(buf[:, :K], A, dtype=dt, out=out2)
            assert torch.equal(out2, t1), (mode, r, M, "dense output differs")
        print("ok", mode, r, flush=True)
'''

_FORWARD = _COMMON + r'''
case = sys.argv[1]
B, S = (1, 576) if case == "s576" else (2, 131)
m = build(2, 16)
emb = T("input.inputs_embeds", (B, S, 4096), 0.05)
mask = None
valid = None
if case == "padded":
    mask = torch.ones(B, S, dtype=torch.long)
    mask[1, 97:] = 0
    valid = mask.bool()
h_ref, l_ref = pick_b(m, emb, mask, 5e-2, valid)
v = slice(None) if valid is None else valid
for mode, tol in MODES:
    with runtime.use_dtype(mode):
        out = m(samples=None, inputs_embeds=emb.cuda(), attention_mask=None if mask is None else hip.with_host(mask, "cuda"), output_hidden_states=True)
    h, lg = out.hidden_states[-1].float().cpu(), out.logits.float().cpu()
    for name, got, want in (("hidden", h, h_ref), ("logits", lg, l_ref)):
        assert torch.isfinite(got[v]).all(), (mode, name)
        err = float((got[v] - want[v]).abs().max()) / float(want[v].abs().max())
        print(case, mode, name, "rel err", err, "tol", tol, flush=True)
        assert err <= tol, (case, mode, name, err)
    print("ok", mode, flush=True)
assert hip.gemm_workspace_ok()
'''

_STACK = _COMMON + r'''
m = build(2, 16, b_std=0.05)
lm = m.model
emb = T("input.inputs_embeds", (2, 131, 4096), 0.05).cuda()
am = torch.ones(2, 131, dtype=torch.long)
am[1, 97:] = 0
for mode in ("bf16", "fp32"):
    res = {}
    for flag in (False, True):
        llama_mod.STACK_ENTRY = flag
        with runtime.use_dtype(mode):
            h_pad, _ = lm.prefill(emb, hip.with_host(am, "cuda"))
            cache = lm.new_cache(2, 140, "cuda")
            h_c, _ = lm.prefill(emb, None, cache=cache)
            res[flag] = (h_pad.clone(), h_c.clone(), [c[:, :131].clone() for c in cache.qkv])
    assert torch.equal(res[False][0][0], res[True][0][0]) and torch.equal(res[False][0][1, :97], res[True][0][1, :97]), "padded rows"
    assert torch.equal(res[False][1], res[True][1]), "into the KV cache"
    for a, b in zip(res[False][2], res[True][2]):
        assert torch.equal(a, b)
    print("ok", mode, flush=True)
assert hip.gemm_workspace_ok()
'''

_FRESH = _COMMON + r'''
emb = T("input.inputs_embeds", (2, 67, 4096), 0.05).cuda()
base = STLLMForCausalLM(StllmConfig(num_hidden_layers=2), device="cuda")
synth.fill_module_(base, 0, "")
m = build(2, 16)                    # B = 0: peft's init
for mod in m._lora_modules():
    assert float(mod.B.abs().max()) == 0.0
for mode, _ in MODES:
    with runtime.use_dtype(mode):
        a = base(samples=None, inputs_embeds=emb).logits
        b = m(samples=None, inputs_embeds=emb).logits
    assert torch.equal(a, b), mode
    print("ok", mode, flush=True)
'''

_MERGE = _COMMON + r'''
m = build(2, 16, b_std=0.05)
emb = T("input.inputs_embeds", (1, 67, 4096), 0.05).cuda()
_, mg = merged_sd(m)
w0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
with runtime.use_dtype("fp32"):
    act = m(samples=None, inputs_embeds=emb).logits.clone()
    m.merge_adapter()
    for li in range(2):
        for t in ("q_proj", "v_proj"):
            k = f"model.layers.{li}.self_attn.{t}"
            want = mg[k + ".weight"]
            got = m.state_dict()[k + ".base_layer.weight"].double().cpu()
            moved = float((want - w0[k + ".base_layer.weight"].double().cpu()).abs().max())
            err = float((got - want).abs().max()) / float(want.abs().max())
            assert moved >= 1e-3 * float(want.abs().max()) and err <= 1e-6, (k, err, moved)
    assert not m.model.lora_active()
    m.unmerge_adapter()
    for k, v in w0.items():
        err = float((m.state_dict()[k].double() - v.double()).abs().max()) / max(float(v.abs().max()), 1e-30)
        assert err <= 1e-6, (k, err)
    assert m.model.lora_active()
    m.merge_and_unload()
    assert not any("lora_" in k or "base_layer" in k for k in m.state_dict())
    plain = m(samples=None, inputs_embeds=emb).logits
    err = float((plain - act).abs().max()) / float(act.abs().max())
    print("merge_and_unload vs active", err, flush=True)
    assert err <= 2e-4, err
print("ok", flush=True)
'''

_DECODE = _COMMON + r'''
m = build(2, 16)
h_ref, l_ref = pick_b(m, T("gen.emb3", (1, 9, 4096), 0.05), None, 2e-4)
with torch.no_grad():
    m.lm_head.weight.mul_(4.0)
Bn, S, n_new = 2, 37, 3
emb = T("input.inputs_embeds", (Bn, S, 4096), 0.05).cuda()
new_emb = m.model.embed_tokens(torch.tensor([[5, 9, 1234], [31000, 8, 4]]))
with runtime.use_dtype("fp32"):
    lm = m.model
    cache = lm.new_cache(Bn, S + n_new, "cuda")
    _, h16 = lm.prefill(emb, None, cache=cache)
    steps = [m.logits_from(h16.view(Bn, S, -1)[:, -1].contiguous(), Bn, 1)[:, 0]]
    for t in range(n_new):
        _, h16 = lm.decode_step(new_emb[:, t:t + 1], cache)
        steps.append(m.logits_from(h16, Bn, 1)[:, 0])
    full = m(samples=None, inputs_embeds=torch.cat([emb, new_emb], dim=1)).logits
    scale = float(full.abs().max())
    for t, lg in enumerate(steps):
        err = float((lg - full[:, S - 1 + t]).abs().max())
        assert err <= 2e-4 * scale, (t, err, scale)
    ids = {}
    for state in ("active", "merged"):
        if state == "merged":
            m.merge_adapter()
        for seed in (3, 4, 5):
            e = T(f"gen.emb{seed}", (1, 9, 4096), 0.05).cuda()
            for kw in (dict(num_beams=1), dict(num_beams=5)):
                ids[(state, seed, kw["num_beams"])] = m.generate(inputs_embeds=e, max_new_tokens=6, do_sample=False, min_length=1, **kw)[0].tolist()
    for (state, seed, nb), v in ids.items():
        if state == "active":
            assert v == ids[("merged", seed, nb)], (seed, nb, v, ids[("merged", seed, nb)])
            print("ids", seed, nb, v, flush=True)
    m.unmerge_adapter()
for mode, tol in (("bf16", 5e-2), ("fp16", 1e-2)):    # the fast modes' adapted decode step (down projection at M = 1..2 + GEMV over K = D + P) against the full prefill
    with runtime.use_dtype(mode):
        cache = lm.new_cache(Bn, S + n_new, "cuda")
        lm.prefill(emb, None, cache=cache)
        _, h16 = lm.decode_step(new_emb[:, :1], cache)
        step = m.logits_from(h16, Bn, 1)[:, 0].float()
        fullm = m(samples=None, inputs_embeds=torch.cat([emb, new_emb[:, :1]], dim=1)).logits[:, S].float()
        err = float((step - full[:, S]).abs().max()) / scale
        print(mode, "decode step vs fp32 full prefill", err, "vs same-mode prefill", float((step - fullm).abs().max()) / scale, flush=True)
        assert err <= tol, (mode, err)
        out = m.generate(inputs_embeds=T("gen.emb3", (1, 9, 4096), 0.05).cuda(), max_new_tokens=4, num_beams=5, min_length=1)
        assert out.shape[0] == 1 and 1 <= out.shape[1] <= 4 and int(out.max()) < 32000
assert hip.gemm_workspace_ok()
print("ok", flush=True)
'''


_TRAIN = r'''
import sys
sys.path[:0] = ["tests", "oracle", "."]
import numpy as np, torch
torch.set_grad_enabled(False)
import _lora_train_case as C
from stllm_amd import runtime, training
mode = sys.argv[1]
cfg, model, samples, osamples = C.build_model("cuda")
want_loss, want = C.oracle_grads(cfg, model, osamples, None)
names = {n for n, _ in training.trainable_parameters(model)}
assert set(want) == names, set(want) ^ names
with runtime.use_dtype(mode):
    loss, _, grads = training.loss_and_grads(model, samples)
    torch.cuda.synchronize()
    for n in sorted(names):
        got, w = grads[n].float().cpu(), want[n]
        if mode == "fp32":      # tests/test_train_gpu.py: 5e-4 of each tensor's abs-max
            err, scale = float((got - w).abs().max()), float(w.abs().max())
            print(n, "err", err, "abs-max", scale, flush=True)
            assert scale > 0 and err <= 5e-4 * scale, (n, err, scale)
        else:                   # bf16: cosine >= 0.995 per tensor
            cs = float((got * w).sum() / (got.norm() * w.norm() + 1e-30))
            print(n, "cos", cs, flush=True)
            assert cs >= 0.995, (n, cs)
    assert abs(loss.item() - want_loss) <= (2e-4 if mode == "fp32" else 2e-2) * abs(want_loss), (loss.item(), want_loss)
    if mode == "fp32":          # one step: lora_B moves, the base Llama weights stay bit-identical, the next forward runs the updated adapters
        opt = training.AdamW(list(training.trainable_parameters(model)), lr=1e-3, max_grad_norm=1.0)
        base = {n: p.detach().clone() for n, p in model.named_parameters() if "lora_" not in n and not n.startswith("model.stllm_model.")}
        lb = {n: p.detach().clone() for n, p in model.named_parameters() if "lora_B" in n}
        l0, _, norm = training.train_step(model, samples, opt)
        now = dict(model.named_parameters())
        assert all(torch.equal(now[n], v) for n, v in base.items())
        assert all(not torch.equal(now[n], v) for n, v in lb.items())
        l1 = model(samples=samples).loss.item()
        fresh = training.loss_and_grads(model, samples)[0].item()
        assert abs(l1 - fresh) <= 1e-4 * abs(fresh) and l1 < l0.item() - 1e-3, (l0.item(), l1, fresh)
print("ok", mode, flush=True)
'''


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_training_step_with_adapters_matches_autograd_through_the_oracle(mode):
    out = _child(["-c", _TRAIN, mode], timeout=900)
    assert "ok " + mode in out, out[-2000:]


@pytest.mark.gpu
def test_lora_down_kernel_matches_fp64_and_is_deterministic():
    out = _child(["-c", _KERNEL], timeout=600)
    assert out.count("ok ") == 9, out[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["padded", "s576"])
def test_forward_with_active_adapters_matches_oracle_on_merged_weights(case):
    out = _child(["-c", _FORWARD, case], timeout=900)
    assert out.count("ok ") == 3, out[-2000:]


@pytest.mark.gpu
def test_fresh_adapters_are_bit_identical_to_the_base_model():
    out = _child(["-c", _FRESH], timeout=600)
    assert out.count("ok ") == 3, out[-2000:]


@pytest.mark.gpu
def test_stack_entry_equals_per_op_path_with_adapters():
    out = _child(["-c", _STACK], timeout=600)
    assert out.count("ok ") == 2, out[-2000:]


@pytest.mark.gpu
def test_merge_unmerge_and_unload_on_device():
    out = _child(["-c", _MERGE], timeout=600)
    assert "ok" in out, out[-2000:]


@pytest.mark.gpu
def test_decode_with_adapters_matches_merged_model():
    out = _child(["-c", _DECODE], timeout=900)
    assert "ok" in out.splitlines()[-1], out[-2000:]
