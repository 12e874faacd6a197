"""CPU (contract backend): the training step with LoRA adapters — dA, dB of every layer and the gradients of the other trainable tensors against
autograd through the oracle (tests/_lora_train_case.py), with and without an injected dropout mask; one train_step moves the adapters only.
Tolerance: 2e-4 of each tensor's abs-max (the CPU backward bound of the issue; tests/test_backward_cpu.py uses 3e-4 against the reference fixture)."""
import pytest
import torch

import _cpu_backend as CB
import _lora_train_case as C

torch.set_grad_enabled(False)
TOL = 2e-4


@pytest.mark.parametrize("dropout", [False, True])
def test_lora_gradients_match_autograd_through_the_oracle(dropout):
    from stllm_amd import runtime, training
    cfg, model, samples, osamples = C.build_model()
    names = {n for n, _ in training.trainable_parameters(model)}
    assert sum("lora_" in n for n in names) == 4 * C.LAYERS
    assert not any(n.startswith("model.layers") and "lora_" not in n for n in names) and "lm_head.weight" not in names   # the base LLM is frozen
    with CB.installed(), runtime.use_dtype("fp32"):
        n_rows = model(samples=samples).logits.shape[:2].numel()
        mask = C.feature_mask(C.LAYERS, n_rows) if dropout else None
        want_loss, want = C.oracle_grads(cfg, model, osamples, mask)
        base_loss, _ = C.oracle_grads(cfg, model, osamples, None)
        loss, _, grads = training.loss_and_grads(model, samples, lora_dropout=mask)
        assert model.model.wd_frag is True                    # the taped forward's switch does not leak
    if dropout:
        assert abs(want_loss - base_loss) > 1e-4 * abs(base_loss)   # the mask matters
    assert abs(loss.item() - want_loss) <= 1e-4, (loss.item(), want_loss)
    assert names <= set(grads) and set(want) == names, names ^ set(want)
    for n in sorted(names):
        scale = want[n].abs().max().item()
        err = (grads[n].cpu() - want[n]).abs().max().item()
        print(n, "err", err, "abs-max", scale)
        assert scale > 0 and err <= TOL * scale, (n, err, scale)


def test_train_step_updates_the_adapters_only_and_the_next_forward_sees_them():
    from stllm_amd import runtime, training
    cfg, model, samples, _ = C.build_model()
    with CB.installed(), runtime.use_dtype("fp32"):
        opt = training.AdamW(list(training.trainable_parameters(model)), lr=1e-3, max_grad_norm=1.0)
        l_before = model(samples=samples).loss.item()
        packed = model.model.pack()
        ptr = packed[0]["wqkv"].data_ptr()
        base = {n: p.detach().clone() for n, p in model.named_parameters() if "lora_" not in n and not n.startswith("model.stllm_model.")}
        lb = {n: p.detach().clone() for n, p in model.named_parameters() if "lora_B" in n}
        l0, _, norm = training.train_step(model, samples, opt)
        assert abs(l0.item() - l_before) <= 1e-4 and norm > 0
        now = dict(model.named_parameters())
        for n, v in base.items():
            assert torch.equal(now[n], v), n                  # every base Llama weight bit-identical
        for n, v in lb.items():
            assert not torch.equal(now[n], v), n
        assert model.model.pack()[0]["wqkv"].data_ptr() == ptr    # the frozen base weights were not packed again: columns refreshed in place
        l1 = model(samples=samples).loss.item()               # ... and the next forward runs the updated adapters (no stale pack)
        fresh = training.loss_and_grads(model, samples)[0].item()
    assert abs(l1 - fresh) <= 1e-4 and l1 < l0.item() - 1e-3, (l0.item(), l1, fresh)
