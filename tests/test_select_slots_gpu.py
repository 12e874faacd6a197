"""GPU (-m gpu): stllm_select_slots on the device.  The kernel cases of tests/test_select_slots_cpu.py, run under poisoned allocations: every launch bit-equal
(token, aux) to hip.select_tokens launched once per slot with that slot's n_prev, suppress_eos and u, and the state and id tables equal to the reference
update of tests/_select_slots_ref.py."""
import pytest
import torch

import _poison
import test_select_slots_cpu as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from stllm_amd import hip as h
    h.lib()
    return h


@pytest.mark.parametrize("V,slots", C.SHAPES)
def test_greedy_state_and_ids_on_device(hip, V, slots):
    with _poison.poisoned_allocations() as counts:
        C.greedy_state_and_ids(hip, "cuda", V, slots)
    assert counts.allocations > 0


def test_stop_sequences_on_device(hip):
    with _poison.poisoned_allocations():
        C.stop_sequences(hip, "cuda")


def test_ids_behind_n_gen_do_not_matter_on_device(hip):
    with _poison.poisoned_allocations():
        C.ids_behind_n_gen_do_not_matter(hip, "cuda")


@pytest.mark.parametrize("V,slots", C.SHAPES)
def test_sample_on_device(hip, V, slots):
    with _poison.poisoned_allocations():
        for config in range(len(C.SAMPLE_CONFIGS)):
            C.sample(hip, "cuda", V, slots, config)


def test_row_that_does_not_fit_raises_on_device(hip):
    V = 39500
    lg = torch.zeros(1, V, device="cuda")
    src = torch.zeros(1, dtype=torch.int32, device="cuda")
    state = torch.tensor([[1, 0, 4, 0]], dtype=torch.int32, device="cuda")
    hip.select_tokens(lg, torch.zeros(1, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="LDS"):
        hip.select_slots(lg, src, state, torch.zeros((1, 512), dtype=torch.int32, device="cuda"))
    assert state.tolist() == [[1, 0, 4, 0]], "nothing ran in its place"
