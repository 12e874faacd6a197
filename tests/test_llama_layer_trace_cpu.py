"""CPU: every Llama host path (prefill, extend, decode_step in all its cache shapes and weight modes, sp_layer_part) makes the calls into `hip` that it
made before the decoder-layer body was written once — same functions, same order, same scalars, same views of the same buffers.  The recorded trace
(tests/golden/llama_layer_trace.json) was written by tests/golden/make_layer_trace.py on the commit before that change; the recorder is replayed here."""
import importlib.util
import json
import os

import pytest

from _util import GOLDEN

_spec = importlib.util.spec_from_file_location("make_layer_trace", os.path.join(GOLDEN, "make_layer_trace.py"))
MT = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MT)

with open(MT.OUT) as _f:
    WANT = json.load(_f)


@pytest.fixture(scope="module")
def got():
    return json.loads(MT.dumps(MT.record()))   # through JSON, as the recorded trace went


def test_the_recorded_cases_are_the_cases_of_the_recorder(got):
    assert list(got["cases"]) == list(WANT["cases"]) and len(WANT["cases"]) == 22


@pytest.mark.parametrize("case", list(WANT["cases"]))
def test_layer_paths_make_the_recorded_calls(got, case):
    have, want = got["cases"][case], WANT["cases"][case]
    for i, (h, w) in enumerate(zip(have, want)):
        assert h == w, f"{case}: call {i} differs"
    assert len(have) == len(want), f"{case}: {len(have)} calls, recorded {len(want)}"


def test_uploads_per_decode_step(got):
    """hip.h2d calls of one decode step: none on a uniform cache, lengths + lengths + 1 on a ragged one, total positions + the two local tables behind a base"""
    assert got["h2d_per_decode_step"] == WANT["h2d_per_decode_step"] == {"uniform": 0, "ragged": 2, "shared": 3}
