"""GPU: the training step makes the launches it made when tests/golden/train_call_trace.json was written - the same entry points in
the same order with the same arguments on the same streams (tools/gen_train_call_trace.py says what a line holds and which cases
are taken).  The host code of lightningfastspeech2_amd/training.py can be rearranged freely under this test; a change that means to
alter the launches regenerates the fixture with the tool."""
import functools
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_train_call_trace as gen  # noqa: E402

pytestmark = pytest.mark.gpu
with open(gen.FIXTURE) as _fh:
    GOLDEN = json.load(_fh)


@functools.lru_cache(maxsize=None)
def _cases():
    return gen.cases()


def test_the_fixture_holds_the_cases_of_the_tool():
    assert list(GOLDEN) == list(_cases())
    assert any(" side" in line for line in GOLDEN["wide-bf16"]) and not any(" side" in line for line in GOLDEN["wide-fp32"])


@pytest.mark.parametrize("name", list(GOLDEN))
def test_training_step_makes_the_recorded_launches(name):
    got, want = gen.trace(*_cases()[name]), GOLDEN[name]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: launch {i} of {len(want)} differs\n   now: {g}\n fixture: {w}"
    assert len(got) == len(want), (name, len(got), len(want), (got + want)[min(len(got), len(want))])
