"""The loss kernels' bits against the build they were recorded from: tests/golden/loss_bits.json holds the SHA-256 of every output
(loss, stats, gradient, probabilities) of every entry point of csrc/loss.hip and csrc/lovasz.hip on the fixed inputs of
tests/loss_bits_cases.py, written by scripts/record_loss_bits.py on the MI355X at the commit the file names.  A change to these
kernels that is meant to keep their arithmetic has to reproduce every digest; one that is meant to change it re-records the file."""

import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import loss_bits_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded(golden_dir):
    with open(os.path.join(golden_dir, "loss_bits.json")) as fp:
        return json.load(fp)


def test_the_record_names_its_origin_and_every_shape(recorded):
    assert len(recorded["commit"]) == 40 and "HIP version" in recorded["compiler"]
    assert sorted(recorded["shapes"]) == sorted(cases.shape_key(s) for s in cases.SHAPES)


@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.shape_key)
def test_every_entry_point_reproduces_the_recorded_bits(recorded, shape):
    want = recorded["shapes"][cases.shape_key(shape)]
    got = cases.run_shape(shape)
    assert sorted(got) == sorted(want), "the cases run and the cases recorded differ"
    wrong = ["{}: {}".format(k, ", ".join(o for o in want[k] if got[k].get(o) != want[k][o])) for k in sorted(want) if got[k] != want[k]]
    assert not wrong, "{} of {} cases differ from the recorded build:\n{}".format(len(wrong), len(want), "\n".join(wrong))
