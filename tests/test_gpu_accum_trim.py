"""The packed accumulate reproduces the recorded results of its parent bit for bit.

tests/golden/accum_trim_golden.npz holds dx and Twc of the calls listed in
tests/golden/make_accum_trim_golden.py, recorded from a build of the commit BEFORE the accumulate's
step loop was unrolled by two, its addresses became 32-bit offsets and a lane of the
ray-constrained calib stream kept its pixel columns from step to step.  None of that touches a
floating-point operation, an operand or the order of the sums, and the kernel's sums have a fixed
order, so every array must be `array_equal`.

What runs which loop shape (4 points per lane and step, 1024 per workgroup and step):
  small graphs (6 keyframes, 10 directed edges): the planner cuts these images into chunks of at
    most 1024 points, so a workgroup runs one step -- partial (24x32: 768 points; 36x64: 3 chunks of
    768; 40x52: 696, 696, 688) or full (48x64, 64x64);
  deep graphs (65 keyframes, 4096 directed edges): a chunk is the whole image, so the unrolled loop
    runs 2 full steps and a partial one (36x64, and 40x52 whose width does not divide 1024: the
    path that divides by the width every step), exactly 3 steps (48x64: odd) and exactly 4
    (64x64: even); the rays and points modes (2 points per lane) run 4 full steps and a partial one.
3 iterations run the kernel that builds the packed records and then the one that reads them;
M3S_GN_PACK=2 at 1 iteration runs the former alone.
"""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_accum_trim_golden",
                                               os.path.join(HERE, "golden", "make_accum_trim_golden.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def golden():
    with np.load(rec.GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_recording_covers_every_call(golden):
    want = {f"{spec[0]}/{mode}/{tag}/{what}" for spec in rec.GRAPHS for mode in rec.MODES[spec[0]]
            for tag, _, _ in rec.CALLS for what in ("Twc", "dx")}
    want |= {f"{spec[0]}/{mode}/inputs" for spec in rec.GRAPHS for mode in rec.MODES[spec[0]]}
    assert set(golden) == want


@pytest.mark.parametrize("spec", rec.GRAPHS, ids=[s[0] for s in rec.GRAPHS])
def test_accumulate_is_bitwise_the_recording(backend, golden, spec):
    g = rec.make_graph(spec)
    out = rec.run_graph(backend, g, rec.MODES[spec[0]])
    # the inputs first: a recording made from other inputs (another generator) compares nothing
    for k, v in out.items():
        if k.endswith("/inputs"):
            assert np.array_equal(v, golden[f"{spec[0]}/{k}"]), f"{spec[0]}/{k}: the synthetic inputs differ"
    bad = []
    for k, v in out.items():
        ref = golden[f"{spec[0]}/{k}"]
        assert np.isfinite(v).all(), k
        if not np.array_equal(v, ref):
            bad.append(f"{k}: max |diff| {np.abs(v.astype(np.float64) - ref).max():.3g}")
    assert not bad, "; ".join(bad)
