"""The float32 restatement of the tracker's accumulate (tests/track_model.py, sums_f32) against
the float64 sums of the oracle's solve (sums_f64), on the host: no GPU.

(a) The restatement stays inside the bound tests/test_gpu_track_sums.py holds the kernel to
    (track_model.errors, TOL = 2e-5), at 24x32, 37x53 and 96x128, both modes, with the start 0,
    0.02 and 0.1 (times 7 standard normals, retracted) away from the generating pose.
(b) Every deliberate error of track_model.MUTATIONS pushes the same comparison, on the same
    inputs, outside the bound: the bound tells a wrong accumulate from a right one.

The inputs (track_model.model_case) are stronger than oracle.make_tracking_pair alone, on which
three of the errors change nothing: 10 % gross outliers (at a start on the truth no residual of a
calib pair reaches the huber threshold otherwise), fy = 0.85 fx (fx == fy hides a mixed-up focal
length), and for calib the mask groups of track_model.masked_calib (every point of a plain pair
is inside the border, in front of the camera and measured).

Measured (this file, worst over the 18 inputs): the restatement differs from the float64 sums by
4.1e-6 (H), 1.4e-6 (g) and 1.1e-7 (cost) of the normalisers, against the bound 2e-5.  On plain
make_tracking_pair inputs started on the truth g reaches 6.4e-6: the residuals there are float32
differences of nearly equal numbers.  The smallest error of a mutation (its largest of the three
components, the smallest over the inputs) is 1.1e-4 for dup_first and 3.0e-4 for drop_last, both
at 96x128 (one point of 12288); every other mutation is at 0.1 or above.
"""
import functools

import numpy as np
import pytest

import track_model as TM
from oracle import track_oracle as TO

CFG = TO.TRACKING_CFG
SHAPES = [(24, 32), (37, 53), (96, 128)]
PERTS = [0.0, 0.02, 0.1]


@functools.lru_cache(maxsize=None)
def _case(mode, hw, pert):
    p, T = TM.model_case(mode, hw, pert, CFG)
    Ho, go, co, aux = TM.sums_f64(mode, p, T, CFG, hw)
    return p, T, Ho, go, co, aux


@pytest.mark.parametrize("pert", PERTS)
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("mode", ["rays", "calib"])
def test_f32_model_inside_the_bound(mode, hw, pert):
    p, T, Ho, go, co, aux = _case(mode, hw, pert)
    # the input exercises what the mutations change
    act = aux["si"] != 0
    share = float((np.abs(aux["wr"][act]) >= CFG["huber"]).mean())
    assert 0.05 <= share <= 0.95, share
    if mode == "calib":
        masked = 1.0 - float((aux["ok"] & np.asarray(p["valid"])[:, 0]).mean())
        assert 0.2 <= masked <= 0.6, masked
        assert TM.border_distance(aux["uv"], hw, CFG["pixel_border"]).min() > 1e-2
        assert np.abs(aux["X"][:, 2]).min() > 1e-3
    e = TM.errors(*TM.sums_f32(mode, p, T, CFG, hw), Ho, go, co)
    print(f"{mode} {hw} pert {pert}: f32 model vs f64 sums H {e[0]:.2e} g {e[1]:.2e} cost {e[2]:.2e}, "
          f"huber share {share:.2f}")
    assert max(e) <= TM.TOL, e


@pytest.mark.parametrize("pert", PERTS)
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("mutation,mode", [(m, mode) for m, modes in TM.MUTATIONS.items() for mode in modes])
def test_mutation_outside_the_bound(mutation, mode, hw, pert):
    p, T, Ho, go, co, _ = _case(mode, hw, pert)
    e = TM.errors(*TM.sums_f32(mode, p, T, CFG, hw, mutate=mutation), Ho, go, co)
    print(f"{mutation} {mode} {hw} pert {pert}: H {e[0]:.2e} g {e[1]:.2e} cost {e[2]:.2e}")
    assert max(e) > TM.TOL, e


def test_pack_roundtrip_and_layout():
    """unpack36 reads H's upper triangle row-major, then g, then the sum of b^2."""
    S = np.arange(36, dtype=np.float64) + 1.0
    H, g, c = TM.unpack36(S)
    assert H[0, 0] == 1 and H[0, 6] == 7 and H[1, 1] == 8 and H[6, 6] == 28 and H[3, 1] == H[1, 3]
    assert np.array_equal(g, np.arange(29, 36)) and c == 18.0
    assert np.array_equal(TM.pack36(H, g, c), S)


def test_f64_sums_are_the_oracles_solve():
    """sums_f64 at the start pose gives the oracle's first step: tau = H^-1 g retracts to the
    oracle's pose after one iteration, and the costs agree."""
    for mode in ("rays", "calib"):
        hw = (24, 32)
        p = TO.make_tracking_pair(hw, seed=3, mode=mode, noise=0.003)
        T0 = TO.sim3_mul(TO.sim3_inv(np.asarray(p["T_WCk"], np.float64)), np.asarray(p["T_WCf"], np.float64))
        H, g, c, _ = TM.sums_f64(mode, p, T0, CFG, hw)
        T1 = TO.sim3_retr(T0, np.linalg.solve(H, g))
        cfg = dict(CFG, rel_error=0.0, delta_norm=0.0)
        if mode == "rays":
            _, To, _, co = TO.opt_pose_ray_dist_sim3(p["Xf"], p["Xk"], p["T_WCf"], p["T_WCk"], p["Qk"], p["valid"], cfg, 1)
        else:
            _, To, _, co = TO.opt_pose_calib_sim3(p["Xf"], p["T_WCf"], p["T_WCk"], p["Qk"], p["valid"], p["meas_k"],
                                                  p["valid_meas_k"], p["K"], hw, cfg, 1)
        np.testing.assert_allclose(T1, To, rtol=0, atol=1e-10)
        assert abs(c - co) <= 1e-12 * co
