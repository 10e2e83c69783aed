"""The host model of the direct solve (tests/solve_model.py) on the CPU oracle's systems -- no GPU.

tests/test_gpu_solve_exact.py holds every direct GN solve path to solve_model.bound around an
extended-precision solve.  What makes that a condition the reference alone satisfies, and one a
subtly wrong solver does not, is checked here on oracle.gn_build_system:
  * solve_ld leaves a residual at longdouble level, the oracle's own Cholesky lies inside the
    bound, and e64 (what a float64 Cholesky loses over 8 elimination orders) is 1e-15 .. 1e-9;
  * the ill-conditioned fixture (one pose observed by `keep` points only) has cond > 1e8, no
    float64 Cholesky of it fails in any ordering, and e64 stays far inside float32's half ulp;
  * three deliberately wrong solves each violate the bound: a Schur complement rounded to float32
    once, one rank-1 update of one 7x7 block dropped, one back-substitution term of the
    smallest-|x| pose dropped -- the last one while passing the solver-against-solver tests'
    1e-8 max|dx| criterion.

Measured on the oracle's systems (24x32, seed 3), cond / e64 of the weakly observed fixture:
  graph     keep   rays               calib              points
  clique12     3   1.2e+12 / 1.8e-09  3.2e+11 / 9.2e-10  8.7e+10 / 1.9e-10
  clique12     8   2.9e+09 / 4.8e-11  1.6e+09 / 6.9e-12  1.5e+09 / 2.0e-11
  clique29     3   2.6e+12 / 1.3e-09  1.1e+12 / 2.6e-10  3.4e+11 / 2.7e-11
  clique29     8   7.5e+09 / 3.5e-11  5.0e+09 / 1.6e-11  4.8e+09 / 4.3e-12
  cfg3 round   3   5.8e+12 / 5.6e-09  1.3e+12 / 1.7e-09  2.6e+10 / 1.4e-10
  cfg3 round   8   1.4e+09 / 2.2e-11  1.7e+09 / 4.4e-12  1.4e+09 / 3.3e-11
  cfg3 core    3   1.4e+12 / 8.7e-10  not pos. definite  1.2e+11 / 6.1e-10
  cfg3 core    5          -           5.8e+10 / 1.5e-10         -
  cfg3 core    8   1.0e+09 / 4.9e-12  3.5e+08 / 6.2e-12  3.5e+08 / 2.6e-12
(cfg3's core pose in calib is the one cell that takes keep = 5 for 3: solve_model.CFG3_SINGULAR.)
The kept points are the edge's first live ones, neighbours in a pixel row: harder than points
spread over the image (every second live point: 5e10 at keep = 3, 9e8 at keep = 8 in rays, but
9e7 in points), and 4 e64 still stays inside float32's half ulp of the largest component (3e-8).
The plain cliques: cond 8e2 .. 4e4, e64 1e-14 .. 7e-14.
"""
import functools

import numpy as np
import pytest

from tests import solve_model as sm
from tests.test_gpu_gn import _params

KEEPS = (3, 8)  # the values tests/test_gpu_solve_exact.py uses


@functools.lru_cache(maxsize=None)
def _system(oracle, name, mode, keep=None, pose=None):
    g = sm.graph(name, mode)
    if keep is not None:
        g = sm.weakly_observed(g, keep, pose)
    H, b = sm.oracle_system(oracle, g, mode, _params)
    x = sm.solve_ld(H, b)
    return H, b, x, sm.e64(H, b, x)


# ---- the model itself ----
def test_solve_ld_on_a_known_system():
    rng = np.random.default_rng(0)
    Q, _ = np.linalg.qr(rng.standard_normal((140, 140)))
    A = (Q * np.geomspace(1.0, 1e10, 140)) @ Q.T
    A = (A + A.T) / 2
    rhs = A.astype(np.longdouble) @ np.ones(140, np.longdouble)  # (in float64 its rounding alone costs 1e-6)
    x = sm.solve_ld(A, rhs)
    assert x.dtype == np.longdouble and np.finfo(np.longdouble).nmant >= 63
    # cond 1e10 in a 64-bit mantissa: ~1e-9 at worst; float64 cannot (1e10 * 2^-53 = 1e-6)
    assert np.abs(x - 1).max() < 1e-8
    assert sm.residual_ld(A, rhs, x) < 2.0 ** -60
    # only the lower triangle is read
    U = A.copy()
    U[np.triu_indices(140, 1)] = 7.0
    assert np.array_equal(sm.solve_ld(U, rhs), x)


def test_solve_ld_raises_on_a_pivot_that_is_not_positive():
    A = np.diag([1.0, 2.0, 0.0, 3.0])
    with pytest.raises(sm.PivotFailure, match="pivot 2"):
        sm.solve_ld(A, np.ones(4))
    A[2, 2] = np.nan
    with pytest.raises(sm.PivotFailure):
        sm.solve_ld(A, np.ones(4))
    with pytest.raises(np.linalg.LinAlgError):
        sm.e64(np.diag([1.0, -1.0] + [1.0] * 5), np.ones(7), np.ones(7))


def test_bound_terms():
    x = np.array([1.0, 1e-3, -3.0, 0.0] + [0.0] * 3)
    b = sm.bound(x, 0.0)
    floor = 4 * 7 * 2.0 ** -53 * 3.0
    assert np.allclose((b - floor)[:4], [2.0 ** -24, 2.0 ** -34, 2.0 ** -23, 0.5 * np.spacing(np.float32(0))], rtol=1e-6, atol=0)
    assert np.allclose(sm.bound(x, 1e-10) - 0.5 * sm.ulp_f32(x), 4 * 1e-10 * 3.0)
    # dx = -(float)x passes at ratio <= 1, one float32 ulp off fails
    xr = np.random.default_rng(1).standard_normal(70)
    dx = (-xr).astype(np.float32)
    assert sm.errors(dx, xr, 0.0)[0].max() <= 1.0
    dx[3] = np.nextafter(dx[3], np.float32(9))
    assert sm.errors(dx, xr, 0.0)[0][3] > 1.0
    assert sm.dx_norm_f32(np.array([3.0, 4.0], np.float32)) == np.float32(5.0)


# ---- on the oracle's systems ----
@pytest.mark.parametrize("mode", sm.MODES)
@pytest.mark.parametrize("name", ["clique4", "clique12", "clique21"])
def test_model_on_oracle_systems(oracle, name, mode):
    H, b, x, E = _system(oracle, name, mode)
    n = b.shape[0]
    res = sm.residual_ld(H, b, x)
    x_o, rc = oracle.cholesky_solve(H, b)
    ratio, _ = sm.errors(-x_o, x, E)
    print(f"{name}-{mode}: n {n} cond {np.linalg.cond(H):.1e} residual {res:.1e} e64 {E:.1e} "
          f"oracle's Cholesky err / bound {ratio.max():.2e}")
    assert res < 2.0 ** -60, res
    assert rc == 0 and ratio.max() <= 1.0, ratio.max()
    assert 1e-15 < E < 1e-9, E


@pytest.mark.parametrize("mode", sm.MODES)
@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("name", ["clique12", "clique29"])
def test_weakly_observed_fixture_is_hard_and_not_singular(oracle, name, keep, mode):
    H, b, x, E = _system(oracle, name, mode, keep)  # (e64 raises if an ordering's factor fails)
    cond = np.linalg.cond(H)
    half_ulp = 2.0 ** -25  # float32's, of the largest component, relative
    print(f"{name}-{mode}-keep{keep}: cond {cond:.1e} e64 {E:.1e}")
    assert cond > 1e8, cond
    assert 1e-15 < E and 4 * E < half_ulp, E  # (the reference alone stays inside float32's half ulp)
    x_o, rc = oracle.cholesky_solve(H, b)
    assert rc == 0 and sm.errors(-x_o, x, E)[0].max() <= 1.0


@pytest.mark.parametrize("where,mode,keep", sm.CFG3_CELLS)
def test_weakly_observed_fixture_in_cfg3(oracle, backend, where, mode, keep):
    """cfg3's weak pose is a round pose / a core pose of the shipped plan, and the fixture is hard
    and not singular there too: keep = 3 and 8, but for the core pose in calib, which takes 5
    (solve_model.CFG3_SINGULAR; the test below keeps that exception honest)."""
    g = sm.graph("cfg3", mode)
    p = backend.gn_plan_info(g.ii, g.jj, g.N)
    assert (p["solver"], p["rounds"], p["core_poses"]) == ("hybrid", 5, 34)
    assert sm.CFG3_WEAK_POSE[where] - 1 == (p["order"][0] if where == "round" else p["order"][-1])
    H, b, x, E = _system(oracle, "cfg3", mode, keep, sm.CFG3_WEAK_POSE[where])
    cond = np.linalg.cond(H)
    print(f"cfg3-{where}-{mode}-keep{keep}: cond {cond:.1e} e64 {E:.1e}")
    assert cond > 1e8, cond
    assert 1e-15 < E and 4 * E < 2.0 ** -25, E


def test_the_one_cfg3_cell_that_does_not_take_keep_3_is_singular(oracle):
    """The core pose in calib with keep = 3: the system is not positive definite, so that cell
    alone runs with 5.  Should it become solvable, the exception goes."""
    where, mode, keep = sm.CFG3_SINGULAR
    g = sm.weakly_observed(sm.graph("cfg3", mode), keep, sm.CFG3_WEAK_POSE[where])
    H, b = sm.oracle_system(oracle, g, mode, _params)
    with pytest.raises(sm.PivotFailure):
        sm.solve_ld(H, b)
    assert [c for c in sm.CFG3_CELLS if c[2] not in KEEPS] == [("core", "calib", 5)]


# ---- sensitivity: what the bound sees of a wrong solve ----
FIXTURES = [("clique12", "rays", None), ("clique12", "calib", 8), ("clique29", "points", 3)]


def _as_dx(x):
    return (-np.asarray(x, np.float64)).astype(np.float32)


@pytest.mark.parametrize("name,mode,keep", FIXTURES)
def test_right_solves_pass(oracle, name, mode, keep):
    H, b, x, E = _system(oracle, name, mode, keep)
    assert sm.errors(_as_dx(x), x, E)[0].max() <= 1.0
    assert sm.errors(_as_dx(np.linalg.solve(H, b)), x, E)[0].max() <= 1.0
    assert sm.errors(_as_dx(sm._substitute(sm._chol_right_looking(sm._sym_lower(H, np.float64)), b)), x, E)[0].max() <= 1.0


@pytest.mark.parametrize("name,mode,keep", FIXTURES)
def test_schur_complement_rounded_to_f32_violates_the_bound(oracle, name, mode, keep):
    H, b, x, E = _system(oracle, name, mode, keep)
    r = sm.errors(_as_dx(sm.wrong_schur_f32(H, b)), x, E)[0]
    print(f"{name}-{mode}-{keep}: err / bound {r.max():.2e}, {int((r > 1).sum())} of {r.size} components outside")
    assert (r > 1.0).any()


@pytest.mark.parametrize("name,mode,keep", FIXTURES)
def test_dropped_rank1_update_violates_the_bound(oracle, name, mode, keep):
    H, b, x, E = _system(oracle, name, mode, keep)
    r = sm.errors(_as_dx(sm.wrong_dropped_update(H, b)), x, E)[0]
    print(f"{name}-{mode}-{keep}: err / bound {r.max():.2e}, {int((r > 1).sum())} of {r.size} components outside")
    assert (r > 1.0).any()


@pytest.mark.parametrize("name,mode,keep", FIXTURES)
def test_dropped_back_substitution_term_passes_the_old_criterion_not_the_bound(oracle, name, mode, keep):
    """The case the max-norm tests cannot see: one back-substitution term of the smallest-|x|
    pose dropped, small enough (at most 0.5e-8 max|x|) to pass 1e-8 max|dx| -- and outside the
    per-component bound."""
    H, b, x, E = _system(oracle, name, mode, keep)
    below = 0.5e-8 * float(np.abs(x).max())
    xw, pose, change = sm.wrong_dropped_back_term(H, b, x, below)
    r, ulps = sm.errors(_as_dx(xw), x, E)
    print(f"{name}-{mode}-{keep}: pose {pose} max|x_pose| / max|x| "
          f"{np.abs(x[7 * pose:7 * pose + 7]).max() / np.abs(x).max():.1e} change {change / np.abs(x).max():.1e} max|x| "
          f"err / bound {r.max():.2e} ({ulps.max():.1f} ulp)")
    # (the well-conditioned clique has no pose that weakly coupled: there every term shows in
    # the max norm too)
    assert change <= below or keep is None
    if change <= below:
        assert sm.old_criterion(_as_dx(xw), _as_dx(x))
    assert (r > 1.0).any()
    assert np.flatnonzero(r > 1.0).min() // 7 == pose == np.flatnonzero(r > 1.0).max() // 7
