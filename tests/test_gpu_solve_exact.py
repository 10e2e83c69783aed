"""Every direct Gauss-Newton solve path held to an extended-precision solve of its own system.

The solver-against-solver tests of test_gpu_gn.py compare two GPU solvers in the max norm at
1e-8 max|dx|, in rays mode on one seed, on whatever plan the switches fell back to.  Here one call
is ONE iteration, the dense system (H, b) of that iteration is read back from the GPU
(m3s.debug.build_system_gpu at the poses the call starts from, the same M3S_GN_PACK), and
tests/solve_model.py says what the step must be:
    x_ref = solve_ld(H, b)                 Cholesky in numpy.longdouble
    E     = e64(H, b, x_ref)               what a float64 Cholesky loses over 8 elimination orders
    |dx_i + x_ref_i| <= 0.5 ulp_f32(x_ref_i) + 4 max(E, n 2^-53) max|x_ref|      for every i
    Twc == retracted(oracle, Twc_0, dx)    bit for bit (every copy of the retraction)
    two runs bitwise equal
PATHS pins each solver by environment, and expected_plan states the plan m3s_gn_plan_info must
report under that environment (solver, rounds, core poses), so a fallback fails the row instead of
testing another path; the rows that cannot run on the requested solver are listed as the
fallback they take.  What the plan cannot show: launch_dense_factor_solve takes the per-panel
launches when the dataflow launch itself returns a runtime error, so a row pinned with
M3S_CHOL_DF=1 (dense-df, s2-df, s3) would then pass on the other tile factor; and for the dense
rows nothing but the switch itself says that the dense solver ran.  Not covered: the copy of the
failure rule in sp_rounds_df_kernel (the ticketed rounds of gn_sparse.hip), which runs only as a
PCG iteration's fallback or under M3S_SOLVE_DF=2, read once per process; every call here runs
with M3S_GN_PCG=0.  The dense solver (M3S_SOLVER_DENSE=1) plans no elimination: run() skips
choose_sparse_plan, nothing else can run.  "s3" is M3S_SOLVER=3 as shipped (the hybrid's core
factored by chol_df); "s3-reg" adds M3S_HYB_CORE=0, the hybrid with gn_solve's in-register core.

Further: the first iteration of a call that starts from the poses an earlier call returned; the
ill-conditioned fixture (solve_model.weakly_observed: cond 1e9 .. 1e12, where the elimination
orders truly differ and the bound's second term counts); a pivot that fails late (one pose without
observations, placed at a tile boundary, in a late tile column, in the first / last elimination
round, at the first / last core pose); a NaN that passes through every solver; and the early-exit
compare two float32 ulps either side of ||dx|| in each copy of the retraction.

The two entry points build the same system: both go through setup(), prepare_iterations() and
enqueue_system(); run() lets its first accumulate build the packed records itself
(M3S_GN_PACK_FIRST, the same records) and assembles into the sparse solvers' block format instead
of the dense solver's compact one (the same sums in the same order).  The record below shows it: the
well-conditioned rows sit at the float32 rounding of x_ref (<= 0.5 ulp), not at 1e-6.

What these tests found: m3s_gn_debug_flags never reported a pivot failure.  The retraction that
acts on kFlagFail (it zeroes the step) clears it for the next iteration, so the flags read back
after the call held fail = 0 on all 54 pivot rows, through every solver.  The retractions now
leave a sticky kFlagFailed behind, and the readback reports it.

The record of a full run (MI355X).  Per row: n, cond(H), e64, and over the seven paths the largest
error / bound and the largest error in float32 ulps of its component (where the paths differ: their
range).  The bound itself always comes from the run's own model values, never from this record.
  row                mode      n     cond      e64  err / bound    ulp
  pair               rays      7  8.3e+03  1.5e-14  0.801          0.40
  pair               calib     7  5.8e+03  9.8e-15  0.799          0.40
  pair               points    7  1.9e+02  6.7e-16  0.833          0.42
  star6              rays     35  1.9e+04  3.7e-14  0.985          0.49
  star6              calib    35  1.5e+04  3.6e-14  0.999          0.50
  star6              points   35  2.7e+02  3.7e-15  0.989          0.49
  chain24            rays    161  5.3e+07  3.3e-11  0.982          0.50
  chain24            calib   161  2.2e+07  1.4e-11  0.963          0.50
  chain24            points  161  2.0e+05  3.8e-13  0.999          0.50
  hub23              rays    154  3.7e+06  5.8e-13  0.994          0.50
  hub23              calib   154  2.9e+06  2.3e-13  0.999          0.50
  hub23              points  154  8.3e+04  1.4e-13  0.999          0.50
  clique4            rays     21  2.6e+04  1.5e-14  0.998          0.50
  clique4            calib    21  1.7e+04  9.2e-15  0.968          0.48
  clique4            points   21  8.4e+02  1.0e-14  0.921          0.46
  clique12           rays     77  3.0e+04  5.9e-14  0.989          0.49
  clique12           calib    77  2.4e+04  7.0e-14  0.988          0.49
  clique12           points   77  2.3e+03  1.3e-14  0.984          0.49
  clique17           rays    112  3.4e+04  1.4e-13  1.000          0.50
  clique17           calib   112  2.9e+04  8.4e-14  0.997          0.50
  clique17           points  112  3.4e+03  2.0e-14  0.997          0.50
  clique21           rays    140  4.2e+04  5.8e-14  0.999          0.50
  clique21           calib   140  3.8e+04  6.9e-14  0.991          0.50
  clique21           points  140  4.2e+03  1.9e-14  0.996          0.50
  clique28           rays    189  5.8e+04  1.5e-13  0.995          0.50
  clique28           calib   189  5.3e+04  9.0e-14  0.992          0.50
  clique28           points  189  5.5e+03  3.0e-14  0.995          0.50
  clique29           rays    196  6.2e+04  1.5e-13  0.992          0.50
  clique29           calib   196  5.6e+04  2.0e-13  0.993          0.50
  clique29           points  196  5.7e+03  3.6e-14  0.992          0.50
  cfg3               rays    889  7.9e+05  1.2e-13  0.999          0.50
  cfg3               calib   889  6.3e+05  9.9e-14  0.999          0.50
  cfg3               points  889  8.9e+04  3.1e-14  1.000          0.50
  clique4-pack0      rays     21  2.6e+04  1.5e-14  0.998          0.50
  clique4-pack0      calib    21  1.7e+04  9.2e-15  0.910          0.46
  clique4-pack0      points   21  8.4e+02  1.0e-14  0.921          0.46
  hub23-from-Twc1    rays    154  2.3e+08  3.1e-12  0.993          0.50
  hub23-from-Twc1    calib   154  4.2e+07  1.0e-13  0.984          0.49
  hub23-from-Twc1    points  154  8.8e+04  2.2e-14  0.997          0.50
  clique12-keep3     rays     77  1.2e+12  9.0e-10  0.570          0.50
  clique12-keep3     calib    77  2.8e+11  1.0e-09  0.515          0.50
  clique12-keep3     points   77  1.1e+11  3.5e-10  0.901          0.49
  clique12-keep8     rays     77  2.8e+09  8.7e-12  0.899          0.50
  clique12-keep8     calib    77  1.6e+09  1.0e-11  0.862          0.50
  clique12-keep8     points   77  1.5e+09  7.9e-12  0.789          0.49
  clique29-keep3     rays    196  2.5e+12  5.6e-10  0.744          0.50
  clique29-keep3     calib   196  1.0e+12  3.1e-10  0.704          0.50
  clique29-keep3     points  196  3.0e+11  1.3e-10  0.553          0.50
  clique29-keep8     rays    196  7.5e+09  3.5e-11  0.989          0.50
  clique29-keep8     calib   196  5.0e+09  9.0e-12  0.917          0.49
  clique29-keep8     points  196  4.8e+09  3.6e-12  0.975          0.50
  cfg3-round-keep3   rays    889  2.1e+12  5.2e-09  0.630          0.51
  cfg3-round-keep8   rays    889  1.4e+09  1.6e-11  0.991          0.50
  cfg3-round-keep3   calib   889  9.4e+11  2.3e-10  0.921          0.50
  cfg3-round-keep8   calib   889  1.7e+09  7.5e-12  0.988          0.50
  cfg3-round-keep3   points  889  2.7e+10  2.0e-10  0.968          0.50
  cfg3-round-keep8   points  889  1.4e+09  5.1e-11  0.951          0.50
  cfg3-core-keep3    rays    889  1.2e+12  1.4e-09  0.654          0.50 .. 3.88
  cfg3-core-keep8    rays    889  1.0e+09  2.0e-12  0.995          0.50
  cfg3-core-keep5    calib   889  4.9e+10  2.8e-10  0.853          0.50
  cfg3-core-keep8    calib   889  3.4e+08  1.5e-12  0.996          0.50
  cfg3-core-keep3    points  889  1.0e+11  4.5e-10  0.747          0.50 .. 0.65
  cfg3-core-keep8    points  889  3.5e+08  4.2e-12  0.979          0.50
Largest err / bound 1.0000, largest error 3.88 float32 ulp, over 441 path rows.  The pivot rows: fail = 1,
done = 1, dx = 0 on all 54; the NaN rows: all 77 entries of dx NaN on every path.
"""
import contextlib
import dataclasses
import os

import numpy as np
import pytest

from tests import solve_model as sm
from tests.test_gpu_gn import LOCAL, _rel, _run_gpu, _run_oracle

pytestmark = pytest.mark.gpu

PATHS = {
    "dense-df": dict(M3S_SOLVER_DENSE=1, M3S_CHOL_DF=1),
    "dense-ml": dict(M3S_SOLVER_DENSE=1, M3S_CHOL_DF=0),
    "s1": dict(M3S_SOLVER=1),
    "s2-df": dict(M3S_SOLVER=2, M3S_CHOL_DF=1),
    "s2-ml": dict(M3S_SOLVER=2, M3S_CHOL_DF=0),
    "s3": dict(M3S_SOLVER=3),
    "s3-reg": dict(M3S_SOLVER=3, M3S_HYB_CORE=0),
}
SPARSE = tuple(p for p in PATHS if not p.startswith("dense"))
SOLVER_OF = {"s1": "fused", "s2-df": "multi", "s2-ml": "multi", "s3": "hybrid", "s3-reg": "hybrid"}
# topology -> (elimination rounds, core poses) of every sparse plan, but for the rows below
ROUNDS_CORE = {"pair": (0, 1), "star6": (1, 0), "chain24": (2, 5), "hub23": (1, 2), "clique4": (0, 3),
               "clique12": (0, 11), "clique17": (0, 16), "clique21": (0, 20), "clique28": (0, 27),
               "clique29": (0, 28), "cfg3": (5, 34)}
# (topology, path) -> (solver, rounds, core poses) where the requested solver cannot run, or plans otherwise
EXCEPTIONS = {
    ("pair", "s2-df"): ("multi", 1, 0), ("pair", "s2-ml"): ("multi", 1, 0),  # the multi plan eliminates it in a round
    ("clique29", "s1"): ("multi", 0, 28),       # 28 poses: beyond the in-register core, the multi plan
    ("clique29", "s3-reg"): ("multi", 0, 28),
    ("cfg3", "s1"): ("multi", 5, 34),           # more rounds than the single-workgroup solve stages
    ("cfg3", "s3-reg"): ("hybrid", 8, 26),      # rounds down to a core the registers hold
}
TOPOS = tuple(sm.TOPOLOGIES)


def expected_plan(topo, path):
    if path.startswith("dense"):
        return None
    return EXCEPTIONS.get((topo, path), (SOLVER_OF[path],) + ROUNDS_CORE[topo])


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _call(backend, g, mode, path, iters=1, delta=0.0, pack=2):
    """One op call on `path`: (Twc, dx, debug flags); gn_check raises a deferred timeout."""
    with _env(M3S_GN_DEBUG_FLAGS=2, M3S_GN_PACK=pack, M3S_GN_PCG=0, **PATHS[path]):
        T, dx = _run_gpu(backend, g, mode, iters, delta)
        backend.gn_check()
        return T, dx, backend.gn_debug_flags()


def _plan(backend, g, path):
    with _env(**PATHS[path]):
        return backend.gn_plan_info(g.ii, g.jj, g.N)


def _assert_plan(backend, g, topo, path):
    want = expected_plan(topo, path)
    if want is None:
        assert 7 * (g.N - 1) <= 8192  # (the dense solve's limit; it plans nothing else)
        return
    p = _plan(backend, g, path)
    assert (p["solver"], p["rounds"], p["core_poses"]) == want, (topo, path, p["solver"], p["rounds"], p["core_poses"])
    assert p["core_fits"]


class Reference:
    """Graph variants and the model's solves of the GPU-built systems, each made once."""

    def __init__(self, backend):
        self.backend = backend
        self._g, self._sys = {}, {}

    def graph(self, topo, mode, variant=None):
        """variant: None | ("weak", keep, pose) | ("unobserved", pose) | ("nan",).  The graph
        carries its key (g.key) for system()'s cache."""
        key = (topo, mode, variant)
        if key not in self._g:
            g = sm.graph(topo, mode)
            if variant is not None and variant[0] == "weak":
                g = sm.weakly_observed(g, variant[1], variant[2])
            elif variant is not None and variant[0] == "unobserved":
                g = sm.unobserved(g, variant[1])
            elif variant is not None:
                g = sm.nan_in_an_unread_point(g)
            g = dataclasses.replace(g)  # (a shallow copy: sm.graph's own object stays unmarked)
            g.key = key
            self._g[key] = g
        return self._g[key]

    def system(self, g, mode, pack=2, nperm=7):
        """dict(H, b, x, E, cond, n) of the system the GPU assembles at g.Twc."""
        from m3s.debug import build_system_gpu

        key = (g.key, g.Twc.numpy().tobytes(), pack, nperm)
        assert g.key[1] == mode
        if key not in self._sys:
            with _env(M3S_GN_PACK=pack):
                H, b = build_system_gpu(g, mode, LOCAL)
            x = sm.solve_ld(H, b)
            cond = float(np.linalg.cond(sm._sym_lower(H, np.float64)))
            self._sys[key] = dict(H=H, b=b, x=x, E=sm.e64(H, b, x, nperm), cond=cond, n=b.shape[0])
        return self._sys[key]


@pytest.fixture(scope="module")
def ref(backend):
    return Reference(backend)


def _check_step(backend, oracle, ref, g, mode, path, row, pack=2, runs=2):
    """Section 3's check of one one-iteration call from g.Twc."""
    s = ref.system(g, mode, pack)
    T0 = g.Twc.numpy()
    T, dx, st = _call(backend, g, mode, path, pack=pack)
    assert dx.shape == (g.N - 1, 7) and np.isfinite(dx).all() and np.isfinite(T).all()
    ratio, ulps = sm.errors(dx, s["x"], s["E"])
    print(f"ROW {row} {mode} {path}: n {s['n']} cond {s['cond']:.1e} e64 {s['E']:.1e} err/bound {ratio.max():.3f} "
          f"ulp {ulps.max():.2f}")
    bad = np.flatnonzero(ratio > 1.0)
    assert bad.size == 0, (row, mode, path, bad[:8], ratio[bad[:8]], ulps[bad[:8]])
    assert np.array_equal(T[0], T0[0])
    T_r = sm.retracted(oracle, T0, dx)
    assert np.array_equal(T, T_r), _rel(T, T_r)
    assert not st["fail"], st
    for _ in range(runs - 1):
        T2, dx2, _ = _call(backend, g, mode, path, pack=pack)
        assert np.array_equal(T2, T) and np.array_equal(dx2, dx)
    return T, dx


# ---- 3. each path against the extended-precision solve ----
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("mode", sm.MODES)
@pytest.mark.parametrize("topo", TOPOS)
def test_one_iteration_is_the_extended_precision_solve(backend, oracle, ref, topo, mode, path):
    g = ref.graph(topo, mode)
    _assert_plan(backend, g, topo, path)
    _check_step(backend, oracle, ref, g, mode, path, topo)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("mode", sm.MODES)
def test_one_iteration_with_the_unpacked_accumulate(backend, oracle, ref, mode, path):
    """M3S_GN_PACK=0 in both calls: the unpacked accumulate feeds the same solvers."""
    g = ref.graph("clique4", mode)
    _assert_plan(backend, g, "clique4", path)
    _check_step(backend, oracle, ref, g, mode, path, "clique4-pack0", pack=0)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("mode", sm.MODES)
def test_first_iteration_of_a_later_call(backend, oracle, ref, mode, path):
    """From Twc_1, the poses a one-iteration call returned: a call's first iteration that is not
    the graph's first step."""
    g = ref.graph("hub23", mode)
    _assert_plan(backend, g, "hub23", path)
    T1, _, _ = _call(backend, g, mode, path)
    g1 = sm.with_poses(g, T1)
    g1.key = g.key  # (system()'s cache key carries the poses too)
    _check_step(backend, oracle, ref, g1, mode, path, "hub23-from-Twc1")


# ---- ill-conditioned rows ----
KEEPS = (3, 8)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("mode", sm.MODES)
@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("topo", ["clique12", "clique29"])
def test_weakly_observed_pose(backend, oracle, ref, topo, keep, mode, path):
    g = ref.graph(topo, mode, ("weak", keep, None))
    _assert_plan(backend, g, topo, path)
    s = ref.system(g, mode)
    assert s["cond"] > 1e8, s["cond"]
    _check_step(backend, oracle, ref, g, mode, path, f"{topo}-keep{keep}")


def _cfg3_pose(backend, where):
    """solve_model.CFG3_WEAK_POSE by its place in the shipped plan (M3S_SOLVER=3): the first pose
    of the first round / the last core pose -- a round pose / a core pose of every sparse plan."""
    g = sm.graph("cfg3", "rays")
    p = _plan(backend, g, "s3")
    idx = {"round": p["order"][0], "core": p["order"][-1]}[where]
    assert idx + 1 == sm.CFG3_WEAK_POSE[where]  # (keyframe 0 is pinned)
    for path in SPARSE:
        q = _plan(backend, g, path)
        part = q["order"][:q["eliminated"]] if where == "round" else q["order"][q["eliminated"]:]
        assert idx in part, (where, path)
    return idx + 1


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("where,mode,keep", sm.CFG3_CELLS)
def test_weakly_observed_pose_in_cfg3(backend, oracle, ref, where, mode, keep, path):
    """keep = 3 and 8 as on the cliques; the core pose in calib takes 5 for 3, the one cell whose
    keep = 3 system is not positive definite (solve_model.CFG3_SINGULAR)."""
    g = ref.graph("cfg3", mode, ("weak", keep, _cfg3_pose(backend, where)))
    _assert_plan(backend, g, "cfg3", path)
    s = ref.system(g, mode)
    assert s["cond"] > 1e8, s["cond"]
    _check_step(backend, oracle, ref, g, mode, path, f"cfg3-{where}-keep{keep}")


# ---- 4. pivot failure wherever the flag can be raised ----
def _pivot_cases():
    c = []
    dense_pos = {"first": 0, "tile-boundary": 9, "tile-column-2": 22, "last": 27}  # free-pose positions of clique29
    for path in ("dense-df", "dense-ml", "s2-df", "s2-ml"):
        c += [("clique29", path, w) for w in dense_pos]
    for path in SPARSE:
        c += [("cfg3", path, w) for w in ("first-round", "last-round", "first-core", "last-core")]
    for path in ("s1", "s3", "s3-reg"):
        for topo in ("clique21", "clique28"):
            c += [(topo, path, w) for w in ("core-0", "core-2", "core-last")]
    return c, dense_pos


PIVOT_CASES, DENSE_POS = _pivot_cases()


def _pivot_pose(backend, g, topo, path, where):
    """The keyframe whose pivot fails: `where` as a position in the elimination order of `path`
    (the dense solver's: the free poses in keyframe order)."""
    if path.startswith("dense"):
        return DENSE_POS[where] + 1
    p = _plan(backend, g, path)
    order, rp, nel = p["order"], p["round_ptr"], p["eliminated"]
    pos = {"first-round": 0, "last-round": rp[-2] if len(rp) > 1 else 0, "first-core": nel, "last-core": len(order) - 1,
           "core-0": nel, "core-2": nel + 2, "core-last": len(order) - 1}
    pos.update({w: nel + k for w, k in DENSE_POS.items()})
    return order[pos[where]] + 1


@pytest.mark.parametrize("topo,path,where", PIVOT_CASES, ids=lambda v: str(v))
def test_late_pivot_failure_gives_a_zero_step(backend, oracle, ref, topo, path, where):
    """One pose without observations: its pivot is exactly zero in any order and every earlier
    pivot succeeds.  pivot <= 0 => dx = 0, poses untouched, the loop exits (as SimplicialLLT's
    failure in the reference, and the oracle); no error; and the next call is right again."""
    mode = "rays"
    g0 = ref.graph(topo, mode)
    _assert_plan(backend, g0, topo, path)
    pose = _pivot_pose(backend, g0, topo, path, where)
    g = ref.graph(topo, mode, ("unobserved", pose))
    T, dx, st = _call(backend, g, mode, path, iters=10, delta=1e-8)
    print(f"PIVOT {topo} {path} {where}: keyframe {pose} flags done {st['done']} fail {st['fail']}")
    assert np.all(dx == 0), np.abs(dx).max()
    assert np.array_equal(T, g.Twc.numpy())
    assert st["fail"] == 1 and st["done"] == 1, st  # (reported, and the zero step exited the loop)
    T_o, dx_o, it = _run_oracle(oracle, g, mode, 10, delta=1e-8)
    assert it == 1 and np.array_equal(T_o, g.Twc.numpy())
    # the flag was cleared: a healthy graph of the same shape through the same path
    _check_step(backend, oracle, ref, g0, mode, path, f"{topo}-after-pivot-failure", runs=1)


@pytest.mark.parametrize("path", PATHS)
def test_nan_passes_through_the_solver(backend, oracle, ref, path):
    """A NaN in an invalid point nothing reads poisons the system (the reference's 0 * NaN); NaN
    pivots pass the pivot <= 0 test, so the call returns a NaN step, not a zeroed one -- without
    error and without a timed-out wait.  Which entries are NaN depends on the elimination order."""
    topo, mode = "clique12", "rays"
    g = ref.graph(topo, mode, ("nan",))
    _assert_plan(backend, g, topo, path)
    T, dx, st = _call(backend, g, mode, path)  # (gn_check inside: no deferred timeout)
    print(f"NAN {path}: {int(np.isnan(dx).sum())} of {dx.size} entries NaN, flags {st['done']} {st['fail']}")
    assert np.isnan(dx).any() and not np.all(dx == 0)
    assert not st["fail"] and not st["done"], st  # (a NaN pivot is no failure; NaN < delta is false)
    _, dx_o, _ = _run_oracle(oracle, g, mode, 1)
    assert np.isnan(dx_o).any()
    _check_step(backend, oracle, ref, ref.graph(topo, mode), mode, path, f"{topo}-after-nan", runs=1)


# ---- 5. the early-exit compare at its threshold, in each copy of the retraction ----
def _ulps(x, k):
    x = np.float32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.float32(np.inf if k > 0 else 0))
    return float(x)


@pytest.mark.parametrize("path", ["dense-df", "s2-df", "s1", "s3", "s3-reg"])
@pytest.mark.parametrize("mode", sm.MODES)
def test_early_exit_compare_at_its_threshold(backend, oracle, ref, mode, path):
    """gn_retract_kernel (dense, s2) and gn_solve's retraction (s1, s3): delta_thresh two float32
    ulps above ||dx_1|| exits after iteration 1 (bitwise the one-iteration call), two below does
    not.  (Two ulps absorb the tree-versus-serial float64 sum; equality itself is not tested.)
    The oracle: its own ||dx_1|| differs from the op's by the accumulate's summation order (1e-7 ..
    4e-7 here, one to four ulps), so at the op's two deltas its iteration count is held to its own
    norm, and to the op's count wherever both norms lie on the same side; two ulps either side of
    its OWN norm it must count as the op does at the op's: 1 and 2; and 16 ulps above / below BOTH
    norms, clear of their distance, op and oracle must agree outright: 1 and 2."""
    topo = "clique12"
    g = ref.graph(topo, mode)
    _assert_plan(backend, g, topo, path)
    T1, dx1, st1 = _call(backend, g, mode, path)
    T2, dx2, _ = _call(backend, g, mode, path, iters=2)
    T3, _, _ = _call(backend, g, mode, path, iters=3)
    assert not st1["done"] and not np.array_equal(T2, T1) and not np.array_equal(T3, T2)
    nrm, nrm2 = float(sm.dx_norm_f32(dx1)), float(sm.dx_norm_f32(dx2))
    _, dx_o, _ = _run_oracle(oracle, g, mode, 1)
    nrm_o = float(sm.dx_norm_f32(dx_o))
    hi, lo = _ulps(nrm, 2), _ulps(nrm, -2)
    assert nrm2 < lo < nrm < hi
    T_hi, dx_hi, st_hi = _call(backend, g, mode, path, iters=3, delta=hi)
    assert st_hi["done"] == 1 and np.array_equal(T_hi, T1) and np.array_equal(dx_hi, dx1)
    T_lo, dx_lo, st_lo = _call(backend, g, mode, path, iters=3, delta=lo)
    # ||dx_2|| < lo: it exits after iteration 2
    assert st_lo["done"] == 1 and np.array_equal(T_lo, T2) and np.array_equal(dx_lo, dx2)
    assert not np.array_equal(T_lo, T1)
    for delta, it_op in ((hi, 1), (lo, 2)):
        _, _, it = _run_oracle(oracle, g, mode, 3, delta)
        print(f"EXIT {mode} {path}: ||dx_1|| {nrm!r} oracle's {nrm_o!r} delta {delta!r}: op {it_op} oracle {it}")
        assert it == (1 if nrm_o < delta else 2)
        if (nrm_o < delta) == (nrm < delta):
            assert it == it_op
    for delta, it_op in ((_ulps(nrm_o, 2), 1), (_ulps(nrm_o, -2), 2)):
        _, _, it = _run_oracle(oracle, g, mode, 3, delta)
        assert it == it_op, (it, it_op, nrm_o, delta)
    # the unconditional cross-check: 16 ulps clear of both norms
    for delta, it_op, T_k, dx_k in ((_ulps(max(nrm, nrm_o), 16), 1, T1, dx1), (_ulps(min(nrm, nrm_o), -16), 2, T2, dx2)):
        assert nrm2 < delta
        T_w, dx_w, st_w = _call(backend, g, mode, path, iters=3, delta=delta)
        assert st_w["done"] == 1 and np.array_equal(T_w, T_k) and np.array_equal(dx_w, dx_k)
        _, dx_ow, it = _run_oracle(oracle, g, mode, 3, delta)
        assert it == it_op, (it, it_op, nrm, nrm_o, delta)
