"""The lagged-factor PCG (gn_pcg.hip: sp_inverse_kernel, pcg_kernel) held to a host CG model,
one solve at a time.

test_gpu_pcg.py compares poses after 10 iterations of nearly converged graphs, where dx ~ 1e-6
and a PCG step wrong by tens of percent passes, and a PCG that does not converge falls back to
the direct solve silently.  Here a call contains exactly ONE PCG solve, at an iteration where dx
is still 1e-3 .. 1e-1, and tests/pcg_model.py -- pcg_kernel's recurrence in numpy f64 on the dense
system m3s.debug.build_system_gpu assembles -- says what that solve must do: whether it converges,
in how many steps, and to what.

One case = (graph, mode, k, lag, onex) x M3S_SOLVER 2 (multi plan) / 3 (hybrid plan), every call
with M3S_GN_PCG=2, M3S_GN_DEBUG_FLAGS=2 and M3S_GN_PACK=2 (one accumulate path for every max_iter):
  reference: PCG off, max_iter = k -> Twc_k; PCG off, max_iter = k + 1 -> dx_direct, T_direct;
  tested:    M3S_PCG_FROM=k, M3S_PCG_LAG=lag, max_iter = k + 1: one PCG solve, at iteration k;
  model:     (H, b) at Twc_k and Twc_{k-lag} -> outcome_m, steps_m, x_m, e_m (f32 M; and f64 M).
Asserted: the plan (planned, from, lag, onex, rows per workgroup R, workgroups, item capacity as
choose_pcg derives them from n and the largest pose degree), pcg_runs == 1, and
  model converged:  no fallback, |steps - steps_m| <= 1, max|dx - dx_direct| <= 4 E max|dx_direct|
                    (E: the largest e_m of all converged model solves; 4: the other summation
                    order and dx's f32 rounding), Twc bitwise the oracle's retraction of dx;
  model gave up / broke down: one fallback, Twc and dx bitwise the PCG-off call's.
Where the f32-M and f64-M models disagree on the outcome the reference does not decide the row
(pcg_model.UNDECIDED): either model's answer is accepted, as a whole.

Both solvers plan a PCG for every graph here.  M3S_SOLVER=3 falls back to the multi plan where
the hybrid's core does not fit (n1540, n2303: the same plan as M3S_SOLVER=2 then).  The graph at
the cap is N = 330 with E = 1260, not the E = 1320 first listed: that one fits no workgroup shape
(pcg_model.GRAPHS), so no PCG is planned for it at all -- below the cap in n, it takes the direct
solve for a reason the unknown count alone does not show.

E measured on the first GPU run (MI355X): 1.751e-05, over 80 converged model solves (E_FIRST_RUN
below); it comes from the model on the GPU-built systems alone, never from the kernel's output.
On that run the kernel's step counts were the f32-M model's on every row, and its dx errors at
most 1.15 times their own row's e_m wherever e_m > 2e-7 (below that dx's f32 rounding, ~1e-7,
shows).  A second, sharper bound therefore holds each row to its own e_m: the kernel and the model
run one recurrence on one system and differ in M's last f32 bit and the summation order, so the
error left at the stop is the same to rounding; 2 max(e_m, e_m of the f64-M model) + 4 ulp of f32
(dx is f32; the direct solve's own error) bounds it with room.

The record of that run (the same figures under both solvers; dx err and e_m relative to max|dx|):
  case                            n  R nwg onex steps gpu / model (f32 M)           fallbacks  dx err / e_m
  pair-rays-k1-lag1               7 12   1 0    7 / converged 7                        0   0.00e+00 / 6.36e-12
  pair-rays-k2-lag1               7 12   1 0    5 / converged 5                        0   3.11e-07 / 2.70e-07
  pair-points-k1-lag1             7 12   1 0    5 / converged 5                        0   1.81e-07 / 1.87e-07
  pair-points-k2-lag1             7 12   1 0    2 / converged 2                        0   5.87e-07 / 6.09e-07
  pair-calib-k1-lag1              7 12   1 0    6 / converged 6                        0   2.24e-09 / 1.84e-09
  pair-calib-k2-lag1              7 12   1 0    4 / converged 4                        0   5.76e-07 / 5.31e-07
  star6-rays-k1-lag1             35 12   3 0   14 / gave_up 14                         1   0.00e+00 / -
  star6-points-k1-lag1           35 12   3 0    7 / converged 7                        0   9.70e-07 / 9.60e-07
  star6-calib-k1-lag1            35 12   3 0   17 / converged 17 / f64-M gave_up 13    0   5.13e-08 / 5.24e-08
  clique4-rays-k1-lag1           21 12   2 0   15 / converged 15                       0   7.91e-08 / 7.88e-08
  clique4-points-k1-lag1         21 12   2 0    8 / converged 8                        0   6.19e-07 / 5.93e-07
  clique4-calib-k1-lag1          21 12   2 0   14 / converged 14                       0   2.38e-08 / 2.24e-08
  clique12-rays-k1-lag1          77 12   7 0    9 / converged 9                        0   1.82e-06 / 1.82e-06
  clique12-rays-k2-lag2          77 12   7 0   11 / converged 11                       0   1.29e-06 / 1.29e-06
  clique12-points-k1-lag1        77 12   7 0    7 / converged 7                        0   5.42e-07 / 5.39e-07
  clique12-points-k2-lag2        77 12   7 0    7 / converged 7                        0   2.39e-07 / 2.52e-07
  clique12-calib-k1-lag1         77 12   7 0    9 / converged 9                        0   3.90e-07 / 3.90e-07
  clique12-calib-k2-lag2         77 12   7 0    9 / converged 9                        0   1.45e-07 / 1.45e-07
  clique28-rays-k1-lag1         189 12  16 0    7 / converged 7                        0   1.68e-06 / 1.62e-06
  clique28-rays-k2-lag2         189 12  16 0    9 / converged 9                        0   1.08e-06 / 1.09e-06
  clique28-points-k1-lag1       189 12  16 0    7 / converged 7                        0   5.14e-07 / 5.22e-07
  clique28-points-k2-lag2       189 12  16 0    7 / converged 7                        0   4.69e-07 / 4.71e-07
  clique28-calib-k1-lag1        189 12  16 0    8 / converged 8                        0   6.28e-07 / 6.64e-07
  clique28-calib-k2-lag2        189 12  16 0    8 / converged 8                        0   2.01e-07 / 1.94e-07
  hub23-rays-k2-lag1            154 12  13 0   12 / converged 12                       0   3.89e-06 / 3.89e-06
  hub23-rays-k3-lag2            154 12  13 0   17 / converged 17                       0   1.23e-06 / 3.86e-06
  hub23-points-k2-lag1          154 12  13 0    4 / converged 4                        0   1.10e-07 / 5.58e-08
  hub23-calib-k2-lag1           154 12  13 0    8 / converged 8                        0   1.54e-07 / 1.69e-07
  chain24-calib-k4-lag1         161 12  14 0    5 / converged 5                        0   1.26e-07 / 1.47e-07
  chain24-rays-k2-lag1          161 12  14 0    4 / gave_up 4                          1   0.00e+00 / -
  cfg2-rays-k3-lag1             224 12  19 0   17 / converged 17                       0   8.10e-07 / 8.07e-07
  cfg2-rays-k5-lag2             224 12  19 0   16 / converged 16                       0   6.69e-07 / 6.58e-07
  cfg2-points-k4-lag1           224 12  19 0    3 / converged 3                        0   8.59e-08 / 1.68e-08
  cfg2-calib-k4-lag1            224 12  19 0   22 / converged 22                       0   3.54e-07 / 3.51e-07
  n770-rays-k4-lag1             770 24  33 0   14 / converged 14                       0   4.12e-06 / 4.11e-06
  n1540-rays-k4-lag1           1540 12 129 0   13 / converged 13                       0   1.88e-06 / 1.89e-06
  n1540-rays-k5-lag2           1540 12 129 0   22 / converged 22                       0   5.53e-07 / 5.49e-07
  n2303-rays-k3-lag1           2303 12 192 0   16 / converged 16                       0   1.75e-05 / 1.75e-05
  clique12-rays-k1-lag1-onex     77 12   7 1    9 / converged 9                        0   1.59e-06 / 1.59e-06
  hub23-rays-k2-lag1-onex       154 12  13 1   12 / converged 12                       0   4.00e-06 / 3.80e-06
  cfg2-rays-k3-lag1-onex        224 12  19 1   19 / converged 19                       0   2.95e-06 / 2.95e-06
  n770-rays-k4-lag1-onex        770 12  65 1   15 / converged 15                       0   3.56e-06 / 3.55e-06
star6-calib-k1-lag1 is the undecided row: with the unpacked accumulate (M3S_GN_PACK unset) the
systems differ in the last bits, the two models answer as above, and the kernel gave up at 13 and
fell back -- with the f64-M model there, with the f32-M model here.
"""
import contextlib
import dataclasses
import os

import numpy as np
import pytest
import torch

from m3s import synth

from tests import pcg_model as pm
from tests.test_gpu_gn import LOCAL, _rel, _run_gpu, _run_oracle

pytestmark = pytest.mark.gpu

SOLVERS = ("2", "3")
HYBRID_CORE_TOO_LARGE = ("n1540", "n2303")  # M3S_SOLVER=3 takes the multi plan there
E_FIRST_RUN = 1.751e-05  # (a record: the bound uses the E fixture's value of the run itself)


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


def _call(backend, g, mode, iters, delta=0.0, **env):
    env.setdefault("M3S_GN_PCG", 2)
    # M3S_GN_PACK=2: the packed stream whatever max_iter is.  By default a call of fewer than 3
    # iterations accumulates unpacked, and calib's ray-constrained packed records round otherwise:
    # the 2-iteration call's Twc_2 would then not be, bit for bit, the state a 3-iteration call
    # solves iteration 2 from (1e-7 apart), and the retraction could not be checked bitwise
    env.setdefault("M3S_GN_PACK", 2)
    with _env(M3S_GN_DEBUG_FLAGS=2, **env):
        T, dx = _run_gpu(backend, g, mode, iters, delta)
        backend.gn_check()
        return T, dx, backend.gn_debug_flags()


class Reference:
    """Graphs, PCG-off runs, GPU-built systems and model solves, each made once."""

    def __init__(self, backend):
        self.backend = backend
        self._graphs, self._direct, self._sys, self._model = {}, {}, {}, {}

    def graph(self, name, mode):
        if name not in self._graphs:
            self._graphs[name] = pm.make_graph(name)
        if (name, mode) not in self._graphs:
            self._graphs[name, mode] = pm.for_mode(self._graphs[name], mode)
        return self._graphs[name, mode]

    def direct(self, name, mode, solver, iters, delta=0.0):
        """(Twc, dx) after `iters` iterations of the direct solve (PCG off)."""
        key = (name, mode, solver, iters, delta)
        if key not in self._direct:
            g = self.graph(name, mode)
            if iters == 0:
                self._direct[key] = (g.Twc.numpy().copy(), None)
            else:
                T, dx, st = _call(self.backend, g, mode, iters, delta, M3S_GN_PCG=0, M3S_SOLVER=solver)
                assert not st["pcg_planned"] and st["pcg_runs"] == 0 and st["pcg_R"] == 0, st
                self._direct[key] = (T, dx)
        return self._direct[key]

    def system(self, name, mode, Twc):
        """(H, b) as the GPU assembles them at Twc."""
        from m3s.debug import build_system_gpu

        key = (name, mode, Twc.tobytes())
        if key not in self._sys:
            g = dataclasses.replace(self.graph(name, mode), Twc=torch.from_numpy(np.ascontiguousarray(Twc)))
            self._sys[key] = build_system_gpu(g, mode, LOCAL)
        return self._sys[key]

    def model(self, case, solver):
        """The model's solve of the case: dict(s32, s64, e_m, decided)."""
        lag = pm.lag_for(case.k, case.lag)
        Tk = self.direct(case.graph, case.mode, solver, case.k)[0]
        Tl = self.direct(case.graph, case.mode, solver, case.k - lag)[0]
        key = (case, Tk.tobytes(), Tl.tobytes())
        if key not in self._model:
            H, b = self.system(case.graph, case.mode, Tk)
            Hl, _ = self.system(case.graph, case.mode, Tl)
            Minv = np.linalg.inv(Hl)
            s32 = pm.pcg(H, b, Minv.astype(np.float32).astype(np.float64), onex=bool(case.onex))
            s64 = pm.pcg(H, b, Minv, onex=bool(case.onex))
            e_m = pm.rel_err(s32.x, H, b) if s32.outcome == pm.CONVERGED else None
            e_m64 = pm.rel_err(s64.x, H, b) if s64.outcome == pm.CONVERGED else None
            self._model[key] = dict(s32=s32, s64=s64, e_m=e_m, e_m64=e_m64, decided=s32.outcome == s64.outcome)
        return self._model[key]


@pytest.fixture(scope="module")
def ref(backend):
    return Reference(backend)


@pytest.fixture(scope="module")
def E(ref):
    """The largest e_m (max |x_m - solve(H, b)| / max |solve(H, b)|) over all converged model
    solves of the case matrix, on the GPU-built systems."""
    e = []
    for case in pm.CASES:
        for solver in SOLVERS:
            m = ref.model(case, solver)
            print(f"MODEL {case.id} solver {solver}: f32-M {m['s32'].outcome} {m['s32'].steps}, "
                  f"f64-M {m['s64'].outcome} {m['s64'].steps}, e_m {m['e_m']}")
            if m["e_m"] is not None:
                e.append(m["e_m"])
    print(f"E = {max(e):.3e} over {len(e)} converged model solves")
    return max(e)


def _expected_plan(g, onex):
    n = 7 * (g.N - 1)
    return pm.expected_shape(n, pm.max_degree(g.ii, g.jj), onex)


def _assert_plan(st, g, case_k, lag, onex):
    R, nwg, ox, nitem = _expected_plan(g, onex)
    assert st["pcg_planned"] and st["pcg_from"] == case_k, st
    assert st["pcg_lag"] == pm.lag_for(case_k, lag) and st["pcg_onex"] == ox == int(bool(onex)), st
    assert (st["pcg_R"], st["pcg_nwg"], st["pcg_nitem"]) == (R, nwg, nitem), (st, R, nwg, nitem)


def _retracted(oracle, Twc, dx):
    return np.stack([Twc[0]] + [oracle.retr_sim3(dx[p - 1], Twc[p]) for p in range(1, Twc.shape[0])])


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("case", pm.CASES, ids=lambda c: c.id)
def test_one_pcg_solve_matches_the_host_model(backend, oracle, ref, E, case, solver):
    g = ref.graph(case.graph, case.mode)
    k = case.k
    with _env(M3S_SOLVER=solver):
        kind = backend.gn_plan_info(g.ii, g.jj, g.N)["solver"]
    assert kind == ("hybrid" if solver == "3" and case.graph not in HYBRID_CORE_TOO_LARGE else "multi"), kind
    Tk, _ = ref.direct(case.graph, case.mode, solver, k)
    T_d, dx_d = ref.direct(case.graph, case.mode, solver, k + 1)
    m = ref.model(case, solver)
    T_p, dx_p, st = _call(backend, g, case.mode, k + 1, M3S_SOLVER=solver, M3S_PCG_FROM=k, M3S_PCG_LAG=case.lag,
                          M3S_PCG_ONEX=case.onex)
    _assert_plan(st, g, k, case.lag, case.onex)
    assert st["pcg_runs"] == 1, st
    s32, s64 = m["s32"], m["s64"]
    err = float(np.abs(dx_p - dx_d).max() / np.abs(dx_d).max())
    print(f"ROW {case.id} solver {solver}: n {7 * (g.N - 1)} R {st['pcg_R']} nwg {st['pcg_nwg']} onex {st['pcg_onex']} "
          f"nitem {st['pcg_nitem']} | gpu steps {st['pcg_steps']} fallbacks {st['pcg_fallbacks']} | model f32-M "
          f"{s32.outcome} {s32.steps} f64-M {s64.outcome} {s64.steps} | dx err {err:.2e} e_m {m['e_m']} "
          f"bound {4 * E:.2e} max|dx| {np.abs(dx_d).max():.2e}" + ("" if m["decided"] else " UNDECIDED"))
    # the reference's answer: the f32-M model's; where the two roundings of M disagree on the
    # outcome, whichever the kernel sided with
    fell = st["pcg_fallbacks"] == 1
    s = s32
    if not m["decided"] and fell != (s32.outcome != pm.CONVERGED):
        s = s64
    if s.outcome == pm.CONVERGED:
        assert st["pcg_fallbacks"] == 0, (st, s.outcome, s.steps)
        assert abs(st["pcg_steps"] - s.steps) <= 1, (st, s.steps)
        assert np.isfinite(dx_p).all()
        assert err <= 4 * E, (err, 4 * E)
        own = 2 * max(e for e in (m["e_m"], m["e_m64"]) if e is not None) + 4 * 2.0 ** -23
        assert err <= own, (err, own)
        # the PCG's own retraction: the oracle's retraction of its dx, pose 0 untouched
        assert np.array_equal(T_p[0], Tk[0])
        assert np.array_equal(T_p, _retracted(oracle, Tk, dx_p)), _rel(T_p, _retracted(oracle, Tk, dx_p))
    else:
        assert st["pcg_fallbacks"] == 1, (st, s.outcome, s.steps)
        assert np.array_equal(T_p, T_d) and np.array_equal(dx_p, dx_d)


def test_the_fallback_case_falls_back_in_the_model(ref):
    """The listed fallback row is one on the GPU-built systems too (under both roundings of M):
    test_one_pcg_solve_matches_the_host_model then holds it to the bitwise direct result."""
    for solver in SOLVERS:
        m = ref.model(pm.FALLBACK_CASE, solver)
        assert m["s32"].outcome != pm.CONVERGED and m["s64"].outcome != pm.CONVERGED, m


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name", pm.ABOVE_CAP)
def test_above_the_cap_no_pcg_is_planned(backend, ref, name, solver):
    """n = 2310 > kPcgMaxN = 2304 (three vector entries per thread): no PCG, bitwise the PCG-off
    call -- for the graph as listed and for one whose workgroup shape would fit."""
    g = ref.graph(name, "rays")
    assert 7 * (g.N - 1) == 2310
    T_d, dx_d = ref.direct(name, "rays", solver, 4)
    T_p, dx_p, st = _call(backend, g, "rays", 4, M3S_SOLVER=solver, M3S_PCG_FROM=3, M3S_PCG_LAG=1)
    assert not st["pcg_planned"] and st["pcg_runs"] == 0, st
    assert (st["pcg_R"], st["pcg_nwg"], st["pcg_onex"], st["pcg_lag"], st["pcg_nitem"]) == (0, 0, 0, 0, 0), st
    assert np.array_equal(T_p, T_d) and np.array_equal(dx_p, dx_d)


def _policy(ref, name, mode, solver, iters, frm, lag):
    """The policy model (f32 M and f64 M) on the GPU-built systems along the direct trajectory."""
    g = ref.graph(name, mode)
    systems = pm.trajectory_systems(g, iters, lambda k: ref.direct(name, mode, solver, k)[0],
                                    lambda gk: ref.system(name, mode, gk.Twc.numpy()))
    return [pm.call_policy(systems, frm, lag, f32=f) for f in (True, False)]


def _assert_policy(st, pols):
    """fallbacks equal the policy model's count and the steps its total, within one per solve --
    for the f32-M model, or where the two roundings disagree, for either."""
    got = []
    for pol in pols:
        fb = sum(s.outcome != pm.CONVERGED for _, _, s in pol)
        total = sum(s.steps for _, _, s in pol)
        got.append((len(pol), fb, total))
        print("POLICY", [(k, m_it, s.outcome, s.steps) for k, m_it, s in pol])
    accept = got[:1] if got[0][:2] == got[1][:2] else got
    assert any(st["pcg_runs"] == r and st["pcg_fallbacks"] == fb and abs(st["pcg_steps"] - tot) <= r
               for r, fb, tot in accept), (st, got)


@pytest.mark.parametrize("solver", SOLVERS)
def test_m_is_refreshed_after_a_fallback(backend, ref, E, solver):
    """cfg2 topology, rays, PCG from iteration 2 with lag 1, 6 iterations: the model's first solve
    gives up (M from iteration 1), its factor refreshes M and the next converges with it.  Four
    PCG solves, the model's fallback count, its step total within one per solve.  Final poses:
    each converged solve moves dx by at most 4 E max|dx_k| (the per-solve bound), the retraction
    scales that by at most max(1, max|Twc|), and Gauss-Newton does not amplify it (it contracts
    towards the same minimum), so the poses differ by at most the sum over the PCG iterations."""
    name, mode, frm, iters = "cfg2", "rays", 2, 6
    g = ref.graph(name, mode)
    pols = _policy(ref, name, mode, solver, iters, frm, 1)
    assert sum(s.outcome != pm.CONVERGED for _, _, s in pols[0]) >= 1  # (a fallback to refresh after)
    T_d, _ = ref.direct(name, mode, solver, iters)
    T_p, dx_p, st = _call(backend, g, mode, iters, M3S_SOLVER=solver, M3S_PCG_FROM=frm, M3S_PCG_LAG=1)
    print("refresh", solver, st)
    _assert_plan(st, g, frm, 1, 0)
    assert st["pcg_runs"] == 4, st
    _assert_policy(st, pols)
    steps = sum(float(np.abs(ref.direct(name, mode, solver, k + 1)[1]).max()) for k in range(frm, iters))
    bound = 4 * E * steps * max(1.0, float(np.abs(T_d).max()))
    d = float(np.abs(T_p - T_d).max())
    print(f"refresh: max|T_pcg - T_direct| {d:.2e}, bound {bound:.2e}")
    assert np.isfinite(T_p).all() and d <= bound, (d, bound)


@pytest.mark.parametrize("solver", SOLVERS)
def test_early_exit_through_the_pcgs_own_retraction(backend, oracle, ref, solver):
    """clique28, calib, PCG from iteration 2 (default lag 2: M from a snapshot of iteration 0's
    factor): delta_thresh between |dx_1| and |dx_2| -- the PCG solve of iteration 2 is the first
    below it, its own retraction sets the early-exit flag, and the call's remaining iterations
    return at once: bitwise the 3-iteration PCG call."""
    name, mode = "clique28", "calib"
    g = ref.graph(name, mode)
    m = ref.model(pm.Case(name, mode, 2, 2), solver)
    assert m["s32"].outcome == pm.CONVERGED and m["decided"], m  # (the PCG's retraction is what runs)
    nrm = [float(np.sqrt((ref.direct(name, mode, solver, k + 1)[1].astype(np.float64) ** 2).sum())) for k in (0, 1, 2)]
    assert nrm[0] > nrm[1] > nrm[2] > 0, nrm
    delta = float(np.sqrt(nrm[1] * nrm[2]))
    T3, dx3, st3 = _call(backend, g, mode, 3, M3S_SOLVER=solver, M3S_PCG_FROM=2)
    assert st3["pcg_runs"] == 1 and st3["pcg_fallbacks"] == 0 and st3["pcg_lag"] == 2 and not st3["done"], st3
    T6, dx6, st6 = _call(backend, g, mode, 6, delta, M3S_SOLVER=solver, M3S_PCG_FROM=2)
    print("early exit", solver, nrm, delta, st6)
    assert st6["pcg_planned"] and st6["pcg_runs"] == 1 and st6["pcg_fallbacks"] == 0, st6
    assert st6["done"] == 1, st6
    assert np.array_equal(T6, T3) and np.array_equal(dx6, dx3)
    _, _, it = _run_oracle(oracle, g, mode, 6, delta)
    assert it == 3


def test_cfg2_full_size_ten_iterations_default_policy(backend, oracle):
    """cfg2 (33 keyframes, 64 pairs, 512x384, rays), 10 iterations, default environment: poses
    within 1e-5 of the oracle; the PCG is planned exactly when choose_pcg's rule says so for the
    plan m3s_gn_plan_info reports (the default plan here is the single-workgroup solve, whose
    factor the inverse does not read: none), and when it is, it runs 10 - from solves with the
    policy model's fallbacks."""
    g = synth.make_graph("cfg2")
    plan = backend.gn_plan_info(g.ii, g.jj, g.N)
    tiles = plan["core_unknowns_padded"] // 64
    frm = 3 if tiles >= 8 else 4
    planned = (plan["solver"] in ("hybrid", "multi") and tiles >= 1 and 7 * (g.N - 1) <= pm.PCG_MAX_N
               and _expected_plan(g, 0) is not None)
    with _env(M3S_GN_DEBUG_FLAGS=2):
        T_p, dx_p = _run_gpu(backend, g, "rays", 10)
        backend.gn_check()
        st = backend.gn_debug_flags()
    print("cfg2 full size:", plan["solver"], "tiles", tiles, st)
    assert bool(st["pcg_planned"]) == planned, (st, plan)
    if planned:
        from m3s.debug import build_system_gpu

        assert st["pcg_from"] == frm and st["pcg_runs"] == 10 - frm, st
        with _env(M3S_GN_PCG=0):
            Ts = [g.Twc.numpy()] + [_run_gpu(backend, g, "rays", k)[0] for k in range(1, 10)]
        systems = [build_system_gpu(dataclasses.replace(g, Twc=torch.from_numpy(T)), "rays", LOCAL) for T in Ts]
        _assert_policy(st, [pm.call_policy(systems, frm, 2, f32=f) for f in (True, False)])
    else:
        assert st["pcg_runs"] == 0 and st["pcg_fallbacks"] == 0, st
    T_o, _, it = _run_oracle(oracle, g, "rays", 10)
    d = _rel(T_p, T_o)
    print("cfg2 full size: pcg planned", planned, "fallbacks", st["pcg_fallbacks"], "vs oracle", d)
    assert it == 10 and np.isfinite(T_p).all() and d < 1e-5, d
