"""A host model (numpy f64) of the lagged-factor PCG: pcg_kernel's recurrence (gn_pcg.hip), the
driver's policy for M over one Gauss-Newton call (gn_driver.hip run()), the workgroup shape
choose_pcg derives, and the case list tests/test_pcg_model.py (CPU, the oracle's systems) and
tests/test_gpu_pcg_solves.py (GPU) share.  Plain helpers, no test in here.

The recurrence, as the kernel runs it:
    x = 0, r = b, z = M r, rho0 = rho = r'z (breakdown unless rho > 0 and finite), p = z
    step s = 1 .. kmax:
        q = A p;  p'q <= 0 or not finite -> breakdown (the step is not counted)
        alpha = rho / p'q;  x += alpha p;  r -= alpha q
        z = M r          (ONEX: z -= alpha (B p), B = float32(M A))
        rho1 = r'z; the step is counted; rho1 < 0 or not finite -> breakdown
        rho1 <= tol^2 rho0 -> converged
        s >= 4 and rho1 > rho0 exp(log(tol^2) s / kmax) -> gave up
        p = z + (rho1 / rho) p;  rho = rho1
    kmax steps without convergence -> gave up
M = float32(inv(H_lagged)): the kernel's is the f32 rounding of an f64 inverse through the
factor, the model's numpy's inverse rounded to f32.  Every outcome but "converged" is a fallback
to the direct solve.
"""
import dataclasses
import math

import numpy as np

KMAX = 30
TOL = 1e-6

CONVERGED, GAVE_UP, BREAKDOWN = "converged", "gave_up", "breakdown"


@dataclasses.dataclass
class Solve:
    outcome: str
    steps: int
    x: np.ndarray


def preconditioner(H_lagged, f32=True):
    """M = inv(H_lagged), rounded to f32 like sp_inverse_kernel's copy (f32=False: kept in f64)."""
    M = np.linalg.inv(np.asarray(H_lagged, np.float64))
    return M.astype(np.float32).astype(np.float64) if f32 else M


def pcg(A, b, M, onex=False, kmax=KMAX, tol=TOL):
    """pcg_kernel's recurrence on the dense system (A, b) with the preconditioner M (f64 array
    holding f32 values).  onex: the one-exchange variant (z updated through B = float32(M A))."""
    A = np.asarray(A, np.float64)
    b = np.asarray(b, np.float64)
    n = b.shape[0]
    tol2 = tol * tol
    B = (M @ A).astype(np.float32).astype(np.float64) if onex else None
    x = np.zeros(n)
    r = b.copy()
    with np.errstate(all="ignore"):
        z = M @ r
        rho = float(r @ z)
        rho0 = rho
        if not (rho > 0.0 and math.isfinite(rho)):
            return Solve(BREAKDOWN, 0, x)
        p = z.copy()
        steps = 0
        for s in range(1, kmax + 1):
            q = A @ p
            pq = float(p @ q)
            if not (pq > 0.0 and math.isfinite(pq)):
                return Solve(BREAKDOWN, steps, x)
            alpha = rho / pq
            x = x + alpha * p
            r = r - alpha * q
            z = z - alpha * (B @ p) if onex else M @ r
            rho1 = float(r @ z)
            steps = s
            if not (rho1 >= 0.0 and math.isfinite(rho1)):
                return Solve(BREAKDOWN, steps, x)
            if rho1 <= tol2 * rho0:
                return Solve(CONVERGED, steps, x)
            if s >= 4 and rho1 > rho0 * math.exp(math.log(tol2) * s / kmax):
                return Solve(GAVE_UP, steps, x)
            p = z + (rho1 / rho) * p
            rho = rho1
    return Solve(GAVE_UP, steps, x)


def rel_err(x, H, b):
    """e_m: max |x - solve(H, b)| / max |solve(H, b)|."""
    xd = np.linalg.solve(np.asarray(H, np.float64), np.asarray(b, np.float64))
    return float(np.abs(x - xd).max() / np.abs(xd).max())


def lag_for(frm, lag):
    """gn_plan.hip pcg_lag_for."""
    return max(1, min(frm, lag))


def call_policy(systems, frm, lag, onex=False, f32=True, kmax=KMAX, tol=TOL):
    """The driver's policy over one call of len(systems) iterations, systems[k] = (H_k, b_k) the
    system of iteration k: M from iteration frm - lag; iterations frm .. are PCG solves; after a
    solve that did not converge M is refreshed from that iteration's own factor; a converged
    solve keeps M.  Returns the list of (iteration, iteration of M, Solve)."""
    lag = lag_for(frm, lag)
    m_it = frm - lag
    M = preconditioner(systems[m_it][0], f32)
    out = []
    for k in range(frm, len(systems)):
        H, b = systems[k]
        s = pcg(H, b, M, onex=onex, kmax=kmax, tol=tol)
        out.append((k, m_it, s))
        if s.outcome != CONVERGED:
            m_it = k
            M = preconditioner(H, f32)
    return out


# ---- choose_pcg's workgroup shape (gn_plan.hip choose_pcg, gn_pcg.hip pcg_lds_bytes) ----
PCG_MAX_N = 2304            # kPcgMaxN
PCG_THREADS = 768           # kPcgThreads
PCG_MAX_LDS = 160 * 1024 - 1024
PCG_MAX_R_ONEX = 24         # kPcgMaxR
PCG_WG_CAP = 64             # M3S_PCG_WG's default


def max_degree(ii, jj):
    """1 + the most distinct non-pinned neighbours of a non-pinned pose (pose 0 is pinned; the
    keyframe ids are 0 .. N-1 here)."""
    nb = {}
    for a, b in zip(np.asarray(ii).tolist(), np.asarray(jj).tolist()):
        if a > 0 and b > 0 and a != b:
            nb.setdefault(a, set()).add(b)
            nb.setdefault(b, set()).add(a)
    return 1 + max((len(v) for v in nb.values()), default=0)


def lds_bytes(n, R, nitem, onex):
    nv = 256 if n < 256 else (n + 3) // 4 * 4
    r4 = (R + 1 + 3) // 4 * 4
    return 8 * (nv + 16 + 8 * nitem) + 4 * (2 * nitem + r4 + 4) + 4 * R * n * (2 if onex else 1)


def expected_shape(n, maxdeg, want_onex):
    """(R, nwg, onex, nitem) as choose_pcg picks them; None when no workgroup shape fits."""
    items = lambda R: 7 * maxdeg * (R // 7 + 2)

    def pick(ox):
        R = PCG_THREADS // 64
        fits = lambda r: lds_bytes(n, r, items(r), ox) <= PCG_MAX_LDS and (not ox or r <= PCG_MAX_R_ONEX)
        if -(-n // R) > PCG_WG_CAP and fits(2 * R):
            R *= 2
        return 0 if -(-n // R) > 240 or not fits(R) else R

    onex = bool(want_onex) and pick(True) > 0
    R = pick(onex)
    if R == 0:
        return None
    return R, -(-n // R), int(onex), items(R)


# ---- the case list ----
@dataclasses.dataclass(frozen=True)
class Case:
    graph: str
    mode: str
    k: int          # the iteration the one PCG solve replaces (M3S_PCG_FROM)
    lag: int        # M3S_PCG_LAG
    onex: int = 0   # M3S_PCG_ONEX

    @property
    def id(self):
        return f"{self.graph}-{self.mode}-k{self.k}-lag{self.lag}" + ("-onex" if self.onex else "")


def _clique(N):
    return [(a, b) for a in range(N) for b in range(a + 1, N)]


# graph name -> (N, undirected edges or the number of synth.make_edges edges, (H, W)); seed 3
GRAPHS = {
    "pair": (2, [(0, 1)], (24, 32)),
    "star6": (6, [(0, k) for k in range(1, 6)], (24, 32)),
    "clique4": (4, _clique(4), (24, 32)),
    "clique12": (12, _clique(12), (24, 32)),
    "clique28": (28, _clique(28), (24, 32)),
    "hub23": (23, [(0, 1), (1, 2)] + [(h, k) for k in range(3, 23) for h in (1, 2)], (24, 32)),
    "chain24": (24, [(k - 1, k) for k in range(1, 24)], (24, 32)),
    "cfg2": (33, 64, (24, 32)),
    "n770": (111, 444, (16, 24)),
    "n1540": (221, 884, (16, 24)),
    # the cap, kPcgMaxN = 2304.  With E = 1320 (seed 3) one pose has 24 non-pinned neighbours and
    # the items of 12 rows no longer fit the LDS beside M's rows (choose_pcg's pick() finds no R):
    # no PCG is planned (NO_FIT below).  E = 1260 is the largest edge count of the same sequence
    # at which one is (21 neighbours at most).
    "n2303": (330, 1260, (16, 24)),
    # above the cap: the graph as listed (which would not fit the LDS either), and one whose shape
    # fits, so that n > kPcgMaxN alone decides
    "n2310": (331, 1324, (16, 24)),
    "n2310fit": (331, 1150, (16, 24)),
}
NO_FIT = (330, 1320)
LARGE = ("n770", "n1540", "n2303", "n2310", "n2310fit")
SEED = 3
MODES3 = ("rays", "points", "calib")


def make_graph(name):
    from m3s import synth

    N, und, (H, W) = GRAPHS[name]
    if isinstance(und, int):
        return synth.make_graph(dict(N=N, E=und), H=H, W=W, seed=SEED)
    return synth.make_graph(dict(N=N, E=len(und)), H=H, W=W, seed=SEED, edges_only=und)


def for_mode(g, mode):
    """The graph as `mode` takes it (calib: points constrained to their pixel's ray); a copy."""
    if mode != "calib":
        return g
    from m3s.geometry import constrain_points_to_ray

    return dataclasses.replace(g, Xs=constrain_points_to_ray((g.H, g.W), g.Xs, g.K).contiguous())


def _cases():
    c = []
    c += [Case("pair", m, k, 1) for m in MODES3 for k in (1, 2)]
    c += [Case("star6", m, 1, 1) for m in MODES3]
    c += [Case("clique4", m, 1, 1) for m in MODES3]
    c += [Case("clique12", m, k, lag) for m in MODES3 for k, lag in ((1, 1), (2, 2))]
    c += [Case("clique28", m, k, lag) for m in MODES3 for k, lag in ((1, 1), (2, 2))]
    c += [Case("hub23", "rays", 2, 1), Case("hub23", "rays", 3, 2), Case("hub23", "points", 2, 1),
          Case("hub23", "calib", 2, 1)]
    c += [Case("chain24", "calib", 4, 1), Case("chain24", "rays", 2, 1)]  # (the second: a fallback case)
    c += [Case("cfg2", "rays", 3, 1), Case("cfg2", "rays", 5, 2), Case("cfg2", "points", 4, 1),
          Case("cfg2", "calib", 4, 1)]
    c += [Case("n770", "rays", 4, 1)]
    c += [Case("n1540", "rays", 4, 1), Case("n1540", "rays", 5, 2)]
    c += [Case("n2303", "rays", 3, 1)]
    # ONEX: the one-exchange variant, against the ONEX model
    c += [Case("clique12", "rays", 1, 1, 1), Case("hub23", "rays", 2, 1, 1), Case("cfg2", "rays", 3, 1, 1),
          Case("n770", "rays", 4, 1, 1)]
    return c


CASES = _cases()
# Rows whose outcome the reference does not decide: the f32-M and the f64-M model disagree.
#   star6-calib-k1-lag1 (M from iteration 0, cond(M A) = 320; the oracle's systems): both models'
#   r'z / r0'z0 run 13 % under the give-up schedule at step 11 (3.47e-5 against 3.98e-5), are equal
#   to 3 digits through step 11, then part: f32-M 1.58e-5 at step 13 (above the schedule's 6.3e-6:
#   gives up), f64-M 1.71e-6 (goes on and converges at step 17).  M's f32 rounding is a ~1e-3
#   relative change along its weak directions (cond(M) = 1.5e4), which a residual below 1e-3 sees.
# There the GPU test accepts either model's answer as a whole (outcome, steps, result); everywhere
# else the f32-M model's alone.
UNDECIDED = ("star6-calib-k1-lag1",)


def decided(s32, s64):
    """Rounding M to f32 changes neither the outcome nor the step count by more than one."""
    return s32.outcome == s64.outcome and abs(s32.steps - s64.steps) <= 1
# the row whose model gives up (the PCG runs and falls back); the row above the cap plans none
FALLBACK_CASE = Case("chain24", "rays", 2, 1)
ABOVE_CAP = ("n2310", "n2310fit")


def directed_edges(name_or_spec):
    """(ii, jj) of a graph of GRAPHS, or of an (N, E) synth.make_edges spec, without its images."""
    from m3s import synth

    N, und = GRAPHS[name_or_spec][:2] if isinstance(name_or_spec, str) else name_or_spec
    if isinstance(und, int):
        und = synth.make_edges(N, und, SEED)
    return [a for a, b in und] + [b for a, b in und], [b for a, b in und] + [a for a, b in und]


def trajectory_systems(g, iters, poses_after, build):
    """systems[k], k = 0 .. iters-1, along the direct solve's trajectory: poses_after(k) -> Twc
    [N, 8] (numpy) after k direct iterations, build(graph) -> (H, b) at the graph's Twc."""
    import torch

    return [build(dataclasses.replace(g, Twc=torch.from_numpy(np.ascontiguousarray(poses_after(k)))) if k else g)
            for k in range(iters)]


def solve_case(sys_k, sys_lagged, onex=False, f32=True):
    """One case's model solve: the system of iteration k, M from the lagged iteration's."""
    return pcg(sys_k[0], sys_k[1], preconditioner(sys_lagged[0], f32), onex=onex)
