"""A host model of the direct Gauss-Newton solve: an extended-precision Cholesky solve of the dense
normal equations, what an honest float64 Cholesky can lose on them, the per-component bound the
GPU solvers are held to, and the graphs / fixtures tests/test_solve_model.py (CPU, the oracle's
systems) and tests/test_gpu_solve_exact.py (GPU) share.  Plain helpers, no test in here.

The GPU's direct solvers (chol_df.hip, the tile Cholesky of gn_kernels.hip, gn_sparse.hip,
gn_solve.hip) are float64 Choleskys of one matrix in different elimination orders, and the step
leaves them as dx = -(float)x.  So a solve is right when every component of dx is the float32
rounding of the exact solution, up to what a float64 Cholesky in another order may lose:
    |dx_i + x_ref_i| <= 0.5 ulp_f32(x_ref_i) + 4 max(E, n 2^-53) max|x_ref|
x_ref: solve_ld, a Cholesky in numpy.longdouble (64-bit mantissa);  E: e64, the largest distance
of a float64 Cholesky solve from x_ref over the natural order and random permutations of the pose
blocks;  4: the margin over the reference's own error for another summation order (the margin of
tests/test_gpu_pcg_solves.py).  Nothing in the bound comes from a kernel's output.
"""
import dataclasses

import numpy as np

from tests import pcg_model as pm

LD = np.longdouble
SEED = 3
HW_SHAPE = (24, 32)
MODES = ("rays", "calib", "points")


class PivotFailure(np.linalg.LinAlgError):
    pass


def _sym_lower(H, dtype):
    """The symmetric matrix whose lower triangle is H's (the solvers read the lower triangle)."""
    L = np.tril(np.asarray(H, dtype))
    return L + np.tril(L, -1).T


def solve_ld(H, b):
    """x = H^-1 b by a column Cholesky and the two substitutions in numpy.longdouble; raises
    PivotFailure when a pivot is not positive (a NaN pivot included)."""
    A = _sym_lower(H, LD)
    n = A.shape[0]
    L = np.zeros((n, n), LD)
    for j in range(n):
        row = L[j, :j]
        d = A[j, j] - row @ row
        if not d > 0:
            raise PivotFailure(f"pivot {j} of {n} is {d}")
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ row) / L[j, j]
    y = np.asarray(b, LD).copy()
    for j in range(n):  # L y = b
        y[j] /= L[j, j]
        y[j + 1:] -= L[j + 1:, j] * y[j]
    for j in range(n - 1, -1, -1):  # L' x = y
        y[j] /= L[j, j]
        y[:j] -= L[j, :j] * y[j]
    return y


def residual_ld(H, b, x):
    """max |H x - b| / (max|H| max|x| n), in longdouble."""
    A = _sym_lower(H, LD)
    r = A @ np.asarray(x, LD) - np.asarray(b, LD)
    return float(np.abs(r).max() / (np.abs(A).max() * np.abs(x).max() * A.shape[0]))


def _cho_solve64(A, b):
    try:
        from scipy.linalg import cho_solve
    except ImportError:  # two triangular solves by hand
        L = np.linalg.cholesky(A)
        y = np.array(b, np.float64)
        n = y.shape[0]
        for j in range(n):
            y[j] /= L[j, j]
            y[j + 1:] -= L[j + 1:, j] * y[j]
        for j in range(n - 1, -1, -1):
            y[j] /= L[j, j]
            y[:j] -= L[j, :j] * y[j]
        return y
    return cho_solve((np.linalg.cholesky(A), True), b)


def pose_orders(npose, nperm=7, seed=0):
    """The natural order and nperm random permutations of the pose blocks (a fixed seed)."""
    rng = np.random.default_rng(seed)
    return [np.arange(npose)] + [rng.permutation(npose) for _ in range(nperm)]


def e64(H, b, x_ref, nperm=7, seed=0):
    """How far an honest float64 Cholesky solve of (H, b) lands from x_ref: the largest
    max|x64 - x_ref| / max|x_ref| over the natural order and nperm random permutations of the 7x7
    pose blocks.  numpy.linalg.LinAlgError when some ordering's factorisation fails."""
    A = _sym_lower(H, np.float64)
    b = np.asarray(b, np.float64)
    n = b.shape[0]
    scale = float(np.abs(x_ref).max())
    worst = 0.0
    for order in pose_orders(n // 7, nperm, seed):
        p = (7 * order[:, None] + np.arange(7)[None, :]).ravel()
        x = np.empty(n)
        x[p] = _cho_solve64(A[np.ix_(p, p)], b[p])
        worst = max(worst, float(np.abs(x - np.asarray(x_ref, np.float64)).max() / scale))
    return worst


def ulp_f32(x):
    """The float32 spacing at every component of x."""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def bound(x_ref, E):
    """Per component: dx's float32 rounding (gn_retract_kernel: -(float)x) plus 4 times what a
    float64 Cholesky of this system loses (at least n 2^-53), relative to max|x_ref|."""
    x = np.asarray(x_ref, np.float64)
    return 0.5 * ulp_f32(x) + 4.0 * max(E, x.shape[0] * 2.0 ** -53) * np.abs(x).max()


def errors(dx, x_ref, E):
    """(err / bound, err in float32 ulps of the component), per component of dx [P, 7] or [n]."""
    x = np.asarray(x_ref, np.float64)
    err = np.abs(np.asarray(dx, np.float64).reshape(-1) + x)
    return err / bound(x, E), err / ulp_f32(x)


def old_criterion(dx, dx_other):
    """What the solver-against-solver tests ask of two solvers' float32 steps:
    max|dx - dx_other| <= 1e-8 max(max|dx_other|, 1e-6)."""
    return bool(np.abs(dx - dx_other).max() <= 1e-8 * max(np.abs(dx_other).max(), 1e-6))


def retracted(oracle, Twc, dx):
    """Pose 0 untouched, the oracle's retraction of dx on the rest."""
    return np.stack([Twc[0]] + [oracle.retr_sim3(dx[p - 1], Twc[p]) for p in range(1, Twc.shape[0])])


def dx_norm_f32(dx):
    """The retraction's ||dx|| as it compares it: float32(sqrt(sum of float64 squares))."""
    return np.float32(np.sqrt((np.asarray(dx, np.float64) ** 2).sum()))


# ---- the graphs, all at 24 x 32 (HW = 768) ----
def _clique(N):
    return [(a, b) for a in range(N) for b in range(a + 1, N)]


# name -> (N, undirected edges); "cfg3": synth's cfg3 (128 keyframes, 256 pairs, its own seed)
TOPOLOGIES = {
    "pair": (2, [(0, 1)]),                                       # one pose, 7 unknowns
    "star6": (6, [(0, k) for k in range(1, 6)]),                 # no fronts
    "chain24": (24, [(k - 1, k) for k in range(1, 24)]),         # rounds only (+ a 5-pose core)
    "hub23": (23, [(0, 1), (1, 2)] + [(h, k) for k in range(3, 23) for h in (1, 2)]),  # overflow lists
    "clique4": (4, _clique(4)),
    "clique12": (12, _clique(12)),
    "clique17": (17, _clique(17)),
    "clique21": (21, _clique(21)),
    "clique28": (28, _clique(28)),                               # 27 free poses: the largest in-register core
    "clique29": (29, _clique(29)),                               # 196 unknowns: 4 tile columns of 64
    "cfg3": (128, None),                                         # rounds plus core
}

# cfg3's weakly observed pose: keyframe 4 is the first pose of the first elimination round, keyframe
# 123 the last pose of the dense core, in every sparse plan (the tests check both against
# m3s_gn_plan_info).  keep = 3 and 8 there as on the cliques, but for ONE cell: the core pose in
# calib takes 5 instead of 3 -- its three neighbouring points do not hold it, the float32-summed
# system (the oracle's too: pivot 859 of 889 is negative) is no longer positive definite, a
# singular fixture instead of an ill-conditioned one.
CFG3_WEAK_POSE = {"round": 4, "core": 123}
CFG3_SINGULAR = ("core", "calib", 3)


def cfg3_keeps(where, mode):
    return (5, 8) if (where, mode) == CFG3_SINGULAR[:2] else (3, 8)


CFG3_CELLS = [(w, m, k) for w in ("round", "core") for m in MODES for k in cfg3_keeps(w, m)]

_graphs = {}


def graph(name, mode):
    """The graph `name` as `mode` takes it (calib: ray-constrained points); made once, shared --
    callers that change it take a copy (dataclasses.replace with cloned tensors)."""
    from m3s import synth

    if name not in _graphs:
        N, und = TOPOLOGIES[name]
        H, W = HW_SHAPE
        if und is None:
            _graphs[name] = synth.make_graph(name, H=H, W=W)
        else:
            _graphs[name] = synth.make_graph(dict(N=N, E=len(und)), H=H, W=W, seed=SEED, edges_only=und)
    if (name, mode) not in _graphs:
        _graphs[name, mode] = pm.for_mode(_graphs[name], mode)
    return _graphs[name, mode]


def with_poses(g, Twc):
    import torch

    return dataclasses.replace(g, Twc=torch.from_numpy(np.ascontiguousarray(Twc, np.float32)))


def touching(g, pose):
    """The directed edges with keyframe `pose` at either end (bool [2E])."""
    return ((g.ii == pose) | (g.jj == pose)).numpy()


def weakly_observed(g, keep, pose=None, Q_conf=1.5):
    """The ill-conditioned fixture: every edge touching `pose` (default: the last) invalid, except
    the first `keep` valid points (above Q_conf; neighbours in one pixel row, so the pose is held
    by nearly collinear points) of the first directed edge that starts at it."""
    pose = g.N - 1 if pose is None else pose
    valid = g.valid.clone()
    t = touching(g, pose)
    e = int(np.flatnonzero((g.ii == pose).numpy())[0])
    live = np.flatnonzero((g.valid[e, :, 0] & (g.Q[e, :, 0] > Q_conf)).numpy())[:keep]
    assert live.shape[0] == keep
    import torch

    valid[torch.from_numpy(t)] = False
    valid[e, torch.from_numpy(live), 0] = True
    return dataclasses.replace(g, valid=valid)


def unobserved(g, pose):
    """Exactly one pose without any observation: its diagonal block and couplings are zero, so its
    pivot fails in any elimination order and every earlier pivot succeeds."""
    import torch

    valid = g.valid.clone()
    valid[torch.from_numpy(touching(g, pose))] = False
    return dataclasses.replace(g, valid=valid)


def nan_in_an_unread_point(g):
    """One invalid point that no valid point reads gets a NaN coordinate (the recipe of
    test_compacted_stream_keeps_nan_poisoning_and_empty_edges): it still poisons the system like
    the reference's 0 * NaN."""
    e = min(3, g.ii.shape[0] - 1)
    j = int(g.jj[e])
    valid, Xs = g.valid.clone(), g.Xs.clone()
    valid[g.jj == j, 5] = False                          # every edge that reads it as Xj
    valid[(g.ii == j)[:, None] & (g.idx == 5)] = False   # no valid point gathers it as Xi
    Xs[j, 5, 0] = float("nan")
    return dataclasses.replace(g, valid=valid, Xs=Xs)


def oracle_system(oracle, g, mode, params):
    """(H, b) of one iteration at g.Twc as the CPU oracle builds them."""
    return oracle.gn_build_system(params(oracle, g, mode, 1), g.Twc.numpy(), g.Xs.numpy(), g.Cs.numpy(),
                                  g.ii.numpy(), g.jj.numpy(), g.idx.numpy(), g.valid.numpy(), g.Q.numpy())


# ---- deliberately wrong solves (float64), for the sensitivity tests ----
def _chol_right_looking(A, skip=None):
    """Right-looking Cholesky; skip = (column, block row, block column): that column's rank-1
    update of that 7x7 block of the trailing matrix is left out."""
    A = np.array(A, np.float64)
    n = A.shape[0]
    for j in range(n):
        A[j, j] = np.sqrt(A[j, j])
        A[j + 1:, j] /= A[j, j]
        col = A[j + 1:, j]
        upd = np.outer(col, col)
        if skip is not None and skip[0] == j:
            r0, c0 = 7 * skip[1] - (j + 1), 7 * skip[2] - (j + 1)
            assert r0 >= 0 and c0 >= 0
            upd[r0:r0 + 7, c0:c0 + 7] = 0.0
            upd[c0:c0 + 7, r0:r0 + 7] = 0.0
        A[j + 1:, j + 1:] -= upd
    return np.tril(A)


def _substitute(L, b, drop=None):
    """L L' x = b; drop = (row, column): that one term of the back-substitution is left out."""
    n = b.shape[0]
    y = np.array(b, np.float64)
    for j in range(n):
        y[j] /= L[j, j]
        y[j + 1:] -= L[j + 1:, j] * y[j]
    for i in range(n - 1, -1, -1):
        row = L[i + 1:, i] * y[i + 1:]
        if drop is not None and drop[0] == i:
            row[drop[1] - (i + 1)] = 0.0
        y[i] = (y[i] - row.sum()) / L[i, i]
    return y


def wrong_schur_f32(H, b):
    """The first half of the poses eliminated, the Schur complement rounded to float32 once."""
    A = _sym_lower(H, np.float64)
    b = np.asarray(b, np.float64)
    k = 7 * max(1, (b.shape[0] // 7) // 2)
    A11, A21, A22 = A[:k, :k], A[k:, :k], A[k:, k:]
    W = np.linalg.solve(A11, np.column_stack([A21.T, b[:k]]))
    S = (A22 - A21 @ W[:, :-1]).astype(np.float32).astype(np.float64)
    x2 = np.linalg.solve(S, b[k:] - A21 @ W[:, -1])
    x1 = np.linalg.solve(A11, b[:k] - A21.T @ x2)
    return np.concatenate([x1, x2])


def wrong_dropped_update(H, b):
    """Column 0's rank-1 update of the second pose's diagonal block dropped."""
    A = _sym_lower(H, np.float64)
    return _substitute(_chol_right_looking(A, skip=(0, 1, 1)), np.asarray(b, np.float64))


def wrong_dropped_back_term(H, b, x_ref, below):
    """The smallest-|x| pose moved to the front of the elimination order (nothing is substituted
    after it, so nothing propagates), and one term of its back-substitution dropped: the largest
    one that changes x by at most `below` (the smallest one when none is that small).  Returns
    (x, pose, change)."""
    A = _sym_lower(H, np.float64)
    b = np.asarray(b, np.float64)
    n = b.shape[0]
    P = n // 7
    pose = int(np.argmin(np.abs(np.asarray(x_ref, np.float64)).reshape(P, 7).max(axis=1)))
    order = np.array([pose] + [q for q in range(P) if q != pose])
    p = (7 * order[:, None] + np.arange(7)[None, :]).ravel()
    L = np.linalg.cholesky(A[np.ix_(p, p)])
    x_ok = _substitute(L, b[p])
    best = None
    for i in range(7):
        change = np.abs(L[i + 1:, i] * x_ok[i + 1:] / L[i, i])
        change[:6 - i] = 0.0  # (terms within the pose's own block feed its other rows: left alone)
        for c in np.flatnonzero(change > 0):
            cand = (i, i + 1 + int(c), float(change[c]))
            if best is None or (cand[2] > best[2]) == (cand[2] <= below) or (best[2] > below >= cand[2]):
                best = cand
    x = np.empty(n)
    x[p] = _substitute(L, b[p], drop=best[:2])
    return x, pose, best[2]
