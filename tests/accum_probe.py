"""Helpers of the accumulate probes (tests/test_accum_probe_host.py, tests/test_gpu_accum_probe.py).

An IMPULSE call leaves exactly one valid point on one directed edge of every pair of a set of
DISJOINT keyframe pairs and nothing else, so every non-zero 7x7 block of the dense normal equations
(m3s.debug: m3s_gn_build_system) is ONE point's contribution from ONE known directed edge: no
summation, and a lost, duplicated or mis-gathered point moves a block by all of itself.  The
expected blocks are the oracle's (oracle.gn_align under exact_sums) on the live edges alone.

Everything here that decides where a point goes or which class it falls in asks the oracle
(gn_residuals), never the GPU.  No tests in this file.
"""
from __future__ import annotations

import contextlib
import ctypes
import functools
import os
import types

import numpy as np
import torch

from m3s import synth

LOCAL = dict(sigma_ray=0.003, sigma_dist=10.0, sigma_pixel=1.0, sigma_depth=10.0, sigma_point=0.05,
             C_conf=0.0, Q_conf=1.5, pixel_border=-10, depth_eps=1e-6)
# the class calls: a confidence threshold inside the confidences' range and a border inside the
# image, so that natural points fall on both sides of each
LOCAL_CLASS = dict(LOCAL, C_conf=1.5, pixel_border=3)

HUBER_K = 1.345
# points of one workgroup step (gn_accum.hip: kAccThreads = 256 lanes x acc_np() points: calib 4,
# rays and points 2)
STEP = {"calib": 1024, "rays": 512, "points": 512}

# the accumulate paths and the switches that select them (gn_driver.hip setup(): M3S_GN_PACK,
# M3S_GN_COMPACT, M3S_GN_RAYCHECK; gn_enqueue.hip enqueue_accumulate(): M3S_GN_FUSE_REDUCE).
# m3s_gn_build_system (gn_api.hip) runs setup() without the early pack, then prepare_iterations()
# -- the separate pack pass -- and enqueue_system(): the unpacked kernel, or the record-reading
# packed kernel of the selected stream.
PATHS = {
    "unpacked": {"M3S_GN_PACK": "0"},
    "packed": {"M3S_GN_PACK": "2", "M3S_GN_COMPACT": "0", "M3S_GN_RAYCHECK": "0"},
    "compact": {"M3S_GN_PACK": "2", "M3S_GN_COMPACT": "1"},
    "raycheck": {"M3S_GN_PACK": "2", "M3S_GN_COMPACT": "0", "M3S_GN_RAYCHECK": "1"},
    "unfused": {"M3S_GN_PACK": "2", "M3S_GN_COMPACT": "0", "M3S_GN_FUSE_REDUCE": "0"},
}
_SWITCHES = sorted({k for env in PATHS.values() for k in env})


def paths_for(H, W, mode, on_rays):
    """The paths that exist at this shape: the packed streams need HW % 4 == 0 (gn_driver.hip:
    c.vec), the ray-constrained one calib points on their rays and W % 4 == 0 (gn_accum.hip).
    At other shapes the switches fall back to the unpacked kernel, which is run once."""
    if (H * W) % 4:
        return ["unpacked"]
    out = ["unpacked", "packed", "compact", "unfused"]
    if mode == "calib" and on_rays and W % 4 == 0:
        out.insert(3, "raycheck")
    return out


@contextlib.contextmanager
def path_env(path):
    """The path's switches set, every other path switch unset."""
    old = {k: os.environ.get(k) for k in _SWITCHES}
    for k in _SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(PATHS[path])
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ------------------------------------------------------------------------------------------
# the planner's chunking, restated (gn_plan.hip: chunk_target(), choose_nchunks(), chunk_points())
# ------------------------------------------------------------------------------------------
CHUNK_TARGET = 16384  # chunk_target() without M3S_ACC_CHUNK


def _align_up(x, a):
    return (x + a - 1) // a * a


def choose_nchunks(HW, E):
    nc = (HW + CHUNK_TARGET - 1) // CHUNK_TARGET
    want = (4096 + max(E, 1) - 1) // max(E, 1)
    nc = max(nc, want)
    max_nc = max(1, (HW + 1023) // 1024)
    nc = min(max(nc, 1), max_nc)
    chunk = _align_up((HW + nc - 1) // nc, 4)
    return max((HW + chunk - 1) // chunk, 1)


def chunk_points(HW, nchunks):
    return _align_up((HW + nchunks - 1) // nchunks, 4)


def chunk_starts(HW, E):
    nc = choose_nchunks(HW, E)
    c = chunk_points(HW, nc)
    return [k for k in range(0, HW, c)], c


def live_positions(HW, mode, E):
    """Where a kernel's loop structure changes, modulo HW, without duplicates: the first lanes, wave
    and 16-B group ends, the step ends S (from the image's and from every chunk's first point), the
    chunk boundaries, the last points."""
    S = STEP[mode]
    starts, chunk = chunk_starts(HW, E)
    last_full = HW // S * S
    raw = [0, 1, 3, 4, 63, 64, 255, 256, S - 1, S, 2 * S - 1, 2 * S, last_full - 1, last_full]
    for k0 in starts:
        raw += [k0 - 1, k0]
        k1 = min(k0 + chunk, HW)
        for s in range(k0 + S, k1, S):
            raw += [s - 1, s]
        raw += [k0 + (k1 - k0) // S * S - 1, k0 + (k1 - k0) // S * S]  # the chunk's last full step
    raw += list(range(HW - 5, HW))
    out = []
    for k in raw:
        k %= HW
        if k not in out:
            out.append(k)
    return out


def corner_indices(H, W):
    HW = H * W
    return [0, W - 1, W, HW - W, HW - 1]


# ------------------------------------------------------------------------------------------
# graphs
# ------------------------------------------------------------------------------------------
def probe_graph(H, W, mode, npairs, E_directed=None, seed=21, off_rays=False):
    """A chain of N = 2 npairs + 2 keyframes (m3s.synth.make_graph on the chain's pairs), its pairs
    duplicated cyclically up to E_directed // 2 undirected edges (None: the chain alone).  The
    directed edge list is the op's two-way layout (all forward edges, then all backward ones);
    `src[e]` is the row of directed edge e in the chain graph's idx / valid / Q (duplicates of a
    pair share its matches).  calib points are constrained to their rays as solve_GN_calib's are;
    off_rays moves them off (the positional stream)."""
    N = 2 * npairs + 2
    chain = [(k, k + 1) for k in range(N - 1)]
    nund = len(chain) if E_directed is None else E_directed // 2
    assert nund >= len(chain)
    und = [chain[u % len(chain)] for u in range(nund)]
    g = synth.make_graph(dict(N=N, E=len(chain)), H=H, W=W, seed=seed, edges_only=chain)
    Xs = g.Xs
    if mode == "calib":
        Xs = _constrain(H, W, Xs, g.K)
        if off_rays:
            Xs = (Xs * 1.0001).contiguous()
    p = types.SimpleNamespace()
    p.H, p.W, p.HW, p.N, p.npairs, p.mode, p.on_rays = H, W, H * W, N, npairs, mode, mode == "calib" and not off_rays
    p.off_rays = off_rays
    p.K = g.K.numpy().copy()
    p.Twc = g.Twc.numpy().copy()
    p.Xs = Xs.numpy().copy()
    p.Cs = g.Cs.numpy().copy()
    p.cidx, p.cvalid, p.cQ = g.idx.numpy(), g.valid.numpy()[..., 0], g.Q.numpy()[..., 0]
    p.und = und
    p.ii = np.array([a for a, b in und] + [b for a, b in und], np.int64)
    p.jj = np.array([b for a, b in und] + [a for a, b in und], np.int64)
    nch = len(chain)
    p.src = np.array([u % nch for u in range(nund)] + [nch + u % nch for u in range(nund)], np.int64)
    p.E = len(p.ii)
    return p


def _constrain(H, W, Xs, K):
    from m3s.geometry import constrain_points_to_ray

    return constrain_points_to_ray((H, W), Xs, K).contiguous()


def oracle_params(oracle, p, L):
    if p.mode == "rays":
        return oracle.make_params("rays", L["sigma_ray"], L["sigma_dist"], L["C_conf"], L["Q_conf"], max_iter=1)
    if p.mode == "points":
        return oracle.make_params("points", L["sigma_point"], 0.0, L["C_conf"], L["Q_conf"], max_iter=1)
    return oracle.make_params("calib", L["sigma_pixel"], L["sigma_depth"], L["C_conf"], L["Q_conf"], K=p.K,
                              height=p.H, width=p.W, pixel_border=L["pixel_border"], z_eps=L["depth_eps"],
                              max_iter=1)


def sigmas_inv(mode, L):
    """1/sigma of each residual row as the reference forms it (float of a double quotient)."""
    if mode == "rays":
        a, b = np.float32(1.0 / L["sigma_ray"]), np.float32(1.0 / L["sigma_dist"])
        return [a, a, a, b]
    if mode == "calib":
        a, b = np.float32(1.0 / L["sigma_pixel"]), np.float32(1.0 / L["sigma_depth"])
        return [a, a, b]
    a = np.float32(1.0 / L["sigma_point"])
    return [a, a, a]


# ------------------------------------------------------------------------------------------
# calls
# ------------------------------------------------------------------------------------------
def pair_edges(p, parity, direction, live_at="first"):
    """[(pair, directed edge)] of one impulse call: parity 1 = the odd pairs (2m-1, 2m), 0 = the
    even pairs (2m, 2m+1) including (0, 1); direction 0 = forward (ii < jj), 1 = backward; live_at
    picks the pair's first, a middle or its last duplicate in the edge list."""
    nund, nch = len(p.und), p.N - 1
    out = []
    for c in range(parity, nch, 2):  # chain pair c = (c, c + 1)
        dups = list(range(c, nund, nch))
        u = {"first": dups[0], "middle": dups[len(dups) // 2], "last": dups[-1]}[live_at]
        out.append((c, u + direction * nund))
    return out


def _residuals(oracle, p, L, Xs, Cs, edges, idx_rows, valid_rows, Q_rows):
    P = oracle_params(oracle, p, L)
    return oracle.gn_residuals(P, p.Twc, Xs, Cs, p.ii[edges], p.jj[edges], idx_rows, valid_rows, Q_rows)


def _single(HW, k, v, dtype, fill=0):
    r = np.full((HW,), fill, dtype)
    r[k] = v
    return r


def make_call(oracle, p, L, live, Xs=None, Cs=None, name=""):
    """A call from its live points: `live` = [dict(e=, k=, idx=, Q=, valid=True, cls=, want=)].
    Every other point of every edge is unmatched.  The oracle's verdict on each live point
    (residuals, weights, validity) is attached."""
    c = types.SimpleNamespace(p=p, L=L, name=name, live=live)
    c.Xs = p.Xs if Xs is None else Xs
    c.Cs = p.Cs if Cs is None else Cs
    n, HW = len(live), p.HW
    c.edges = np.array([l["e"] for l in live], np.int64)
    c.idx_rows = np.zeros((n, HW), np.int64)
    c.valid_rows = np.zeros((n, HW), bool)
    c.Q_rows = np.full((n, HW), 2.0, np.float32)
    for r, l in enumerate(live):
        c.idx_rows[r, l["k"]] = l["idx"]
        c.valid_rows[r, l["k"]] = l.get("valid", True)
        c.Q_rows[r, l["k"]] = l["Q"]
    X, err, w, vo = _residuals(oracle, p, L, c.Xs, c.Cs, c.edges, c.idx_rows, c.valid_rows, c.Q_rows)
    for r, l in enumerate(live):
        k = l["k"]
        l.update(X=X[r, k], err=err[r, k], w=w[r, k], ovalid=bool(vo[r, k]))
        assert not vo[r, np.arange(HW) != k].any()
    return c


def tolerance(c):
    """(tol_H, tol_b) per block: max(1e-4, 64 S), S the block's convention spread."""
    return np.maximum(1e-4, 64.0 * c.S_H), np.maximum(1e-4, 64.0 * c.S_b)


def attach_expected(oracle, c, rounding=True):
    """The call's exactly summed oracle system (Hx, bx), its blocks' convention spread S and their
    input-rounding spread R: how far the oracle's own block moves when every coordinate of Xs is
    rounded one f32 ulp up or down -- what two correct f32 evaluations of T_ij Xj may differ by."""
    if not hasattr(c, "S_H"):
        c.S_H, c.S_b, (c.Hx, c.bx) = convention_spread(oracle, c)
    if not rounding:
        return c
    Xs0 = c.Xs
    sys = [(c.Hx, c.bx)]
    try:
        for d in (np.inf, -np.inf):
            c.Xs = np.nextafter(Xs0, np.float32(d)).astype(np.float32)
            sys.append(expected(oracle, c))
    finally:
        c.Xs = Xs0
    c.R_H, c.R_b = (_block_spread([s[q] for s in sys]) for q in (0, 1))
    return c


def _block_spread(sys):
    """per block: the element-wise max - min over the systems, over the first one's largest entry"""
    A = np.stack(sys)
    Rb, Sb = blocks(sys[0]), blocks(A.max(0) - A.min(0))
    ax = tuple(range(Rb.ndim - (2 if sys[0].ndim == 2 else 1), Rb.ndim))
    with np.errstate(invalid="ignore", divide="ignore"):
        s = Sb.max(axis=ax) / np.abs(Rb).max(axis=ax)
    return np.where(np.isfinite(s), s, 0.0)


RESOLVE = 4.0  # the tolerance must cover this many one-ulp input roundings


def unresolved_blocks(c):
    """The pose blocks (0-based poses) whose input-rounding spread exceeds tol / RESOLVE: no f32
    kernel can be held to tol there, whatever it computes."""
    tH, tb = tolerance(c)
    return {int(x) for x in np.argwhere(RESOLVE * c.R_H > tH).ravel()} | \
        {int(x) for x in np.flatnonzero(RESOLVE * c.R_b > tb)}


def unresolved_points(c):
    bad = unresolved_blocks(c)
    return [l for l in c.live if bad & {int(c.p.ii[l["e"]]) - 1, int(c.p.jj[l["e"]]) - 1}]


def impulse_calls(oracle, p, live_at="first", rounds=None, offset=0):
    """The impulse calls of a graph: per round the four (parity, direction) calls, the positions of
    live_positions() dealt over the pairs, as many rounds as it takes to place every position once
    in each direction.  A point the oracle finds invalid at its position is made valid: Q = 4, a
    match at an image corner (corner_indices: the pixel decode's extremes), and -- should its
    projection still fall outside (calib) -- a random depth on its ray / a random finite point.  A
    valid point that f32 cannot resolve to the tolerance (unresolved_points) is matched to a corner
    too: its residual is then many pixels / centimetres, not a near-cancellation."""
    pos = live_positions(p.HW, p.mode, p.E)
    corners = corner_indices(p.H, p.W)
    rng = np.random.default_rng(1234 + p.HW)
    Xs = p.Xs.copy()
    per_call = p.npairs  # the odd calls' pair count (the even ones have one more)
    nrounds = -(-len(pos) // per_call) if rounds is None else rounds
    plans = []
    for rd in range(nrounds):
        for direction in (0, 1):
            for parity in (1, 0):
                live = []
                for m, (cp, e) in enumerate(pair_edges(p, parity, direction, live_at)):
                    k = pos[(offset + rd * per_call + m + 3 * direction) % len(pos)]
                    s = p.src[e]
                    live.append(dict(e=e, k=k, idx=int(p.cidx[s, k]) if p.cvalid[s, k] else 0,
                                     Q=float(p.cQ[s, k]), valid=bool(p.cvalid[s, k]), cls="position", want=True))
                plans.append((f"r{rd}-{'odd' if parity else 'even'}-{'fwd' if direction == 0 else 'bwd'}", live))
    # make every live point valid, by the oracle's verdict (two passes: the cheap fix, then a new Xj)
    for attempt in range(3):
        todo = 0
        for name, live in plans:
            c = make_call(oracle, p, LOCAL, live, Xs=Xs, name=name)
            for l in c.live:
                if l["ovalid"]:
                    continue
                todo += 1
                if attempt == 0:
                    l.update(valid=True, Q=4.0, idx=corners[(l["k"] + l["e"]) % len(corners)])
                else:
                    j = int(p.jj[l["e"]])
                    Xs[j, l["k"]] = _random_point(p, l["k"], rng)
        if todo == 0:
            break
    calls = [attach_expected(oracle, make_call(oracle, p, LOCAL, live, Xs=Xs, name=name), rounding=False)
             for name, live in plans]
    if max(max(c.S_H.max(), c.S_b.max()) for c in calls) > FLOOR_MAX:
        return calls  # (unusable: calls_of takes the next seed)
    for c in calls:
        attach_expected(oracle, c)
    # ... and resolvable: a point whose blocks a one-ulp rounding of the inputs moves by more than a
    # quarter of the tolerance (a residual that nearly cancels) gets a corner match as well
    for attempt in range(1, 4):
        redo = False
        for n, c in enumerate(calls):
            for l in unresolved_points(c):
                l["idx"] = corners[(l["k"] + l["e"] + attempt) % len(corners)]
                l["rematched"] = True
                redo = True
                calls[n] = None
        if not redo:
            break
        calls = [c if c is not None else attach_expected(oracle, make_call(oracle, p, LOCAL, plans[n][1], Xs=Xs,
                                                                            name=plans[n][0]))
                 for n, c in enumerate(calls)]
    return calls


def _random_point(p, k, rng):
    z = np.float32(rng.uniform(2.0, 4.0))
    if p.mode == "calib":  # on its pixel's ray, as constrain_points_to_ray forms it
        u, v = np.float32(k % p.W), np.float32(k // p.W)
        fx, fy, cx, cy = (np.float32(t) for t in (p.K[0, 0], p.K[1, 1], p.K[0, 2], p.K[1, 2]))
        x = np.array([z * ((u - cx) / fx), z * ((v - cy) / fy), z], np.float32)
        return x * np.float32(1.0001) if p.off_rays else x
    return np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), z], np.float32)


# ------------------------------------------------------------------------------------------
# validity and weight classes
# ------------------------------------------------------------------------------------------
def huber_r(p, L, l):
    """sqrt(w) * err per residual row of a live point, as the reference forms it."""
    sq = np.sqrt(np.float32(l["Q"]))
    return np.array([np.float32(s * sq) * np.float32(e) for s, e in zip(sigmas_inv(p.mode, L), l["err"])], np.float64)


def pixel_uv(l):
    """calib: the projection (u, v) the oracle tested, from its pixel residuals and the target."""
    return float(l["err"][0]) + float(l["idx"] % l["W"]), float(l["err"][1]) + float(l["idx"] // l["W"])


def class_names(mode):
    rows = 4 if mode == "rays" else 3
    names = ["unmatched", "q_eq", "q_above", "ci_eq", "cj_eq", "ci_nan", "cj_nan"]
    if mode == "calib":
        names += ["zi_eq", "zi_above", "zt_neg", "left", "right", "top", "bottom", "inside"]
    for r in range(rows):
        names += [f"huber{r}_off", f"huber{r}_on"]
    return names


def class_verdict(p, L, l):
    """The class the ORACLE puts a live point in, as (name matches, valid) checks: returns the set
    of class names whose defining condition holds for this point."""
    out = set()
    valid = l["ovalid"]
    rows = 4 if p.mode == "rays" else 3
    if not l.get("valid", True):
        out.add("unmatched")
    Qt = np.float32(L["Q_conf"])
    if np.float32(l["Q"]) == Qt and not valid:
        out.add("q_eq")
    if np.float32(l["Q"]) == np.nextafter(Qt, np.float32(np.inf)) and valid:
        out.add("q_above")
    ci, cj = l["ci"], l["cj"]
    Ct = np.float32(L["C_conf"])
    if ci == Ct and not valid:
        out.add("ci_eq")
    if cj == Ct and not valid:
        out.add("cj_eq")
    if np.isnan(ci) and not valid:
        out.add("ci_nan")
    if np.isnan(cj) and not valid:
        out.add("cj_nan")
    if p.mode == "calib":
        ze = np.float32(L["depth_eps"])
        if l["zi"] == ze and not valid:
            out.add("zi_eq")
        if l["zi"] == np.nextafter(ze, np.float32(np.inf)) and valid:
            out.add("zi_above")
        if l["X"][2] <= ze and not valid:
            out.add("zt_neg")
        if l["X"][2] > ze and l["zi"] > ze:
            u, v = pixel_uv(l)
            lo, hu, hv = float(L["pixel_border"]), float(p.W - 1 - L["pixel_border"]), float(p.H - 1 - L["pixel_border"])
            m = 1e-3  # px from a border: the kernels' transforms differ from the oracle's by ulps
            in_u, in_v = lo + m <= u <= hu - m, lo + m <= v <= hv - m
            if u <= lo - m and in_v and not valid:
                out.add("left")
            if u >= hu + m and in_v and not valid:
                out.add("right")
            if v <= lo - m and in_u and not valid:
                out.add("top")
            if v >= hv + m and in_u and not valid:
                out.add("bottom")
            if in_u and in_v and valid:
                out.add("inside")
    if valid:
        r = np.abs(huber_r(p, L, l))
        for q in range(rows):
            if r[q] <= HUBER_K * (1 - 1e-3):
                out.add(f"huber{q}_off")
            if r[q] >= HUBER_K * (1 + 1e-3):
                out.add(f"huber{q}_on")
    return out


def _annotate(c):
    p = c.p
    for l in c.live:
        i, j = int(p.ii[l["e"]]), int(p.jj[l["e"]])
        ind = l["idx"] if l.get("valid", True) else 0
        l.update(W=p.W, ci=c.Cs[i, ind, 0], cj=c.Cs[j, l["k"], 0], zi=c.Xs[i, ind, 2])
        l["classes"] = class_verdict(p, c.L, l)
    return c


def class_calls(oracle, p):
    """Calls whose single live points sit in every class of class_names(mode).  Natural classes (a
    projection outside a border, a Huber row on or off) are FOUND among the graph's own matches by
    the oracle's residuals under LOCAL_CLASS; the others are made from a naturally valid point by
    setting the one input the class is about.  One class per pair, dealt over the four (parity,
    direction) calls; each call's points are then classified again by the oracle (`classes`)."""
    L = LOCAL_CLASS
    HW = p.HW
    Cs0 = np.maximum(p.Cs, np.float32(1.6))  # every confidence passes unless a class says otherwise
    # the oracle's verdict on every natural match of the chain's directed edges
    edges = np.array([pe[1] for par in (1, 0) for d in (0, 1) for pe in pair_edges(p, par, d)], np.int64)
    src = p.src[edges]
    X, err, w, vo = _residuals(oracle, p, L, p.Xs, Cs0, edges, p.cidx[src], p.cvalid[src], p.cQ[src])
    slots = list(edges)
    row_of = {int(e): r for r, e in enumerate(edges)}
    names = class_names(p.mode)
    Xs, Cs = p.Xs.copy(), Cs0.copy()
    lives = {}

    # the natural classes of every match, vectorised (class_verdict() re-checks the chosen points)
    matched, nidx, nQ = p.cvalid[src], p.cidx[src], p.cQ[src]
    sq = np.sqrt(nQ.astype(np.float32))
    mask = {None: vo & matched}
    for q, s in enumerate(sigmas_inv(p.mode, L)):
        r = np.abs((s * sq).astype(np.float32) * err[..., q]).astype(np.float64)
        mask[f"huber{q}_off"] = vo & matched & (r <= HUBER_K * (1 - 1e-3))
        mask[f"huber{q}_on"] = vo & matched & (r >= HUBER_K * (1 + 1e-3))
    if p.mode == "calib":
        u = err[..., 0].astype(np.float64) + nidx % p.W
        v = err[..., 1].astype(np.float64) + nidx // p.W
        zi = p.Xs[p.ii[edges][:, None], nidx, 2]
        pre = matched & (nQ > np.float32(L["Q_conf"])) & (X[..., 2] > np.float32(L["depth_eps"])) & \
            (zi > np.float32(L["depth_eps"]))
        lo, hu, hv = float(L["pixel_border"]), float(p.W - 1 - L["pixel_border"]), float(p.H - 1 - L["pixel_border"])
        in_u, in_v = (u >= lo + 1e-3) & (u <= hu - 1e-3), (v >= lo + 1e-3) & (v <= hv - 1e-3)
        mask["left"] = pre & ~vo & (u <= lo - 1e-3) & in_v
        mask["right"] = pre & ~vo & (u >= hu + 1e-3) & in_v
        mask["top"] = pre & ~vo & (v <= lo - 1e-3) & in_u
        mask["bottom"] = pre & ~vo & (v >= hv + 1e-3) & in_u
        mask["inside"] = vo & matched & in_u & in_v

    def natural(e, want):
        """a natural match of edge e in class `want` (None: any valid one), by the oracle"""
        r, s = row_of[e], p.src[e]
        ks = np.flatnonzero(mask[want][r])
        if len(ks) == 0:
            return None
        k = int(ks[(7 * e) % len(ks)])
        return dict(k=k, idx=int(p.cidx[s, k]), Q=float(p.cQ[s, k]))

    # deal the classes over the edges: a class goes to the first free edge (pair) that can hold it
    for name in names:
        for e in slots:
            e = int(e)
            if e in lives:
                continue
            found = name in ("left", "right", "top", "bottom", "inside") or name.startswith("huber")
            l = natural(e, name if found else None)
            if l is None and name in ("huber3_on", "huber2_on") and p.mode != "points":
                # no natural match has so far a distance / depth: make one (below)
                l = natural(e, None)
                found = False
            if l is None:
                continue
            i, j, k, ind = int(p.ii[e]), int(p.jj[e]), l["k"], l["idx"]
            l = dict(e=e, k=k, idx=ind, Q=l["Q"], valid=True, cls=name)
            if not found:
                l["Q"] = 4.0
                ze = np.float32(L["depth_eps"])
                if name == "unmatched":
                    l["valid"] = False
                elif name == "q_eq":
                    l["Q"] = float(np.float32(L["Q_conf"]))
                elif name == "q_above":
                    l["Q"] = float(np.nextafter(np.float32(L["Q_conf"]), np.float32(np.inf)))
                elif name == "ci_eq":
                    Cs[i, ind] = L["C_conf"]
                elif name == "cj_eq":
                    Cs[j, k] = L["C_conf"]
                elif name == "ci_nan":
                    Cs[i, ind] = np.nan
                elif name == "cj_nan":
                    Cs[j, k] = np.nan
                elif name == "zi_eq":
                    Xs[i, ind] = Xs[i, ind] / Xs[i, ind, 2] * ze
                    Xs[i, ind, 2] = ze
                elif name in ("zi_above", "huber2_on"):  # log(zj / zi) ~ 14: the depth row's Huber is on
                    za = np.nextafter(ze, np.float32(np.inf))
                    Xs[i, ind] = Xs[i, ind] / Xs[i, ind, 2] * za
                    Xs[i, ind, 2] = za
                elif name == "zt_neg":
                    Xs[j, k] = -Xs[j, k]
                elif name == "huber3_on":  # rays: the matched point 6x as far
                    Xs[i, ind] = Xs[i, ind] * np.float32(6.0)
            l["want"] = name in ("q_above", "zi_above", "inside") or name.startswith("huber")
            lives[e] = l
            break
        else:
            raise AssertionError(f"{p.mode} {p.H}x{p.W}: no edge can hold class {name}")
    if p.on_rays:  # the doctored depths back on their rays, bit for bit
        Xs = _constrain(p.H, p.W, torch.from_numpy(Xs), torch.from_numpy(p.K)).numpy()
    # group by (parity, direction): the pairs of a call are disjoint
    calls = []
    for parity in (1, 0):
        for direction in (0, 1):
            live = [lives[int(e)] for _, e in pair_edges(p, parity, direction) if int(e) in lives]
            if live:
                c = make_call(oracle, p, L, live, Xs=Xs, Cs=Cs,
                              name=f"class-{'odd' if parity else 'even'}-{'fwd' if direction == 0 else 'bwd'}")
                calls.append(_annotate(c))
    return calls


# ------------------------------------------------------------------------------------------
# expected systems
# ------------------------------------------------------------------------------------------
CONTRACTS = ("nvcc", "off", "nvcc_right")


def assemble(p, edges, Hs, gs):
    """Dense (H, b) of the unpinned poses from per-edge blocks (the reference's SparseBlock:
    rows cat(ii, ii, jj, jj), cols cat(ii, jj, ii, jj); pose 0 pinned)."""
    n = 7 * (p.N - 1)
    H = np.zeros((n, n), np.float64)
    b = np.zeros((n,), np.float64)
    for r, e in enumerate(edges):
        i, j = int(p.ii[e]) - 1, int(p.jj[e]) - 1
        for blk, (a, c) in enumerate(((i, i), (i, j), (j, i), (j, j))):
            if a >= 0 and c >= 0:
                H[7 * a:7 * a + 7, 7 * c:7 * c + 7] += Hs[blk, r].astype(np.float64)
        if i >= 0:
            b[7 * i:7 * i + 7] += gs[0, r].astype(np.float64)
        if j >= 0:
            b[7 * j:7 * j + 7] += gs[1, r].astype(np.float64)
    return H, b


def expected(oracle, c, contract="nvcc"):
    """The call's exactly summed oracle system, from gn_align on its live edges alone."""
    P = oracle_params(oracle, c.p, c.L)
    with oracle.contract(contract), oracle.exact_sums():
        Hs, gs = oracle.gn_align(P, c.p.Twc, c.Xs, c.Cs, c.p.ii[c.edges], c.p.jj[c.edges], c.idx_rows,
                                 c.valid_rows, c.Q_rows)
    return assemble(c.p, c.edges, Hs, gs)


def blocks(A):
    """[n, n] -> [np, np, 7, 7]; [n] -> [np, 7]."""
    A = np.asarray(A)
    m = A.shape[0] // 7
    if A.ndim == 2:
        return A.reshape(m, 7, m, 7).transpose(0, 2, 1, 3)
    return A.reshape(m, 7)


def block_distance(G, R):
    """Per 7x7 block of H (or 7-row block of b): max |G - R| / max |R| of the block, and which blocks
    of R are exactly zero / hold a NaN.  A zero block's distance is 0 when G's block is exactly zero
    too, else inf; a NaN block's is 0 when G has NaN exactly where R has, else inf."""
    Gb, Rb = blocks(G), blocks(R)
    ax = tuple(range(Gb.ndim - (2 if np.asarray(G).ndim == 2 else 1), Gb.ndim))
    nan = np.isnan(Rb).any(axis=ax)
    zero = (Rb == 0).all(axis=ax)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(Gb - Rb).max(axis=ax) / np.abs(Rb).max(axis=ax)
    d = np.where(zero, np.where((Gb == 0).all(axis=ax), 0.0, np.inf), d)
    same_nan = (np.isnan(Gb) == np.isnan(Rb)).all(axis=ax)
    d = np.where(nan, np.where(same_nan, 0.0, np.inf), d)
    d = np.where(~nan & ~zero & np.isnan(d), np.inf, d)  # a NaN of G where R is finite
    return d, zero, nan


def describe_block(c, G, R, blk):
    """For a failure message: the block's worst entry on both sides and the live point(s) that feed
    the block's poses."""
    Gb, Rb = blocks(G)[tuple(blk)], blocks(R)[tuple(blk)]
    with np.errstate(invalid="ignore"):
        at = np.unravel_index(np.nanargmax(np.abs(Gb - Rb)) if np.isfinite(Gb - Rb).any() else 0, Gb.shape)
    poses = {int(x) + 1 for x in blk}
    pts = [f"edge {l['e']} ({int(c.p.ii[l['e']])}->{int(c.p.jj[l['e']])}) point {l['k']} match {l['idx']} "
           f"Q {l['Q']:.3g} {l['cls']}" for l in c.live if poses & {int(c.p.ii[l["e"]]), int(c.p.jj[l["e"]])}]
    return f"entry {tuple(int(x) for x in at)}: got {Gb[at]:.9g}, oracle {Rb[at]:.9g}, block max {np.abs(Rb).max():.3g}; " \
        + "; ".join(pts)


def convention_spread(oracle, c):
    """S: per block, the spread of the oracle's three contraction conventions (element-wise max
    - min) over the default convention's largest entry of the block.  -> (S_H, S_b, (H, b))"""
    sys = [expected(oracle, c, cm) for cm in CONTRACTS]
    return _block_spread([s[0] for s in sys]), _block_spread([s[1] for s in sys]), sys[0]


def intended_blocks(c):
    """The (row, col) pose blocks of H and the rows of b a call's VALID live points must fill."""
    Hb, bb = set(), set()
    for l in c.live:
        if not l["want"]:
            continue
        i, j = int(c.p.ii[l["e"]]) - 1, int(c.p.jj[l["e"]]) - 1
        for a, q in ((i, i), (i, j), (j, i), (j, j)):
            if a >= 0 and q >= 0:
                Hb.add((a, q))
        bb |= {a for a in (i, j) if a >= 0}
    return Hb, bb


def depth_row_b_f64(oracle, c, b):
    """calib: the oracle's b with every live point's DEPTH row re-evaluated in f64.  The reference
    forms that residual as logf(zj) - logf(zi), which loses ~1e-7 / |residual| of itself to
    cancellation; the kernels take one log of the ratio (gn_accum.hip, point_body_x).  Only the
    residual (and the Huber factor that depends on it) is replaced: the row's Jacobian and
    confidence weight stay the oracle's."""
    p = c.p
    b = b.copy()
    sd = sigmas_inv("calib", c.L)[2]
    for l in c.live:
        if not l["ovalid"]:
            continue
        i, j = int(p.ii[l["e"]]), int(p.jj[l["e"]])
        X = l["X"].astype(np.float64)
        zj_inv = np.float32(1.0 / X[2])
        J = np.array([0, 0, zj_inv, np.float32(l["X"][1]) * zj_inv, -(np.float32(l["X"][0]) * zj_inv), 0, 1], np.float32)
        Jj = oracle.apply_sim3_adj_inv(p.Twc[i], J).astype(np.float64)
        e32, w32 = float(l["err"][2]), float(l["w"][2])
        zi = c.Xs[i, l["idx"] if l.get("valid", True) else 0, 2]
        e64 = np.log(X[2]) - np.log(float(zi))
        sw = float(np.float32(sd * np.sqrt(np.float32(l["Q"]))))
        r = abs(sw * e64)
        w64 = (1.0 if r < HUBER_K else HUBER_K / r) * sw * sw
        d = (w64 * e64 - w32 * e32) * Jj
        if i >= 1:
            b[7 * (i - 1):7 * i] -= d
        if j >= 1:
            b[7 * (j - 1):7 * j] += d
    return b


# ------------------------------------------------------------------------------------------
# the GPU side
# ------------------------------------------------------------------------------------------
class DeviceGraph:
    """A probe graph's tensors on the device, uploaded once: the edge arrays start all unmatched and
    a call writes its few live entries (and restores them), so a 4096-edge call moves no edge
    array over the bus."""

    def __init__(self, p):
        dev = torch.device("cuda", 0)
        self.p = p
        self.H, self.W = p.H, p.W
        self.K = torch.from_numpy(p.K).to(dev)
        self.ii = torch.from_numpy(p.ii).to(dev)
        self.jj = torch.from_numpy(p.jj).to(dev)
        self.Twc = torch.from_numpy(p.Twc).to(dev)
        self.idx = torch.zeros((p.E, p.HW), dtype=torch.int64, device=dev)
        self.valid = torch.zeros((p.E, p.HW, 1), dtype=torch.bool, device=dev)
        self.Q = torch.full((p.E, p.HW, 1), 2.0, dtype=torch.float32, device=dev)
        self._x = {}

    def _tensor(self, a):
        k = id(a)
        if k not in self._x:
            self._x[k] = (a, torch.from_numpy(np.ascontiguousarray(a)).cuda())
        return self._x[k][1]

    def build_system(self, c):
        """Dense (H, b) of call c from m3s_gn_build_system under the environment's path switches."""
        import mast3r_slam_backends as mb
        from m3s.debug import make_args

        self.Xs = self._tensor(c.Xs)
        self.Cs = self._tensor(c.Cs)
        e = torch.from_numpy(c.edges).cuda()
        k = torch.tensor([l["k"] for l in c.live], device="cuda")
        self.idx[e, k] = torch.tensor([l["idx"] for l in c.live], device="cuda")
        self.valid[e, k, 0] = torch.tensor([l.get("valid", True) for l in c.live], device="cuda")
        self.Q[e, k, 0] = torch.tensor([l["Q"] for l in c.live], dtype=torch.float32, device="cuda")
        try:
            Twc = self.Twc.clone()
            a, keep = make_args(self, self.p.mode, c.L, Twc, local=(self.idx, self.valid, self.Q))
            n = 7 * (self.p.N - 1)
            H = np.zeros((n, n), np.float64)
            b = np.zeros((n,), np.float64)
            rc = mb.lib.m3s_gn_build_system(ctypes.byref(a), H.ctypes.data_as(ctypes.c_void_p),
                                            b.ctypes.data_as(ctypes.c_void_p))
            mb._raise(rc, "gn_build_system")
            del keep
        finally:
            self.idx[e, k] = 0
            self.valid[e, k, 0] = False
            self.Q[e, k, 0] = 2.0
        return H, b


# the shapes of the impulse probes: (family, H, W, npairs, directed edges or None = the chain alone)
TINY = [(5, 7), (3, 21), (5, 13), (15, 17), (16, 16)]
SMALL = [(24, 32), (36, 64), (40, 52), (37, 53), (48, 64), (64, 64)]
DEEP = [(36, 64), (40, 52), (64, 64)]
SHAPES = ([("tiny", h, w, 16, None) for h, w in TINY] + [("small", h, w, 16, None) for h, w in SMALL] +
          [("deep", h, w, 32, 4096) for h, w in DEEP])
MODES = ["rays", "calib", "points"]
# where the class calls live: a width that is no power of two, three chunks, 34 keyframes
CLASS_SHAPE = (40, 52, 16)
# the reference's own floor a usable graph must keep (the convention spread S of every impulse
# block, the reference-order distance of every dense block); a graph above it gets the next seed
FLOOR_MAX = 1e-4
FIRST_SEED, SEED_TRIES = 21, 24


def shape_id(s):
    return f"{s[0]}{s[1]}x{s[2]}"


@functools.lru_cache(maxsize=None)
def calls_of(oracle, shape, mode, off_rays=False):
    """(graph, impulse calls with their expected systems) of a (shape, mode).  Tiny and small graphs
    place every position (as many rounds as that takes); deep graphs run one round per choice of
    the live duplicate.  The graph's seed is the first from FIRST_SEED on at which no block's
    convention spread exceeds FLOOR_MAX and every block is resolvable (unresolved_blocks)."""
    fam, H, W, npairs, E = shape
    for seed in range(FIRST_SEED, FIRST_SEED + SEED_TRIES):
        p = probe_graph(H, W, mode, npairs, E, seed=seed, off_rays=off_rays)
        p.seed = seed
        if fam == "deep":
            calls = []
            for n, at in enumerate(("first", "middle", "last")):
                for c in impulse_calls(oracle, p, live_at=at, rounds=1, offset=n * (p.npairs + 1)):
                    c.name = f"{at}-{c.name}"
                    calls.append(c)
        else:
            calls = impulse_calls(oracle, p)
        if max(max(c.S_H.max(), c.S_b.max()) for c in calls) > FLOOR_MAX:
            continue
        if not any(unresolved_blocks(c) for c in calls):
            return p, calls
    raise AssertionError(f"{shape_id(shape)} {mode}: no seed keeps the convention spread below {FLOOR_MAX}")


# ------------------------------------------------------------------------------------------
# dense graphs: the accum-trim recording's own graphs (and the tiny shapes) under the oracle
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def trim():
    """tests/golden/make_accum_trim_golden.py as a module (its GRAPHS, MODES, make_graph)."""
    import importlib.util

    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("make_accum_trim_golden",
                                                  os.path.join(here, "golden", "make_accum_trim_golden.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    return rec


ALL_DENSE_MODES = ["calib", "calib_pos", "rays", "points"]


def dense_cases():
    """[(spec, mode)]: every accum-trim graph in the modes its generator lists, and the tiny shapes
    with 6 keyframes in all four."""
    rec = trim()
    out = [(spec, mode) for spec in rec.GRAPHS for mode in rec.MODES[spec[0]]]
    out += [((f"tiny{h}x{w}", 6, 5, h, w, 11), mode) for h, w in TINY for mode in ALL_DENSE_MODES]
    return out


@functools.lru_cache(maxsize=4)
def dense_graph(spec):
    name, N, E, H, W, seed = spec
    if not name.startswith("tiny"):
        return trim().make_graph(spec)
    # the generator's dead points, at indices that exist in a tiny image
    g = synth.make_graph(dict(N=N, E=E), H=H, W=W, seed=seed)
    HW = H * W
    g.valid[1, 2:9] = False
    g.valid[3, HW - 5:] = False
    g.valid[g.E_directed - 1, ::7] = False
    g.Q[0, HW // 2] = 1.0
    return g


def dense_inputs(spec, mode):
    """(graph with the mode's Xs, op mode, points on their rays?)"""
    import dataclasses

    g = dense_graph(spec)
    op, Xs = trim().mode_inputs(g, mode)
    return dataclasses.replace(g, Xs=Xs), op, mode == "calib"


def dense_reference(oracle, g, op):
    """The exactly summed oracle system and the reference-order one of a dense graph."""
    p = types.SimpleNamespace(mode=op, K=g.K.numpy(), H=g.H, W=g.W)
    P = oracle_params(oracle, p, LOCAL)
    arrs = [t.numpy() for t in (g.Twc, g.Xs, g.Cs, g.ii, g.jj, g.idx, g.valid, g.Q)]
    with oracle.exact_sums():
        Hx, bx = oracle.gn_build_system(P, *arrs)
    Hr, br = oracle.gn_build_system(P, *arrs)
    return (Hx, bx), (Hr, br)
