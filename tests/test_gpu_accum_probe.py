"""The GN accumulate against the oracle POINT BY POINT, on every path and at every loop shape.

3a (impulse blocks).  tests/accum_probe.py builds calls in which every non-zero 7x7 block of the
dense normal equations (m3s_gn_build_system) is ONE point's contribution from ONE known directed
edge: a chain of 34 (tiny, small) or 66 (deep: 4096 directed edges, the chunk is the whole image)
keyframes, one live point on one directed edge of each of a set of disjoint pairs, everything else
unmatched.  The live points sit where the kernels' loops change shape (first lanes, wave and step
ends, chunk boundaries, the image's last points; on the deep graphs on the first, a middle and the
last duplicate of a pair, so also on the launch's first and last edge), and in a second family in
every validity and weight class (unmatched, Q at and just above Q_thresh, a confidence at C_thresh
or NaN, calib: the matched depth at and just above z_eps, a transformed depth behind the camera, a
projection outside each border, and every Huber row on and off).  Every block must be within
    tol = max(1e-4, 64 S)
of the exactly summed oracle block, relative to that block's own largest entry: 1e-4 is the
project's normal-equation tolerance (test_normal_equations_match_oracle) applied per block
instead of to the matrix scale, and S is the block's spread over the oracle's three contraction
conventions -- the fast path's formulas (the affine s M x + t, 1-ulp v_rcp / v_rsq, log2 of the
depth ratio) move a term by a few f32 ulp each, as a contraction choice does.  A block the oracle
has exactly zero (dead edges, invalid classes, pairs without an edge) must be exactly zero.
calib's depth residual: the reference's logf(zj) - logf(zi) loses ~1e-7 / |residual| of itself to
cancellation where the kernels take one log of the ratio (gn_accum.hip, point_body_x); a calib b
block outside tol is therefore compared once more with the oracle's block whose depth row is
re-evaluated in f64 (accum_probe.depth_row_b_f64), at the SAME tol.

3b (dense blocks).  The graphs of tests/golden/make_accum_trim_golden.py -- whose recording only
freezes the kernel's bits -- and the tiny shapes with 6 keyframes, every mode the generator
lists, every path: each block of H and b within max(1e-4, 4 sigma_block) of the exactly summed
oracle block, sigma_block = the reference-order oracle's own distance for that block (the form of
tests/test_gpu_gn_stress.py's bound).  A 1-iteration call with the same switches reads the device
flags back: the packed and ray-constrained bits are asserted per path.

Paths (accum_probe.PATHS): unpacked (M3S_GN_PACK=0), packed positional (PACK=2, COMPACT=0,
RAYCHECK=0), compacted (COMPACT=1), calib ray-constrained (RAYCHECK=1, points on their rays),
and the separate edge-reduce launch (M3S_GN_FUSE_REDUCE=0).  Shapes whose point count is no
multiple of 4 have the unpacked kernel's scalar loop only.

Which points can hold a kernel to tol.  The first GPU run had ONE block of ~1e4 outside tol: 36x64,
4096 edges, calib, point 1023 of edge 16->15, b blocks of poses 15 and 16, every path 1.16e-4 from
the oracle at tol 1e-4 (S = 7.9e-9): a pixel residual of 0.04 px at u ~ 40, where one ulp of u is
1e-4 of the block and the conventions happen to agree.  Rounding that point's inputs by one ulp
moves the ORACLE's own block by 1.2e-4, so no f32 kernel can be held to 1e-4 there.  The probes
therefore place only RESOLVABLE points (accum_probe.unresolved_blocks: one-ulp input rounding
moves the oracle's block by at most tol / 4; decided by the oracle alone and pinned in
tests/test_accum_probe_host.py); a point that is not gets a corner match like an invalid one
(0 to 4 % of a graph's points, calib almost only).  tol itself is as above.

Measured on MI355X, largest distance / tol per (mode, path) over all shapes:
  impulse  rays       unpacked 0.407, packed 0.407, compact 0.407, unfused 0.407
           calib      unpacked 0.864, packed 0.319, compact 0.319, raycheck 0.303, unfused 0.303
           calib_pos  unpacked 0.414, packed 0.414, compact 0.414, unfused 0.414
           points     unpacked 0.465, packed 0.465, compact 0.465, unfused 0.465
  classes  rays 0.099, calib 0.058, calib_pos 0.083, points 0.077 (every path alike)
  dense    rays       unpacked 0.018, packed 0.018, compact 0.017, unfused 0.018
           calib      unpacked 0.006, packed 0.006, compact 0.007, raycheck 0.005, unfused 0.005
           calib_pos  unpacked 0.006, packed 0.005, compact 0.005, unfused 0.005
           points     unpacked 0.016, packed 0.016, compact 0.016, unfused 0.016
(calib's unpacked 0.864 comes from the shapes that have the scalar loop only, 5x13 and 37x53; no
calib b block needed the f64 depth row.)  Seeded mutations of gn_accum.hip, each run against this
file: dropping the last group of a partial step fails test_impulse_blocks_match_oracle on every
shape with a partial step and test_dense_blocks_match_oracle; reading idx[p+1] for idx[p] fails
every test here; >= for > in the Q test fails test_class_blocks_match_oracle (class q_eq: a block
where the oracle has exactly zero); W-1 for W in the calib pixel decode fails the calib cases of
all three.
"""
import numpy as np
import pytest

import accum_probe as ap

pytestmark = pytest.mark.gpu

IMPULSE = [(s, m, False) for s in ap.SHAPES for m in ap.MODES]
# calib points moved off their rays (the positional stream whatever M3S_GN_RAYCHECK says)
IMPULSE += [(s, "calib", True) for s in ap.SHAPES if (s[0], s[1], s[2]) in
            (("tiny", 16, 16), ("small", 40, 52), ("deep", 36, 64))]
IMPULSE_IDS = [f"{ap.shape_id(s)}-{m}{'_pos' if off else ''}" for s, m, off in IMPULSE]


def _check_call(oracle, dg, c, path, stats):
    """One call on one path: every block within tol of the oracle's, zero blocks exactly zero."""
    with ap.path_env(path):
        Hg, bg = dg.build_system(c)
    bad = []
    worst = 0.0
    for what, G, R, S in (("H", Hg, c.Hx, c.S_H), ("b", bg, c.bx, c.S_b)):
        d, zero, nan = ap.block_distance(G, R)
        tol = np.maximum(1e-4, 64.0 * S)
        ratio = d / tol
        if what == "b" and c.p.mode == "calib" and (ratio > 1).any() and not np.isinf(d).any():
            # the depth row in f64 (see the module docstring): the same tol
            d2, _, _ = ap.block_distance(G, ap.depth_row_b_f64(oracle, c, R))
            ratio = np.where(ratio > 1, d2 / tol, ratio)
        for blk in np.argwhere(ratio > 1):
            bad.append(f"{c.name} {path} {what}{tuple(int(x) + 1 for x in blk)}: distance "
                       f"{d[tuple(blk)]:.3g}, tol {tol[tuple(blk)]:.3g} ({ap.describe_block(c, G, R, blk)})")
        worst = max(worst, float(ratio.max()))
    stats[path] = max(stats.get(path, 0.0), worst)
    return bad


def _run_calls(oracle, p, calls):
    dg = ap.DeviceGraph(p)
    stats, bad = {}, []
    for path in ap.paths_for(p.H, p.W, p.mode, p.on_rays):
        for c in calls:
            bad += _check_call(oracle, dg, c, path, stats)
    return stats, bad


@pytest.mark.parametrize("shape,mode,off_rays", IMPULSE, ids=IMPULSE_IDS)
def test_impulse_blocks_match_oracle(backend, oracle, shape, mode, off_rays):
    p, calls = ap.calls_of(oracle, shape, mode, off_rays)
    stats, bad = _run_calls(oracle, p, calls)
    print(f"impulse {ap.shape_id(shape)} {mode}{'_pos' if off_rays else ''}: distance / tol "
          + ", ".join(f"{k} {v:.3f}" for k, v in stats.items()))
    assert not bad, f"{len(bad)} blocks: " + "; ".join(bad[:12])


@pytest.mark.parametrize("mode,off_rays", [("rays", False), ("calib", False), ("calib", True), ("points", False)],
                         ids=["rays", "calib", "calib_pos", "points"])
def test_class_blocks_match_oracle(backend, oracle, mode, off_rays):
    """Every validity and weight class: the valid ones within tol of their oracle block, the
    invalid ones exactly zero (tests/test_accum_probe_host.py pins that each class is populated)."""
    H, W, npairs = ap.CLASS_SHAPE
    p = ap.probe_graph(H, W, mode, npairs, off_rays=off_rays)
    calls = [ap.attach_expected(oracle, c) for c in ap.class_calls(oracle, p)]
    for c in calls:
        for l in c.live:
            assert l["cls"] in l["classes"] and l["ovalid"] == l["want"], l["cls"]
    stats, bad = _run_calls(oracle, p, calls)
    print(f"classes {mode}{'_pos' if off_rays else ''}: distance / tol "
          + ", ".join(f"{k} {v:.3f}" for k, v in stats.items()))
    assert not bad, f"{len(bad)} blocks: " + "; ".join(bad[:12])


DENSE = ap.dense_cases()


def _path_flags(backend, g, op, path):
    """The device flags of a 1-iteration call under the path's switches (m3s_gn_build_system does
    not read them back; setup() decides the path from the same switches).  g: on the device."""
    import os

    import torch

    L = ap.LOCAL
    Twc = g.Twc.clone()
    c = lambda t: t
    with ap.path_env(path):
        os.environ["M3S_GN_DEBUG_FLAGS"] = "2"
        try:
            if op == "calib":
                backend.gauss_newton_calib(Twc, c(g.Xs), c(g.Cs), c(g.K), c(g.ii), c(g.jj), c(g.idx), c(g.valid),
                                           c(g.Q), g.H, g.W, L["pixel_border"], L["depth_eps"], L["sigma_pixel"],
                                           L["sigma_depth"], L["C_conf"], L["Q_conf"], 1, 0.0)
            elif op == "rays":
                backend.gauss_newton_rays(Twc, c(g.Xs), c(g.Cs), c(g.ii), c(g.jj), c(g.idx), c(g.valid), c(g.Q),
                                          L["sigma_ray"], L["sigma_dist"], L["C_conf"], L["Q_conf"], 1, 0.0)
            else:
                backend.gauss_newton_points(Twc, c(g.Xs), c(g.Cs), c(g.ii), c(g.jj), c(g.idx), c(g.valid),
                                            c(g.Q), L["sigma_point"], L["C_conf"], L["Q_conf"], 1, 0.0)
            torch.cuda.synchronize()
        finally:
            del os.environ["M3S_GN_DEBUG_FLAGS"]
    return backend.gn_debug_flags()


@pytest.mark.parametrize("spec,mode", DENSE, ids=[f"{s[0]}-{m}" for s, m in DENSE])
def test_dense_blocks_match_oracle(backend, oracle, spec, mode):
    import dataclasses

    import torch
    from m3s.debug import build_system_gpu

    g, op, on_rays = ap.dense_inputs(spec, mode)
    (Hx, bx), (Hr, br) = ap.dense_reference(oracle, g, op)
    # on the device once, for every path's call
    g = dataclasses.replace(g, **{f.name: getattr(g, f.name).cuda() for f in dataclasses.fields(g)
                                  if isinstance(getattr(g, f.name), torch.Tensor)})
    sH, _, _ = ap.block_distance(Hr, Hx)
    sb, _, _ = ap.block_distance(br, bx)
    bad, stats = [], {}
    for path in ap.paths_for(g.H, g.W, op, on_rays):
        with ap.path_env(path):
            Hg, bg = build_system_gpu(g, op, ap.LOCAL)
        worst = 0.0
        for what, G, R, s in (("H", Hg, Hx, sH), ("b", bg, bx, sb)):
            d, zero, nan = ap.block_distance(G, R)
            tol = np.maximum(1e-4, 4.0 * s)
            ratio = d / tol
            for blk in np.argwhere(ratio > 1):
                bad.append(f"{path} {what}{tuple(int(x) + 1 for x in blk)}: distance {d[tuple(blk)]:.3g}, "
                           f"tol {tol[tuple(blk)]:.3g}")
            worst = max(worst, float(ratio.max()))
        stats[path] = worst
        if spec[0].startswith("deep"):  # (the path does not depend on the edge count)
            continue
        st = _path_flags(backend, g, op, path)
        packed = path != "unpacked" and g.HW % 4 == 0
        assert bool(st["packed"]) == packed, (path, st)
        # the ray-constrained stream: points on their rays, the positional streams not forced
        rc = packed and op == "calib" and on_rays and g.W % 4 == 0 and path in ("raycheck", "unfused")
        assert bool(st["ray_constrained"]) == rc, (path, st)
    print(f"dense {spec[0]} {mode}: distance / tol " + ", ".join(f"{k} {v:.3f}" for k, v in stats.items())
          + f"; sigma_block H <= {sH.max():.2e}, b <= {sb.max():.2e}")
    assert not bad, f"{len(bad)} blocks: " + "; ".join(bad[:12])
