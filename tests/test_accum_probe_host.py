"""The accumulate probes' inputs are what they claim to be -- by the oracle alone, without a GPU.

tests/test_gpu_accum_probe.py compares single-point blocks of the GPU's normal equations with the
oracle's.  That comparison would pass vacuously if an impulse call held no valid point, if a block
were fed by two points, or if a validity class were never populated; these tests pin those
conditions, the restated planner chunking, and the reference's own noise floors (printed; measured
here: the three contraction conventions differ by up to 9.5e-5 of a single point's block -- rays
and calib at 36x64 to 64x64 -- and the reference-order system lies 2.5e-8 to 2.4e-7 per block from
the exactly summed one on the dense graphs).

One more floor, which the convention spread S does not see: calib's pixel residual u - u_target is
a difference of two numbers of up to W, and where it is a few hundredths of a pixel ONE ulp of u
is 1e-4 of the point's b block, while the conventions (which touch only u's last multiply-add) may
agree there to 1e-8.  The first GPU run met such a point (36x64, 4096 edges, calib, point 1023 of
edge 16->15: every path 1.16e-4 from the oracle at S = 7.9e-9).  So a live point also has to be
RESOLVABLE: rounding every input coordinate one ulp up or down must move the oracle's own block
by at most a quarter of the tolerance.  A point that is not gets a corner match like an invalid
one (a residual of many pixels); 0 to 4 % of a graph's points.
"""
import numpy as np
import pytest

import accum_probe as ap

IMPULSE = [(s, m) for s in ap.SHAPES for m in ap.MODES]
IMPULSE_IDS = [f"{ap.shape_id(s)}-{m}" for s, m in IMPULSE]
FLOOR_MAX = ap.FLOOR_MAX  # a graph whose reference floor exceeds this is unusable (accum_probe.calls_of)


@pytest.mark.parametrize("shape,mode", IMPULSE, ids=IMPULSE_IDS)
def test_impulse_calls_fill_exactly_the_intended_blocks(oracle, shape, mode):
    """Every live point is valid by the oracle, its blocks are non-zero and finite in the exactly
    summed oracle system, every other block is exactly zero, the conventions' spread S stays
    below FLOOR_MAX, and every block is resolvable: rounding the inputs by one ulp moves the oracle's
    own block by at most a quarter of the GPU test's tolerance max(1e-4, 64 S).  Every position of
    live_positions() is used."""
    p, calls = ap.calls_of(oracle, shape, mode)
    want_pos = set(ap.live_positions(p.HW, mode, p.E))
    seen, worst, worst_r, nre = set(), 0.0, 0.0, 0
    for c in calls:
        assert not ap.unresolved_blocks(c), c.name
        tH, tb = ap.tolerance(c)
        worst_r = max(worst_r, (c.R_H / tH).max(), (c.R_b / tb).max())
        nre += sum(bool(l.get("rematched")) for l in c.live)
        assert all(l["ovalid"] for l in c.live), c.name
        pairs = [frozenset((int(p.ii[l["e"]]), int(p.jj[l["e"]]))) for l in c.live]
        assert len(set().union(*pairs)) == 2 * len(pairs), f"{c.name}: the live pairs share a keyframe"
        seen |= {l["k"] for l in c.live}
        S_H, S_b, H, b = c.S_H, c.S_b, c.Hx, c.bx
        Hb, bb = ap.intended_blocks(c)
        nzH = {tuple(x) for x in np.argwhere(np.abs(ap.blocks(H)).max(axis=(2, 3)) > 0)}
        nzb = {int(x) for x in np.flatnonzero(np.abs(ap.blocks(b)).max(axis=1) > 0)}
        assert nzH == Hb and nzb == bb, c.name
        assert np.isfinite(H).all() and np.isfinite(b).all()
        worst = max(worst, S_H.max(), S_b.max())
    assert seen >= want_pos if shape[0] != "deep" else len(seen) >= min(len(want_pos), 3 * p.npairs)
    if shape[0] == "deep":  # the launch's first and last edge index are live
        live_edges = {int(e) for c in calls for e in c.edges}
        assert 0 in live_edges and p.E - 1 in live_edges
    print(f"{ap.shape_id(shape)} {mode}: seed {p.seed}, {len(calls)} calls, convention spread S <= {worst:.2e}, "
          f"one-ulp input rounding <= {worst_r:.2f} tol, {nre} of {sum(len(c.live) for c in calls)} points re-matched")
    assert 8 * nre <= sum(len(c.live) for c in calls)  # the corner matches stay the exception
    assert worst <= FLOOR_MAX


@pytest.mark.parametrize("mode", ap.MODES)
def test_every_class_is_populated_as_intended(oracle, mode):
    """Each class of the table holds a live point that the ORACLE puts in that class, valid or
    invalid as intended; invalid classes leave their blocks exactly zero in the oracle system."""
    H, W, npairs = ap.CLASS_SHAPE
    p = ap.probe_graph(H, W, mode, npairs)
    calls = ap.class_calls(oracle, p)
    got = {}
    for c in calls:
        for l in c.live:
            assert l["cls"] in l["classes"], (l["cls"], sorted(l["classes"]))
            assert l["ovalid"] == l["want"], l["cls"]
            got[l["cls"]] = l["ovalid"]
        Hx, bx = ap.expected(oracle, c)
        Hb, bb = ap.intended_blocks(c)
        nzH = {tuple(x) for x in np.argwhere(np.abs(ap.blocks(Hx)).max(axis=(2, 3)) > 0)}
        assert nzH == Hb, c.name
    assert set(got) == set(ap.class_names(mode))
    assert sum(got.values()) >= 2 * (4 if mode == "rays" else 3) and not all(got.values())
    print(mode, {k: ("valid" if v else "invalid") for k, v in got.items()})


def test_restated_chunking_matches_what_the_generator_documents():
    """gn_plan.hip's choose_nchunks restated: the small family (10 directed edges; here 66) is cut
    into chunks of at most 1024 points -- 36x64 into 3 x 768, 40x52 into 696, 696, 688 -- and the
    4096-edge family gets the whole image as one chunk."""
    rec = ap.trim()
    for name, N, E, H, W, seed in rec.GRAPHS:
        HW = H * W
        starts, chunk = ap.chunk_starts(HW, 2 * E)
        if name.startswith("small"):
            assert chunk <= 1024 and len(starts) == -(-HW // 1024)
        else:
            assert starts == [0] and chunk == HW
    assert ap.chunk_starts(36 * 64, 10) == ([0, 768, 1536], 768)
    assert ap.chunk_starts(40 * 52, 10) == ([0, 696, 1392], 696)
    assert ap.chunk_starts(24 * 32, 10) == ([0], 768)
    for _, H, W, npairs, E in ap.SHAPES:
        starts, chunk = ap.chunk_starts(H * W, E if E else 2 * (2 * npairs + 1))
        assert (chunk == H * W) if E else (chunk <= 1024)
        assert chunk % 4 == 0 or len(starts) == 1


def test_block_distance_flags_zero_nan_and_single_entries():
    R = np.zeros((14, 14))
    R[:7, :7] = np.arange(49).reshape(7, 7) + 1.0
    R[7, 7] = np.nan
    G = R.copy()
    G[0, 0] += 49 * 1e-3
    d, zero, nan = ap.block_distance(G, R)
    assert zero.tolist() == [[False, True], [True, False]] and nan.tolist() == [[False, False], [False, True]]
    assert abs(d[0, 0] - 1e-3) < 1e-12 and d[0, 1] == 0 and d[1, 1] == 0
    G[0, 13] = 1e-300
    G[7, 7] = 0.0
    d, _, _ = ap.block_distance(G, R)
    assert np.isinf(d[0, 1]) and np.isinf(d[1, 1])
    d, zero, nan = ap.block_distance(np.array([1.0] * 7 + [0.0] * 7), np.array([2.0] * 7 + [0.0] * 7))
    assert d.tolist() == [0.5, 0.0] and zero.tolist() == [False, True]


DENSE = ap.dense_cases()


@pytest.mark.parametrize("spec,mode", DENSE, ids=[f"{s[0]}-{m}" for s, m in DENSE])
def test_dense_reference_floor(oracle, spec, mode):
    """The reference-order oracle's own distance from the exactly summed system, per block: the
    floor the dense GPU comparison's bound max(1e-4, 4 sigma) is built on."""
    g, op, _ = ap.dense_inputs(spec, mode)
    (Hx, bx), (Hr, br) = ap.dense_reference(oracle, g, op)
    dH, zH, nH = ap.block_distance(Hr, Hx)
    db, zb, nb = ap.block_distance(br, bx)
    assert not nH.any() and not nb.any() and not zb.any()
    print(f"{spec[0]} {mode}: sigma_block H <= {dH.max():.2e}, b <= {db.max():.2e}; "
          f"{int((~zH).sum())} of {zH.size} H blocks filled")
    assert dH.max() <= FLOOR_MAX and db.max() <= FLOOR_MAX
