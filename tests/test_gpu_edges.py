"""Edge construction after matching (edges.hip via mast3r_slam_backends.edge_confidence and
m3s.global_opt.FactorGraph.add_matched_factors) against the REFERENCE add_factors
(tests/golden/make_edges_golden.py -> edges_golden.npz: global_opt.py:53-99 run as written)
and against the torch expressions at full size: bit-exact confidences, exact counts.

Below those, the op against the host model (tests/keyframe_model.edge_confidence: f32 product,
correctly rounded sqrt, f32 compare, indices clamped to the pair's row) at every launch shape
(one thread up to B > 2048 and empty trailing chunks), at the Q_conf threshold and at zero,
negative, NaN, Inf and subnormal products, with out-of-range indices, and the binding's checks.
Nothing there compares the op with itself."""
import os

import numpy as np
import pytest
import torch

import keyframe_model as M

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "edges_golden.npz"))
DEV = "cuda"
NAMES = ["idx_i2j", "idx_j2i", "valid_match_j", "valid_match_i", "Qii", "Qjj", "Qji", "Qij"]


def _sqrt_ref_store(c_last, n):
    """The reference store's Q_ii2jj / Q_jj2ii with correctly rounded sqrt (float64 sqrt
    rounded to float32), replaying the accepted edges of calls 0..c_last."""
    parts = []
    for c in range(c_last + 1):
        if bool(GOLD[f"c{c}_reloc"]) and not bool(GOLD[f"c{c}_ret"]):
            continue
        B, HW = GOLD[f"c{c}_idx_i2j"].shape
        bi = np.arange(B)[:, None]
        if n == "Q_ii2jj":
            prod = GOLD[f"c{c}_Qii"][bi, GOLD[f"c{c}_idx_i2j"]] * GOLD[f"c{c}_Qji"]
        else:
            prod = GOLD[f"c{c}_Qjj"][bi, GOLD[f"c{c}_idx_j2i"]] * GOLD[f"c{c}_Qij"]
        q = np.sqrt(prod.astype(np.float64)).astype(np.float32)
        # keep the pairs the reference kept (its store grew by exactly those rows, in order)
        prev = 0 if c == 0 else GOLD[f"c{c - 1}_store_{n}"].shape[0]
        kept = GOLD[f"c{c}_store_ii"][prev:]
        ii = GOLD[f"c{c}_ii"]
        jj = GOLD[f"c{c}_jj"]
        sel = [k for k in range(B) if any((ii[k] == a and jj[k] == b) for a, b in
                                          zip(kept, GOLD[f"c{c}_store_jj"][prev:]))]
        parts.append(q[sel])
    return np.concatenate(parts, axis=0)


def test_add_matched_factors_matches_reference_store():
    from m3s.global_opt import FactorGraph

    fg = FactorGraph(None, None, device=DEV)
    for c in range(int(GOLD["ncalls"])):
        m = [torch.from_numpy(GOLD[f"c{c}_{n}"]).to(DEV) for n in NAMES]
        ret = fg.add_matched_factors(GOLD[f"c{c}_ii"].tolist(), GOLD[f"c{c}_jj"].tolist(), *m,
                                     float(GOLD["min_match_frac"]), is_reloc=bool(GOLD[f"c{c}_reloc"]))
        assert bool(ret) == bool(GOLD[f"c{c}_ret"])
        for n in ["ii", "jj", "idx_ii2jj", "idx_jj2ii", "valid_match_j", "valid_match_i", "Q_ii2jj", "Q_jj2ii"]:
            got = getattr(fg, n).cpu().numpy()
            ref = GOLD[f"c{c}_store_{n}"]
            assert got.shape == ref.shape and got.dtype == ref.dtype, (c, n)
            if n.startswith("Q_"):
                # the fixture ran torch's CPU sqrt, which is not correctly rounded (~1/6 of the
                # values are 1 ulp off); the op rounds correctly like CUDA's sqrtf (checked
                # bit-exactly against float64 sqrt below) -> 1 ulp here
                assert np.array_equal(got, _sqrt_ref_store(c, n)), (c, n)
                assert np.max(np.abs(got.view(np.int32) - ref.view(np.int32))) <= 1, (c, n)
            else:
                assert np.array_equal(got, ref), (c, n)


def test_edge_confidence_full_size_bit_exact(backend):
    B, HW = 8, 384 * 512
    g = torch.Generator(device=DEV).manual_seed(3)
    idx_i2j = torch.randint(0, HW, (B, HW), generator=g, device=DEV)
    idx_j2i = torch.randint(0, HW, (B, HW), generator=g, device=DEV)
    vj = torch.rand((B, HW, 1), generator=g, device=DEV) > 0.2
    vi = torch.rand((B, HW, 1), generator=g, device=DEV) > 0.2
    Q = [torch.exp(torch.randn((B, HW, 1), generator=g, device=DEV)) for _ in range(4)]
    Qj, Qi, counts = backend.edge_confidence(idx_i2j, idx_j2i, vj, vi, *Q, 1.5)
    bi = torch.arange(B, device=DEV)[:, None].repeat(1, HW)
    # global_opt.py:56-57 with a correctly rounded f32 sqrt (CUDA's sqrtf; f64 sqrt rounded)
    ref_Qj = torch.sqrt((Q[0][bi, idx_i2j] * Q[2]).double()).float()
    ref_Qi = torch.sqrt((Q[1][bi, idx_j2i] * Q[3]).double()).float()
    assert torch.equal(Qj, ref_Qj) and torch.equal(Qi, ref_Qi)
    assert torch.equal(counts[:, 0].long(), (vj & (ref_Qj > 1.5)).sum(dim=(1, 2)))
    assert torch.equal(counts[:, 1].long(), (vi & (ref_Qi > 1.5)).sum(dim=(1, 2)))


def test_device_factor_graph_store_equals_reference_store():
    """DeviceFactorGraph appends into its two-way EdgeStore (capacity doubling) instead of
    concatenating: after every add_factors call its edge attributes are exactly the
    reference-compatible FactorGraph's."""
    from m3s.global_opt import DeviceFactorGraph, FactorGraph

    fg = FactorGraph(None, None, device=DEV)
    dg = DeviceFactorGraph(None, None, device=DEV)
    for c in range(int(GOLD["ncalls"])):
        m = [torch.from_numpy(GOLD[f"c{c}_{n}"]).to(DEV) for n in NAMES]
        args = (GOLD[f"c{c}_ii"].tolist(), GOLD[f"c{c}_jj"].tolist(), *m, float(GOLD["min_match_frac"]))
        r1 = fg.add_matched_factors(*args, is_reloc=bool(GOLD[f"c{c}_reloc"]))
        r2 = dg.add_matched_factors(*args, is_reloc=bool(GOLD[f"c{c}_reloc"]))
        assert r1 == r2
        for n in ["ii", "jj", "idx_ii2jj", "idx_jj2ii", "valid_match_j", "valid_match_i", "Q_ii2jj", "Q_jj2ii"]:
            assert torch.equal(getattr(fg, n), getattr(dg, n)), (c, n)
        a, b = fg.prep_two_way_edges(), dg.prep_two_way_edges()
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert dg.edges.capacity >= dg.edges.E


# ------------------------------------------------------------------ against the host model
# (tests/keyframe_model.edge_confidence, held to the reference's add_factors by
# tests/test_keyframe_model.py): confidences bit for bit, NaN as NaN, counts equal.

Q_CONF = 1.5


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _draw(B, HW, seed):
    """Host inputs in NAMES order; about a quarter of the confidences pass Q_CONF."""
    rng = np.random.default_rng(seed)
    idx = [rng.integers(0, max(HW, 1), (B, HW), dtype=np.int64) for _ in range(2)]
    vm = [rng.random((B, HW, 1)) > 0.3 for _ in range(2)]
    Q = [np.exp(rng.standard_normal((B, HW, 1))).astype(np.float32) for _ in range(4)]
    return idx + vm + Q


def _check(backend, m, Q_conf=Q_CONF):
    """Run the op on host inputs, compare with the model; returns the op's host outputs."""
    Qj, Qi, counts = backend.edge_confidence(*_dev(*m), Q_conf)
    rQj, rQi, rcounts = M.edge_confidence(*m, Q_conf)
    B, HW = m[0].shape
    assert Qj.shape == (B, HW, 1) and Qi.shape == (B, HW, 1) and counts.shape == (B, 2)
    assert counts.dtype == torch.int32
    Qj, Qi, counts = Qj.cpu().numpy(), Qi.cpu().numpy(), counts.cpu().numpy().astype(np.int64)
    assert M.same_bits(Qj, rQj) and M.same_bits(Qi, rQi)
    bad = np.nonzero((counts != rcounts).any(axis=1))[0]
    assert bad.size == 0, (bad[:8], counts[bad[:8]], rcounts[bad[:8]])
    return Qj, Qi, counts


# one thread; a partial wave; one chunk short of / exactly / one over a workgroup; ragged chunks
# (per = ceil(HW / chunks), short last chunk); one chunk per pair (B > 2048); 2048 chunks of 257
# of which the last seven are empty (HW = 524300)
EDGE_SHAPES = [(1, 1), (1, 63), (1, 255), (1, 256), (1, 257), (3, 300), (3, 1000), (5, 2049),
               (2100, 70), (1, 524300)]


@pytest.mark.parametrize("B,HW", EDGE_SHAPES)
def test_launch_shapes_against_model(backend, B, HW):
    m = _draw(B, HW, seed=B * 1000003 + HW)
    _, _, counts = _check(backend, m)
    if HW > 1:
        assert counts.sum() > 0
    if B * HW < 100000:
        return
    # the two largest shapes: the only counted pixels of the last pair are the last pixel (j) and
    # the last 20 pixels (i) -- the last lanes of the last chunk that holds any -- so a dropped
    # tail changes the counts
    b = B - 1
    tail = min(20, HW)
    for k in (2, 3):
        m[k][b] = False
    m[2][b, HW - 1] = True
    m[3][b, HW - tail:] = True
    m[0][b, HW - 1] = 5
    m[1][b, HW - tail:] = 7
    m[4][b, 5], m[5][b, 7] = 4.0, 4.0
    m[6][b, HW - 1], m[7][b, HW - tail:] = 4.0, 4.0
    _, _, counts = _check(backend, m)
    assert counts[b].tolist() == [1, tail]


def test_pairs_are_isolated(backend):
    """Pairs 1 and 3 of five pass at every pixel, their neighbours at none; reading a
    neighbour's Qii / Qjj row (or counting into its slot) changes Qj and the counts."""
    B, HW = 5, 300
    m = _draw(B, HW, seed=17)
    rng = np.random.default_rng(18)
    for b in range(B):
        lo, hi = ((4.0, 8.0) if b in (1, 3) else (0.05, 0.1))
        for k in range(4, 8):
            m[k][b] = rng.uniform(lo, hi, (HW, 1)).astype(np.float32)
    m[2][:], m[3][:] = True, True
    _, _, counts = _check(backend, m)
    assert counts.tolist() == [[0, 0], [HW, HW], [0, 0], [HW, HW], [0, 0]]


def _value_lanes(HW=300):
    """B = 2, identity indices; pixel n holds lane n % 16 (direction i: lane (n + 5) % 16), so
    every lane's product is known.  Lanes 14, 15 are ordinary."""
    m = _draw(2, HW, seed=23)
    up = np.nextafter(np.float32(2.25), np.float32(np.inf))
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    #        gathered Q, own Q, valid_match
    lanes = {0: (1.5, 1.5, True),        # product exactly Q_conf**2: sqrt = Q_conf, not counted
             1: (up, 1.0, True),         # the next f32 above: counted
             2: (0.0, 3.0, True),
             3: (-4.0, 4.0, True),       # negative product: NaN, not counted
             4: (nan, 4.0, True),
             5: (inf, 1.0, True),        # Inf: counted
             6: (inf, 0.0, True),        # Inf * 0: NaN
             7: (1e-20, 1e-20, True),    # subnormal product; its sqrt is 1e-20, not 0
             8: (4.0, 4.0, True),        # passes, mask set
             9: (4.0, 4.0, False),       # passes, mask clear
             10: (1.0, 1.0, True),       # fails, mask set
             11: (-4.0, -4.0, True),     # positive product of negatives: counted
             12: (-0.0, 4.0, True),      # -0: sqrt(-0) = -0, not counted
             13: (3.0, 0.75, False)}     # product exactly Q_conf**2 another way, mask clear
    n = np.arange(HW)
    for d, (ki, kg, ko, kv) in enumerate(((0, 4, 6, 2), (1, 5, 7, 3))):
        m[ki][:] = n[None, :]
        lane = (n + 5 * d) % 16
        for k, (g, o, v) in lanes.items():
            m[kg][:, lane == k, 0] = np.float32(g)
            m[ko][:, lane == k, 0] = np.float32(o)
            m[kv][:, lane == k, 0] = v
    return m


def test_threshold_and_values(backend):
    HW = 300
    m = _value_lanes(HW)
    Qj, Qi, counts = _check(backend, m)
    n = np.arange(HW)
    q = Qj[0, :, 0]
    assert np.all(q[n % 16 == 0] == np.float32(1.5))
    assert np.all(q[n % 16 == 1] == np.nextafter(np.float32(1.5), np.float32(2)))
    assert np.all(np.isnan(q[n % 16 == 3])) and np.all(np.isnan(q[n % 16 == 6]))
    assert np.all(q[n % 16 == 7] == np.sqrt(np.float64(np.float32(1e-20) * np.float32(1e-20))).astype(np.float32))
    assert np.all(q[n % 16 == 7] > 0) and np.all(np.isinf(q[n % 16 == 5]))
    # with every other lane's mask cleared the count is exactly lanes 1, 5, 8 and 11
    for d, kv in enumerate((2, 3)):
        lane = (n + 5 * d) % 16
        m[kv][:, lane >= 14, 0] = False
    _, _, counts = _check(backend, m)
    for d in range(2):
        lane = (n + 5 * d) % 16
        assert counts[:, d].tolist() == [int(np.isin(lane, (1, 5, 8, 11)).sum())] * 2


def test_out_of_range_indices_clamp(backend):
    """Indices below 0 read pixel 0 and indices past HW - 1 read pixel HW - 1 of the pair's own
    row; Qii / Qjj sit between canary rows, which never reach the result."""
    B, HW = 3, 300
    m = _draw(B, HW, seed=29)
    rng = np.random.default_rng(30)
    bad = np.array([-1, HW, 2 ** 40, -2 ** 63, -HW, HW + 1, 2 ** 31, 2 ** 32 + 3, -2 ** 32 + 3], np.int64)
    for k in (0, 1):
        pos = rng.permutation(HW)[:4 * len(bad)]
        m[k][:, pos] = np.tile(bad, 4)[None, :]
        m[k][B - 1, HW - 1] = HW  # the last pair's last pixel: one past the whole tensor
        m[k][0, 0] = -1           # the first pair's first pixel: one before it
    for k in (4, 5):  # every pixel's gathered confidence distinct and passing with own Q = 4
        m[k][:] = (2.0 + np.arange(B * HW).reshape(B, HW, 1) / (B * HW)).astype(np.float32)
    m[6][:], m[7][:] = 4.0, 4.0
    m[2][:], m[3][:] = True, True
    d = _dev(*m)
    for k in (4, 5):  # the same values as rows 1..B of a tensor whose other rows are canaries
        big = torch.full((B + 2, HW, 1), 1e30, device=DEV)
        big[1:B + 1] = d[k]
        d[k] = big[1:B + 1]
        assert d[k].is_contiguous()
    Qj, Qi, counts = backend.edge_confidence(*d, Q_CONF)
    rQj, rQi, rcounts = M.edge_confidence(*m, Q_CONF)
    assert M.same_bits(Qj.cpu().numpy(), rQj) and M.same_bits(Qi.cpu().numpy(), rQi)
    assert np.array_equal(counts.cpu().numpy(), rcounts) and rcounts.min() == HW
    # stated directly: -1 gives pixel 0, HW gives pixel HW - 1, of the same pair
    first = np.sqrt(np.float64(m[4][0, 0, 0] * np.float32(4.0))).astype(np.float32)
    last = np.sqrt(np.float64(m[4][B - 1, HW - 1, 0] * np.float32(4.0))).astype(np.float32)
    assert Qj[0, 0, 0].item() == first and Qj[B - 1, HW - 1, 0].item() == last
    assert float(Qj.max()) < 1e3 and float(Qi.max()) < 1e3  # no canary


def test_counts_are_rezeroed_by_every_call(backend):
    """The C entry zeroes counts itself: two calls into the same (dirty) outputs give the counts
    of one call."""
    import ctypes

    B, HW = 3, 1000
    m = _draw(B, HW, seed=37)
    d = _dev(*m)
    Qj = torch.full((B, HW, 1), -1.0, device=DEV)
    Qi = torch.full((B, HW, 1), -1.0, device=DEV)
    counts = torch.full((B, 2), 777, dtype=torch.int32, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rQj, rQi, rcounts = M.edge_confidence(*m, Q_CONF)
    for _ in range(2):
        rc = backend.lib.m3s_edge_confidence(*[p(t) for t in d], Q_CONF, B, HW, p(Qj), p(Qi), p(counts), st)
        assert rc == 0
        assert np.array_equal(counts.cpu().numpy(), rcounts)
        assert M.same_bits(Qj.cpu().numpy(), rQj) and M.same_bits(Qi.cpu().numpy(), rQi)
    # HW = 0 still zeroes the counts of every pair
    counts.fill_(777)
    rc = backend.lib.m3s_edge_confidence(*[p(t) for t in d], Q_CONF, B, 0, p(Qj), p(Qi), p(counts), st)
    assert rc == 0 and counts.cpu().numpy().tolist() == [[0, 0]] * B


def test_empty_batches(backend):
    for B, HW in ((0, 300), (3, 0), (0, 0)):
        m = _draw(B, HW, seed=41)
        Qj, Qi, counts = backend.edge_confidence(*_dev(*m), Q_CONF)
        assert Qj.shape == (B, HW, 1) and Qi.shape == (B, HW, 1)
        assert counts.cpu().numpy().tolist() == [[0, 0]] * B


def test_binding_rejects_bad_arguments(backend):
    B, HW = 3, 300
    m = _draw(B, HW, seed=43)

    def case(**repl):
        a = dict(zip(NAMES, _dev(*m)))
        a.update({k: v(a[k]) for k, v in repl.items()})
        with pytest.raises(RuntimeError):
            backend.edge_confidence(*[a[n] for n in NAMES], Q_CONF)

    for k in ("idx_i2j", "idx_j2i"):
        case(**{k: lambda t: t.int()})
        case(**{k: lambda t: t.cpu()})  # a host tensor among device tensors
        case(**{k: lambda t: t[:, :-1].contiguous()})  # the two index tensors differ in shape
        case(**{k: lambda t: t[:-1].contiguous()})
        case(**{k: lambda t: t.t().contiguous().t()})  # not contiguous
    for k in ("valid_match_j", "valid_match_i"):
        case(**{k: lambda t: t.reshape(B, HW)})
        case(**{k: lambda t: t.to(torch.uint8)})
        case(**{k: lambda t: t.cpu()})
    for k in ("Qii", "Qjj", "Qji", "Qij"):
        case(**{k: lambda t: t.reshape(B, HW)})
        case(**{k: lambda t: t.double()})
        case(**{k: lambda t: t.half()})
        case(**{k: lambda t: t[:, :-1].contiguous()})
        case(**{k: lambda t: t.cpu()})
