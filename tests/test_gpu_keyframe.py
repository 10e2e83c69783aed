"""Keyframe point-map fusion (keyframe.hip via mast3r_slam_backends.pointmap_update and
m3s.frame.Frame.update_pointmap) against the reference's torch expressions
(frame.py:41-105): bit-exact for the per-point arithmetic on identical inputs.

Below the first four tests the op is held to the host model (tests/keyframe_model.py, itself
held to the reference's Frame.update_pointmap by tests/test_keyframe_model.py) and to the
reference's own run (tests/golden/keyframe_golden.npz), at every launch shape:

* without T the three modes are the model's ``fuse`` bit for bit (NaN as NaN), also at 0/0, NaN,
  Inf, negative and subnormal lanes;
* the fused Sim3 transform is within ``act_bound`` = 8 * 2**-24 * (5 |s| ||p|| + max|t|) of the
  float64 transform at every point.  Worst ratio observed on an MI355X over the 14 transforms of
  ``test_transform_within_bound``: 0.1049 of the bound (0.839 of the K = 1 unit; a plain unfused
  f32 restatement reaches 0.97 of the unit on the host);
* the only comparison of the op with itself is the fusion identity (the op with T equals the
  op without T on the "recent"-with-T output, bitwise), and it is stated as such where used;
* ``Frame`` replays the reference's sequences bit for bit; weighted_spherical, a torch
  expression, within 4 times the deviation of the reference's own f32 run from a float64
  evaluation (fixture ``sph_dev``: 0, 5.02e-07, 5.41e-07, 5.80e-07 per call; the factor 4 for the
  device's atan2 / acos / sin / cos being a couple of ulp where the host's are under one; the
  device's own deviation was 0, 5.02e-07, 6.93e-07, 8.35e-07 on an MI355X).
"""
import os

import numpy as np
import pytest
import torch

import keyframe_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "keyframe_golden.npz"))


def _inputs(HW=384 * 512, seed=0):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn((HW, 3), generator=g)
    C = 1.0 + torch.rand((HW, 1), generator=g) * 5
    Xn = torch.randn((HW, 3), generator=g)
    Cn = 1.0 + torch.rand((HW, 1), generator=g) * 5
    return [t.to(DEV) for t in (X, C, Xn, Cn)]


def _T(seed=1):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(4, generator=g)
    q = q / q.norm()
    return torch.cat([torch.randn(3, generator=g) * 0.3, q, torch.tensor([1.1])]).to(DEV)


def _act(T, p):
    t, q, s = T[0:3], T[3:7], T[7]
    u, w = q[:3].expand_as(p), q[3]
    uv = 2.0 * torch.cross(u, p, dim=-1)
    return s * (p + w * uv + torch.cross(u, uv, dim=-1)) + t


def test_weighted_pointmap_bit_exact(backend):
    X, C, Xn, Cn = _inputs()
    ref_X = ((C * X) + (Cn * Xn)) / (C + Cn)  # frame.py:75
    ref_C = C + Cn  # frame.py:76
    backend.pointmap_update("weighted_pointmap", X, C, Xn, Cn)
    assert torch.equal(X, ref_X) and torch.equal(C, ref_C)


def test_indep_conf_and_recent_bit_exact(backend):
    X, C, Xn, Cn = _inputs(seed=3)
    m = Cn > C  # frame.py:70-72
    ref_X, ref_C = X.clone(), C.clone()
    ref_X[m.repeat(1, 3)] = Xn[m.repeat(1, 3)]
    ref_C[m] = Cn[m]
    backend.pointmap_update("indep_conf", X, C, Xn, Cn)
    assert torch.equal(X, ref_X) and torch.equal(C, ref_C)
    backend.pointmap_update("recent", X, C, Xn, Cn)
    assert torch.equal(X, Xn) and torch.equal(C, Cn)


def test_fused_transform(backend):
    X, C, Xn, Cn = _inputs(HW=4096, seed=5)
    T = _T()
    Xt = _act(T, Xn)
    ref_X = ((C * X) + (Cn * Xt)) / (C + Cn)
    X2, C2 = X.clone(), C.clone()
    backend.pointmap_update("weighted_pointmap", X2, C2, Xn, Cn, T)
    torch.testing.assert_close(X2, ref_X, rtol=0, atol=2e-6)
    # with the op's own transform the fusion is exact
    Xo = torch.empty_like(Xn)
    Co = torch.zeros_like(Cn)
    backend.pointmap_update("recent", Xo, Co, Xn, Cn, T)
    torch.testing.assert_close(Xo, Xt, rtol=0, atol=2e-6)
    assert torch.equal(X2, ((C * X) + (Cn * Xo)) / (C + Cn))


def test_frame_update_pointmap_modes():
    from m3s.config import config
    from m3s.frame import Frame

    X, C, Xn, Cn = _inputs(HW=2048, seed=7)
    cfg = {"tracking": dict(config["tracking"], filtering_mode="weighted_pointmap")}
    f = Frame(cfg=cfg)
    f.update_pointmap(X, C)
    assert f.N == 1 and torch.equal(f.X_canon, X)
    f.update_pointmap(Xn, Cn)
    assert f.N == 2 and f.N_updates == 2
    assert torch.equal(f.X_canon, ((C * X) + (Cn * Xn)) / (C + Cn))
    assert torch.equal(f.get_average_conf(), (C + Cn) / 2)
    cfg["tracking"]["filtering_mode"] = "best_score"
    g = Frame(cfg=cfg)
    g.update_pointmap(X, C)
    g.update_pointmap(Xn, Cn)
    better = torch.median(Cn) > torch.median(C)
    assert torch.equal(g.X_canon, Xn if better else X)


# ------------------------------------------------------------------ against the host model

SHAPES = [1, 63, 64, 65, 255, 256, 257, 300, 524288, 524545]  # 524545: 2nd pass + 1-thread block


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _host(t):
    return t.detach().cpu().numpy()


def _draw(HW, seed, span=False):
    """(X, C, Xn, Cn) f32 on the host; a third of the rows have Cn == C exactly.  ``span``:
    point norms spread over 1e-2..1e2."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((HW, 3))
    Xn = rng.standard_normal((HW, 3))
    if span:
        Xn = Xn / np.linalg.norm(Xn, axis=1, keepdims=True) * 10.0 ** rng.uniform(-2, 2, (HW, 1))
    C = (1.0 + 5.0 * rng.random((HW, 1))).astype(np.float32)
    Cn = (1.0 + 5.0 * rng.random((HW, 1))).astype(np.float32)
    tie = np.arange(HW)[:, None] % 3 == 0
    Cn = np.where(tie, C, Cn)
    return X.astype(np.float32), C, Xn.astype(np.float32), Cn


def _sim3(seed, s=1.1, tnorm=0.3, q=None):
    """Sim3 data [t, q(xyzw), s] f32 on the host; random unit q normalised in f32."""
    rng = np.random.default_rng(seed)
    if q is None:
        q = rng.standard_normal(4).astype(np.float32)
        q = q / np.sqrt((q * q).sum(dtype=np.float32))
    t = rng.standard_normal(3)
    t = t / np.linalg.norm(t) * tnorm
    return np.concatenate([t, q, [s]]).astype(np.float32)


def _run(backend, mode, X, C, Xn, Cn, T=None):
    """The op on copies of host arrays -> host (X, C)."""
    dX, dC, dXn, dCn = _dev(X, C, Xn, Cn)
    dT = None if T is None else _dev(T)[0]
    backend.pointmap_update(mode, dX, dC, dXn, dCn, dT)
    return _host(dX), _host(dC)


def _assert_within_bound(got, T, p):
    """|got - act64| <= act_bound at every point; returns the worst ratio."""
    ratio = np.abs(got.astype(np.float64) - M.act64(T, p)) / M.act_bound(T, p)
    assert np.all(ratio <= 1.0), float(ratio.max())
    return float(ratio.max())


@pytest.mark.parametrize("HW", SHAPES)
def test_launch_shapes_against_model(backend, HW):
    X, C, Xn, Cn = _draw(HW, seed=HW)
    T = _sim3(seed=HW + 1)
    # "recent" with T is the transform alone: held to the float64 transform at every point
    Xt, Ct = _run(backend, "recent", X, C, Xn, Cn, T)
    _assert_within_bound(Xt, T, Xn)
    assert M.same_bits(Ct, Cn)
    for mode in M.MODES:
        gX, gC = _run(backend, mode, X, C, Xn, Cn)
        rX, rC = M.fuse(mode, X, C, Xn, Cn)
        assert M.same_bits(gX, rX) and M.same_bits(gC, rC), mode
        # with T: the model fed the transformed observation (fusion identity: the transform
        # inside every mode is the one "recent" applied above, checked against float64 there)
        gX, gC = _run(backend, mode, X, C, Xn, Cn, T)
        rX, rC = M.fuse(mode, X, C, Xt, Cn)
        assert M.same_bits(gX, rX) and M.same_bits(gC, rC), (mode, "T")


@pytest.mark.parametrize("HW", [1, 257, 300, 524545])
def test_untouched_memory(backend, HW):
    """One canary row before and after X and C stays as it was; under indep_conf the rows with
    Cn <= C keep their bits."""
    X, C, Xn, Cn = _draw(HW, seed=7 * HW)
    T = _sim3(seed=3)
    CAN = np.float32(-12345.678)
    for mode in M.MODES:
        for useT in (False, True):
            bigX = torch.full((HW + 2, 3), float(CAN), device=DEV)
            bigC = torch.full((HW + 2, 1), float(CAN), device=DEV)
            dX, dC = bigX[1:HW + 1], bigC[1:HW + 1]
            dX.copy_(torch.from_numpy(X))
            dC.copy_(torch.from_numpy(C))
            dXn, dCn = _dev(Xn, Cn)
            backend.pointmap_update(mode, dX, dC, dXn, dCn, _dev(T)[0] if useT else None)
            for big in (bigX, bigC):
                assert bool((big[0] == float(CAN)).all()) and bool((big[-1] == float(CAN)).all()), mode
            if mode == "indep_conf":
                keep = (Cn <= C)[:, 0]
                assert keep.sum() >= HW // 3
                assert M.same_bits(_host(dX)[keep], X[keep]) and M.same_bits(_host(dC)[keep], C[keep])
            if not useT:
                rX, rC = M.fuse(mode, X, C, Xn, Cn)
                assert M.same_bits(_host(dX), rX) and M.same_bits(_host(dC), rC)


def _edge_values(HW=300):
    """Rows n with n % 16 == k hold lane k's confidences (and, for the subnormal lanes, points);
    lanes 14 and 15 are ordinary."""
    X, C, Xn, Cn = _draw(HW, seed=11)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    lanes = {
        0: (0.0, 0.0),            # 0 / 0
        1: (0.0, 2.0),
        2: (2.0, nan),
        3: (nan, 2.0),
        4: (2.0, inf),
        5: (inf, inf),
        6: (1e-20, 1e-20),        # C X and Cn Xn subnormal (points below)
        7: (1.0, 2.0),            # subnormal inputs, products and quotient
        8: (3.0, 100.0),          # normal sum, subnormal quotient
        9: (2.5, 2.5),            # Cn == C
        10: (-1.0, 3.0),
        11: (2.0, -2.0),          # den = 0 with a non-zero numerator
        12: (-1.0, -3.0),
        13: (-0.0, 0.0),
    }
    pts = {6: (3e-20, 5e-20), 7: (1e-39, 3e-39), 8: (2e-38, 1e-38)}
    n = np.arange(HW)
    for k, (c, cn) in lanes.items():
        C[n % 16 == k, 0] = np.float32(c)
        Cn[n % 16 == k, 0] = np.float32(cn)
    for k, (x, xn) in pts.items():
        sign = np.where(np.random.default_rng(k).random((int((n % 16 == k).sum()), 3)) < 0.5, -1, 1)
        X[n % 16 == k] = np.float32(x) * sign
        Xn[n % 16 == k] = np.float32(xn) * sign
    return X, C, Xn, Cn


def test_edge_values_against_model(backend):
    X, C, Xn, Cn = _edge_values()
    # the lanes are what they claim (f32 host arithmetic keeps subnormals)
    tiny = np.finfo(np.float32).tiny
    rX, rC = M.fuse("weighted_pointmap", X, C, Xn, Cn)
    n = np.arange(len(C))
    assert np.all(np.isnan(rX[n % 16 == 0])) and np.all(np.isnan(rX[n % 16 == 5]))
    assert np.all(np.isinf(rX[n % 16 == 11]))
    with np.errstate(all="ignore"):
        p6 = np.abs((C * X)[n % 16 == 6])
    assert np.all((p6 > 0) & (p6 < tiny))
    for k in (7, 8):
        assert np.all((np.abs(rX[n % 16 == k]) > 0) & (np.abs(rX[n % 16 == k]) < tiny)), k
    T = _sim3(seed=2)
    Xt, _ = _run(backend, "recent", X, C, Xn, Cn, T)
    for mode in M.MODES:
        gX, gC = _run(backend, mode, X, C, Xn, Cn)
        rX, rC = M.fuse(mode, X, C, Xn, Cn)
        bad = [int(k) for k in range(16) if not (M.same_bits(gX[n % 16 == k], rX[n % 16 == k])
                                                  and M.same_bits(gC[n % 16 == k], rC[n % 16 == k]))]
        assert not bad, (mode, "lanes", bad)
        # the same lanes with the transform fused in (fusion identity on the observation)
        gX, gC = _run(backend, mode, X, C, Xn, Cn, T)
        rX, rC = M.fuse(mode, X, C, Xt, Cn)
        assert M.same_bits(gX, rX) and M.same_bits(gC, rC), (mode, "T")


TRANSFORMS = [(s, t) for s in (0.05, 1.0, 1.1, 20.0) for t in (0.0, 0.3, 50.0)]


def test_transform_within_bound(backend):
    """The fused transform ("recent" with T) against the float64 transform, every point, over
    12 random rotations (every s with every |t|) and the exact rotations q = (0,0,0,1) and
    (1,0,0,0) (half a turn about x)."""
    HW = 300
    X, C, Xn, Cn = _draw(HW, seed=21, span=True)
    norms = np.linalg.norm(Xn, axis=1)
    assert norms.min() < 2e-2 and norms.max() > 50
    draws = [_sim3(seed=40 + k, s=s, tnorm=t) for k, (s, t) in enumerate(TRANSFORMS)]
    for q in ((0, 0, 0, 1), (1, 0, 0, 0)):
        draws.append(_sim3(seed=60, s=1.1, tnorm=0.3, q=np.float32(q)))
    worst = 0.0
    for T in draws:
        gX, gC = _run(backend, "recent", X, C, Xn, Cn, T)
        r = _assert_within_bound(gX, T, Xn)
        print(f"s={T[7]:g} |t|={np.linalg.norm(T[:3]):.3g} q={T[3:7]}: worst ratio to act_bound {r:.4f}")
        worst = max(worst, r)
        assert M.same_bits(gC, Cn)
    print(f"worst ratio |op - act64| / act_bound over {len(draws)} transforms: {worst:.4f} "
          f"(= {worst * M.ACT_K:.3f} of the K=1 unit)")
    # half a turn about x with s = 1, t = 0 flips y and z; the identity returns the points by
    # value (== : -0 may become +0)
    flip = np.float32([0, 0, 0, 1, 0, 0, 0, 1])
    gX, _ = _run(backend, "recent", X, C, Xn, Cn, flip)
    assert np.array_equal(gX, Xn * np.float32([1, -1, -1]))
    ident = np.float32([0, 0, 0, 0, 0, 0, 1, 1])
    Xz = Xn.copy()
    Xz[::7] = np.float32([0.0, -0.0, 1.0])
    gX, _ = _run(backend, "recent", X, C, Xz, Cn, ident)
    assert np.array_equal(gX, Xz)
    for mode in M.MODES:
        gX, gC = _run(backend, mode, X, C, Xn, Cn, ident)
        rX, rC = M.fuse(mode, X, C, Xn, Cn)
        assert np.array_equal(gX, rX) and np.array_equal(gC, rC), mode


@pytest.mark.parametrize("HW", [300, 524545])
def test_fusion_identity_every_mode(backend, HW):
    """Fusion identity (the one comparison of the op with itself): the op with T is bitwise the
    op without T given the "recent"-with-T output as the observation."""
    X, C, Xn, Cn = _draw(HW, seed=HW + 5, span=True)
    T = _sim3(seed=9, s=0.7, tnorm=2.0)
    Xt, _ = _run(backend, "recent", X, C, Xn, Cn, T)
    for mode in M.MODES:
        aX, aC = _run(backend, mode, X, C, Xn, Cn, T)
        bX, bC = _run(backend, mode, X, C, Xt, Cn)
        assert M.same_bits(aX, bX) and M.same_bits(aC, bC), mode


# ------------------------------------------------------------------ Frame against the fixture


def _frame(mode, score):
    from m3s.config import config
    from m3s.frame import Frame

    return Frame(cfg={"tracking": dict(config["tracking"], filtering_mode=mode, filtering_score=score)})


def _sph_fuse64(X, C, Xn, Cn):
    """frame.py:78-102 in float64."""
    def to_sph(P):
        r = np.sqrt((P * P).sum(axis=-1, keepdims=True))
        return np.concatenate((r, np.arctan2(P[:, 1:2], P[:, 0:1]), np.arccos(P[:, 2:3] / r)), axis=-1)

    s = ((C * to_sph(X)) + (Cn * to_sph(Xn))) / (C + Cn)
    r, phi, theta = s[:, 0:1], s[:, 1:2], s[:, 2:3]
    return np.concatenate((r * np.sin(theta) * np.cos(phi), r * np.sin(theta) * np.sin(phi),
                           r * np.cos(theta)), axis=-1), C + Cn


@pytest.mark.parametrize("k", range(len(GOLD["names"])), ids=[str(n) for n in GOLD["names"]])
def test_frame_replays_reference_sequence(k):
    name, mode, score = (str(GOLD[a][k]) for a in ("names", "modes", "scores"))
    f = _frame(mode, score)
    g = lambda key: GOLD[f"{name}_{key}"]
    X64 = C64 = None
    for c in range(int(GOLD["ncalls"])):
        X, C = _dev(g("X")[c], g("C")[c])
        X0, C0 = X.clone(), C.clone()
        f.update_pointmap(X, C)
        assert torch.equal(X, X0) and torch.equal(C, C0)  # the observation is not written
        assert f.N == int(g("N")[c]) and f.N_updates == int(g("N_updates")[c]), (name, c)
        assert M.same_bits(_host(f.C), g("C_canon")[c]), (name, c)
        assert M.same_bits(_host(f.get_average_conf()), g("avg_conf")[c]), (name, c)
        if mode == "weighted_spherical":
            Xd, Cd = g("X")[c].astype(np.float64), g("C")[c].astype(np.float64)
            X64, C64 = (Xd, Cd) if c == 0 else _sph_fuse64(X64, C64, Xd, Cd)
            dev_ref = float(GOLD["sph_dev"][c])
            # the fixture's deviation is what the generator measured against the same float64 chain
            # (to float64 rounding: another host's libm may differ in the last bit)
            assert abs(np.abs(g("X_canon")[c].astype(np.float64) - X64).max() - dev_ref) <= 1e-12
            dev = np.abs(_host(f.X_canon).astype(np.float64) - X64).max()
            print(f"weighted_spherical call {c}: device deviation {dev:.3e}, reference's {dev_ref:.3e}")
            assert dev <= 4.0 * dev_ref, (c, dev, dev_ref)
            continue
        assert M.same_bits(_host(f.X_canon), g("X_canon")[c]), (name, c)
        if mode == "best_score":
            replaced = c == 0 or np.array_equal(_host(f.X_canon), g("X")[c])
            assert replaced == bool(g("replaced")[c]), (name, c)
            ref = float(g("score")[c])
            if score == "median":
                assert float(f.score) == ref
            else:
                # each side is a sum of HW positive f32 terms in its own order and one divide:
                # within HW * 2**-24 (relative) of the exact mean, so within twice that of each other
                assert abs(float(f.score) - ref) <= 2 * len(C) * 2.0 ** -24 * ref


def test_frame_weighted_pointmap_with_transform(backend):
    """update_pointmap(X, C, T=...) over the weighted_pointmap sequence, the first call (the
    transformed copy) included: the model fed the transformed observations.  Fusion identity: the
    observation is "recent"-with-T's output, itself held to the float64 transform here."""
    f = _frame("weighted_pointmap", "median")
    rX = rC = None
    for c in range(int(GOLD["ncalls"])):
        X, C = GOLD["weighted_pointmap_X"][c], GOLD["weighted_pointmap_C"][c]
        T = _sim3(seed=70 + c, s=(0.8, 1.0, 1.3, 2.0)[c], tnorm=(0.0, 0.3, 1.0, 5.0)[c])
        Xt, _ = _run(backend, "recent", X, C, X, C, T)
        _assert_within_bound(Xt, T, X)
        dX, dC, dT = _dev(X, C, T.reshape(1, 8))
        f.update_pointmap(dX, dC, T=dT)
        rX, rC = (Xt, C) if c == 0 else M.fuse("weighted_pointmap", rX, rC, Xt, C)
        assert f.N == c + 1 and f.N_updates == c + 1
        assert M.same_bits(_host(f.X_canon), rX) and M.same_bits(_host(f.C), rC), c
        assert M.same_bits(_host(f.get_average_conf()), rC / np.float32(c + 1)), c


# ------------------------------------------------------------------ the binding's checks


def test_binding_rejects_bad_arguments(backend):
    HW = 300
    X, C, Xn, Cn = _draw(HW, seed=31)
    dT = _dev(_sim3(seed=1))[0]

    def case(mode="weighted_pointmap", T=None, **repl):
        a = dict(zip(("X", "C", "Xn", "Cn"), _dev(X, C, Xn, Cn)))
        keepX, keepC = a["X"], a["C"]
        a.update({k: v(a[k]) for k, v in repl.items()})
        with pytest.raises(RuntimeError):
            backend.pointmap_update(mode, a["X"], a["C"], a["Xn"], a["Cn"], T)
        assert M.same_bits(_host(keepX), X) and M.same_bits(_host(keepC), C), (mode, sorted(repl))

    case(mode="weighted_spherical")
    case(mode="nearest")
    for k in ("X", "C", "Xn", "Cn"):
        case(**{k: lambda t: t.double()})
        case(**{k: lambda t: t.half()})
        case(**{k: lambda t: t.cpu()})  # a host tensor among device tensors
    case(C=lambda t: t.reshape(-1))
    case(Cn=lambda t: t.reshape(-1))
    case(Xn=lambda t: t[:-1].contiguous())
    case(Cn=lambda t: t[:-1].contiguous())
    case(X=lambda t: t.t().contiguous().t())  # [HW,3] with strides (1, HW)
    case(Xn=lambda t: t.repeat(1, 2)[:, :3])
    case(T=dT[:7].contiguous())
    case(T=dT.double())
    case(T=dT.cpu())


def test_empty_point_map(backend):
    z3, z1 = torch.empty((0, 3), device=DEV), torch.empty((0, 1), device=DEV)
    for mode in M.MODES:
        for T in (None, _dev(_sim3(seed=1))[0]):
            X, C = backend.pointmap_update(mode, z3, z1, z3.clone(), z1.clone(), T)
            assert X.shape == (0, 3) and C.shape == (0, 1)
