"""Head finish (head.hip via mast3r_slam_backends.head_finish and m3s.mast3r_utils) against the
host model (tests/head_model.py): D bit for bit with the f32 model, X, C, Q inside the derived
bounds of the f64 model, and the reference's own outputs (tests/golden/head_golden.npz).  Shapes
are the smallest at which the indexing can go wrong: a 2x3 token grid (row and column token index
differ), two batch items (batch stride), strides that leave partial patches and unaligned runs,
the compile-time (F = 24) and run-time descriptor widths, 16-byte and 4-byte D stores."""
import functools
import os

import numpy as np
import pytest
import torch

import head_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("X", "C", "D", "Q")
INF = float("inf")


@functools.lru_cache(maxsize=None)
def gold():
    g = np.load(os.path.join(HERE, "golden", "head_golden.npz"))
    return dict(g=g, T1=M.tol(g["T_expm1"]), T=M.tol(g["T_exp"]))


@functools.lru_cache(maxsize=None)
def case(B=2, H=32, W=48, F=24, seed=1):
    """Raw heads (host f32 arrays, made once and left unchanged)."""
    pts, planar = M.make_inputs(B, H, W, F, seed)
    feat = M.unshuffle(planar) if H % 16 == 0 and W % 16 == 0 else None
    return dict(pts=pts, planar=planar, feat=feat, F=F)


@functools.lru_cache(maxsize=None)
def models(key, ds):
    c = case(*key)
    return M.model_f32(c["pts"], c["planar"], ds), M.model_f64(c["pts"], c["planar"], ds)


def dev(a):
    return torch.from_numpy(a).to(DEV)


def run(c, layout, ds=1, **kw):
    import mast3r_slam_backends as mb

    f = c["feat"] if layout == "tokens" else c["planar"]
    out = mb.head_finish(dev(c["pts"]), dev(f), layout=layout, downsample=ds, **kw)
    return [o.cpu().numpy() for o in out]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_against_models(got, pts, m32, m64, ds, F):
    """D: the f32 model's bits (NaN where it has NaN).  X, C, Q: NaN / inf positions and signs the
    f32 model's; where that is finite, inside the bounds of the f64 model."""
    G = gold()
    dn = M.norm_f64(pts, ds)[..., None]
    bds = (M.bound_X(dn, G["T1"]), M.bound_CQ(G["T"]), M.bound_D(F), M.bound_CQ(G["T"]))
    worst = {}
    for n, a, s, d, bd in zip(NAMES, got, m32, m64, bds):
        assert a.shape == s.shape and a.dtype == np.float32, n
        assert M.same_specials(a, s), n
        fin = np.isfinite(s)
        e = M.rel_err_u(a, d)
        worst[n] = float(e[fin].max()) if fin.any() else 0.0
        assert np.all((e * M.U <= np.broadcast_to(bd, a.shape))[fin]), (n, worst[n])
    nan = np.isnan(m32[2])
    assert np.array_equal(bits(got[2])[~nan], bits(m32[2])[~nan]), "D differs from the f32 model"
    print("worst distance from the f64 model [u]:", {k: round(v, 2) for k, v in worst.items()})


@pytest.mark.parametrize("ds", [1, 2])
def test_layouts_and_downsample(ds):
    c = case()
    tok, pla = run(c, "tokens", ds), run(c, "planar", ds)
    m32, m64 = models((), ds)
    check_against_models(tok, c["pts"], m32, m64, ds, c["F"])
    for n, a, b in zip(NAMES, tok, pla):
        assert np.array_equal(bits(a), bits(b)), f"{n}: tokens and planar differ"


@pytest.mark.parametrize("ds", [1, 2])
def test_golden(ds):
    """Kernel against the reference's outputs: the kernel's bound plus the reference's."""
    G = gold()
    g = G["g"]
    pts, feat, F = g["pts"], g["feat"], int(g["F"])
    planar = M.shuffle(feat, pts.shape[2], pts.shape[3])
    got = run(dict(pts=pts, feat=feat, planar=planar), "tokens", ds)
    m32, m64 = M.model_f32(pts, planar, ds), M.model_f64(pts, planar, ds)
    check_against_models(got, pts, m32, m64, ds, F)
    dn = M.norm_f64(pts, ds)[..., None]
    bds = (M.bound_X(dn, G["T1"]), M.bound_CQ(G["T"]), M.bound_D(F), M.bound_CQ(G["T"]))
    for n, a, d, bd in zip(NAMES, got, m64, bds):
        ref = g[f"ds{ds}_{n}"].astype(np.float64)
        assert np.all(np.abs(a - ref) <= 2 * bd * np.abs(d)), n


def test_special_points():
    c = case(1, 32, 48, 24, 2)
    pts, planar = c["pts"].copy(), c["planar"].copy()
    F = 24
    pts[0, :3, 0, 0] = 0.0                       # X = 0
    pts[0, :3, 0, 1] = (1e-9, 0.0, 0.0)          # the clip branch: m = 1e-8
    pts[0, :3, 0, 2] = (100.0, 0.0, 0.0)         # expm1 overflows: (inf, 0 inf, 0 inf)
    pts[0, :3, 0, 3] = (-60.0, 80.0, 0.0)        # d = 100: (-inf, inf, NaN)
    pts[0, :3, 17, 20] = (np.nan, 1.0, 1.0)      # NaN in, NaN out
    planar[0, :F, 1, 0] = 0.0                    # 0 / 0: F NaNs
    pts[0, 3, 1, 1], planar[0, F, 1, 1] = 100.0, 100.0      # exp overflows
    pts[0, 3, 1, 2], planar[0, F, 1, 2] = -np.inf, -np.inf  # exp = 0: vmin
    pts[0, 3, 31, 47], planar[0, F, 31, 47] = np.nan, np.nan
    cc = dict(pts=pts, planar=planar, feat=M.unshuffle(planar))
    m32, m64 = M.model_f32(pts, planar), M.model_f64(pts, planar)
    for layout in ("tokens", "planar"):
        X, C, D, Q = got = run(cc, layout)
        check_against_models(got, pts, m32, m64, 1, F)
        assert np.all(X[0, 0, 0] == 0.0)
        assert abs(X[0, 0, 1, 0] / 1e-10 - 1.0) < 1e-5 and np.all(X[0, 0, 1, 1:] == 0.0)
        assert X[0, 0, 2, 0] == INF and np.isnan(X[0, 0, 2, 1:]).all()
        assert X[0, 0, 3, 0] == -INF and X[0, 0, 3, 1] == INF and np.isnan(X[0, 0, 3, 2])
        assert np.isnan(X[0, 17, 20]).all() and np.isnan(X).sum() == 3 + 3
        assert np.isnan(D[0, 1, 0]).all() and np.isnan(D).sum() == F
        assert C[0, 1, 1] == INF and Q[0, 1, 1] == INF
        assert C[0, 1, 2] == 1.0 and Q[0, 1, 2] == 0.0
        assert np.isnan(C[0, 31, 47]) and np.isnan(Q[0, 31, 47])
        assert np.isnan(C).sum() == 1 and np.isnan(Q).sum() == 1


def test_strided_views():
    """pts and feat as views of one [B,29,H,W] tensor: the batch stride is not the item size."""
    import mast3r_slam_backends as mb

    c = case()
    raw = dev(np.concatenate([c["pts"], c["planar"]], axis=1))
    assert raw.shape[1] == 29
    got = mb.head_finish(raw[:, :4], raw[:, 4:], layout="planar")
    ref = mb.head_finish(raw[:, :4].contiguous(), raw[:, 4:].contiguous(), layout="planar")
    for n, a, b in zip(NAMES, got, ref):
        assert np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy())), n
    check_against_models([o.cpu().numpy() for o in got], c["pts"], *models((), 1), 1, 24)


def test_out_slices():
    import mast3r_slam_backends as mb

    c = case(1, 32, 48, 24, 3)
    pts, feat = dev(c["pts"]), dev(c["feat"])
    plain = mb.head_finish(pts, feat, downsample=2)
    S = -777.0
    stack = [torch.full((4, 16, 24) + tail, S, device=DEV) for tail in ((3,), (), (24,), ())]
    ret = mb.head_finish(pts, feat, downsample=2, out=tuple(t[1:2] for t in stack))
    for n, t, r, p in zip(NAMES, stack, ret, plain):
        assert r.data_ptr() == t[1:2].data_ptr(), n
        assert torch.equal(t[1:2], p), n
        assert bool((t[0] == S).all()) and bool((t[2:] == S).all()), f"{n}: wrote outside its slot"
    # without feat, D and Q are not touched
    stack = [torch.full((4, 16, 24) + tail, S, device=DEV) for tail in ((3,), (), (24,), ())]
    X, C, D, Q = mb.head_finish(pts, None, downsample=2, out=tuple(t[1:2] for t in stack))
    assert D is None and Q is None
    assert torch.equal(stack[0][1:2], plain[0]) and torch.equal(stack[1][1:2], plain[1])
    assert bool((stack[2] == S).all()) and bool((stack[3] == S).all())
    X, C, D, Q = mb.head_finish(pts, None, downsample=2)
    assert D is None and Q is None and torch.equal(X, plain[0]) and torch.equal(C, plain[1])


def test_downsample_3_is_a_slice():
    """16 % 3 != 0: the kept pixels sit at a different phase in every patch."""
    c = case()
    full = run(c, "tokens", 1)
    for layout in ("tokens", "planar"):
        third = run(c, layout, 3)
        for n, a, b in zip(NAMES, full, third):
            assert b.shape[1:3] == (11, 16), n
            assert np.array_equal(bits(a[:, ::3, ::3]), bits(b)), (layout, n)


ODD = {
    # name: (B, H, W, F, seed), layout, ds
    "grid4x5": ((1, 64, 80, 24, 5), "tokens", 1),
    "grid4x5_planar_ds2": ((1, 64, 80, 24, 5), "planar", 2),
    "F16_generic": ((2, 32, 48, 16, 6), "tokens", 1),
    "F16_planar_ds2": ((2, 32, 48, 16, 6), "planar", 2),
    "F5_scalar_stores": ((2, 32, 48, 5, 7), "tokens", 1),
    "F32_widest": ((1, 32, 32, 32, 8), "tokens", 1),
    "F1": ((1, 16, 32, 1, 9), "planar", 1),
    "partial_patches": ((2, 20, 27, 24, 10), "planar", 1),
    "partial_patches_ds5": ((2, 37, 21, 7, 11), "planar", 5),
    "ds_past_the_image": ((1, 16, 32, 24, 12), "tokens", 40),
}


@pytest.mark.parametrize("name", sorted(ODD))
def test_odd_sizes(name):
    key, layout, ds = ODD[name]
    c = case(*key)
    got = run(c, layout, ds)
    m32, m64 = models(key, ds)
    check_against_models(got, c["pts"], m32, m64, ds, c["F"])


def test_unaligned_D_takes_the_scalar_stores():
    """A D buffer that is 4- but not 16-byte aligned gives the same bytes."""
    import mast3r_slam_backends as mb

    c = case()
    pts, feat = dev(c["pts"]), dev(c["feat"])
    plain = mb.head_finish(pts, feat)
    n = plain[2].numel()
    store = torch.full((n + 8,), -1.0, device=DEV)
    D = store[1:1 + n].view(plain[2].shape)
    assert D.data_ptr() % 16 == 4
    out = (torch.empty_like(plain[0]), torch.empty_like(plain[1]), D, torch.empty_like(plain[3]))
    mb.head_finish(pts, feat, out=out)
    for n_, a, b in zip(NAMES, out, plain):
        assert torch.equal(a, b) or np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy())), n_
    assert float(store[0]) == -1.0 and bool((store[1 + n:] == -1.0).all())


def test_conf_bounds_are_applied():
    """Finite (vmin, vmax): clip(exp(a), max = vmax - vmin) + vmin in f32."""
    c = case()
    X, C, D, Q = run(c, "tokens", 1, conf=(1.0, 3.0), desc_conf=(0.5, 2.5))
    m32 = M.model_f32(c["pts"], c["planar"], 1, (1.0, 3.0), (0.5, 2.5))
    m64 = M.model_f64(c["pts"], c["planar"], 1, (1.0, 3.0), (0.5, 2.5))
    assert C.max() == 3.0 and Q.max() == 2.5 and (C == 3.0).sum() > 10 and (C < 3.0).sum() > 10
    for a, s, d in ((C, m32[1], m64[1]), (Q, m32[3], m64[3])):
        assert np.all(M.rel_err_u(a, d) * M.U <= M.bound_CQ(gold()["T"]))


def test_postprocess_torch_on_device_within_bounds_of_kernel():
    from m3s.mast3r_utils import postprocess_torch, shuffle_tokens

    G = gold()
    c = case()
    pts, feat = dev(c["pts"]), dev(c["feat"])
    for ds in (1, 2):
        ref = postprocess_torch(torch.cat([pts, shuffle_tokens(feat, 32, 48)], dim=1), 24, downsample=ds)
        got = run(c, "tokens", ds)
        m64 = models((), ds)[1]
        dn = M.norm_f64(c["pts"], ds)[..., None]
        bds = (M.bound_X(dn, G["T1"]), M.bound_CQ(G["T"]), M.bound_D(24), M.bound_CQ(G["T"]))
        for n, a, r, d, bd in zip(NAMES, got, ref, m64, bds):
            r = r.cpu().numpy().astype(np.float64)
            assert r.shape == a.shape, n
            assert np.all(np.abs(a - r) <= 2 * bd * np.abs(d)), (n, ds)


@functools.lru_cache(maxsize=None)
def four_heads():
    """ii, ji, jj, ij at 48x64: (pts, feat) on the device."""
    heads = []
    for k in range(4):
        c = case(1, 48, 64, 24, 30 + k)
        heads.append((dev(c["pts"]), dev(c["feat"])))
    return heads


def _match_by_hand(h1, h2):
    import mast3r_slam_backends as mb
    from m3s.config import DEFAULT_CONFIG

    m = DEFAULT_CONFIG["matching"]
    X1, C1, D1, Q1 = mb.head_finish(*h1)
    X2, C2, D2, Q2 = mb.head_finish(*h2)
    idx, valid = mb.match_iterative_proj(X1, X2, D1, D2, None, m["max_iter"], m["lambda_init"],
                                         m["convergence_thresh"], m["dist_thresh"], m["radius"],
                                         m["dilation_max"])
    return idx, valid, (X1, C1, Q1), (X2, C2, Q2)


def test_glue_asymmetric_and_mono():
    from m3s import mast3r_utils as U
    from m3s.config import DEFAULT_CONFIG

    ii, ji, jj, ij = four_heads()
    hw = 48 * 64
    out = U.mast3r_match_asymmetric_raw(ii, ji, cfg=DEFAULT_CONFIG)
    assert len(out) == 8
    idx_i2j, valid_match_j, Xii, Cii, Qii, Xji, Cji, Qji = out
    assert idx_i2j.shape == (1, hw) and idx_i2j.dtype == torch.int64
    assert valid_match_j.shape == (1, hw, 1) and valid_match_j.dtype == torch.bool
    for t, last in ((Xii, 3), (Cii, 1), (Qii, 1), (Xji, 3), (Cji, 1), (Qji, 1)):
        assert t.shape == (hw, last) and t.dtype == torch.float32
    idx, valid, (X1, C1, Q1), (X2, C2, Q2) = _match_by_hand(ii, ji)
    assert torch.equal(idx_i2j, idx) and torch.equal(valid_match_j, valid)
    assert torch.equal(Xii, X1.view(hw, 3)) and torch.equal(Cji, C2.view(hw, 1))
    assert torch.equal(Qii, Q1.view(hw, 1)) and torch.equal(Xji, X2.view(hw, 3))
    # a warm start is passed through
    out2 = U.mast3r_match_asymmetric_raw(ii, ji, idx_i2j_init=idx_i2j, cfg=DEFAULT_CONFIG)
    assert out2[0].shape == (1, hw) and torch.equal(out2[2], Xii)
    Xm, Cm = U.mast3r_inference_mono_raw(ii, cfg=DEFAULT_CONFIG)
    assert torch.equal(Xm, Xii) and torch.equal(Cm, Cii)


def test_glue_symmetric_feeds_add_matched_factors():
    from m3s import mast3r_utils as U
    from m3s.config import DEFAULT_CONFIG
    from m3s.global_opt import FactorGraph

    ii, ji, jj, ij = four_heads()
    hw = 48 * 64
    out = U.mast3r_match_symmetric_raw(ii, ji, jj, ij, cfg=DEFAULT_CONFIG)
    assert len(out) == 8
    for t in out[:2]:
        assert t.shape == (1, hw) and t.dtype == torch.int64
    for t in out[2:4]:
        assert t.shape == (1, hw, 1) and t.dtype == torch.bool
    for t in out[4:]:
        assert t.shape == (1, hw, 1) and t.dtype == torch.float32
    idx_i2j, idx_j2i, valid_match_j, valid_match_i, Qii, Qjj, Qji, Qij = out
    a_idx, a_valid, (_, _, Q_ii), (_, _, Q_ji) = _match_by_hand(ii, ji)   # X11 = [ii; jj]
    b_idx, b_valid, (_, _, Q_jj), (_, _, Q_ij) = _match_by_hand(jj, ij)   # X21 = [ji; ij]
    assert torch.equal(idx_i2j, a_idx) and torch.equal(valid_match_j, a_valid)
    assert torch.equal(idx_j2i, b_idx) and torch.equal(valid_match_i, b_valid)
    assert not torch.equal(a_idx, b_idx)
    for got, want in ((Qii, Q_ii), (Qjj, Q_jj), (Qji, Q_ji), (Qij, Q_ij)):
        assert torch.equal(got, want.view(1, hw, 1))
    # swapping the two frames swaps the halves
    swapped = U.mast3r_match_symmetric_raw(jj, ij, ii, ji, cfg=DEFAULT_CONFIG)
    for k, j in ((0, 1), (1, 0), (2, 3), (3, 2), (4, 5), (5, 4), (6, 7), (7, 6)):
        assert torch.equal(swapped[k], out[j]), (k, j)
    # two pairs at once: each raw head [2,...]
    both = lambda a, b: (torch.cat([a[0], b[0]]), torch.cat([a[1], b[1]]))
    two = U.mast3r_match_symmetric_raw(both(ii, jj), both(ji, ij), both(jj, ii), both(ij, ji),
                                       cfg=DEFAULT_CONFIG)
    for k, j in enumerate((1, 0, 3, 2, 5, 4, 7, 6)):
        assert two[k].shape[0] == 2
        assert torch.equal(two[k][0:1], out[k]) and torch.equal(two[k][1:2], out[j]), k

    fg = FactorGraph(None, None, device=DEV, cfg=DEFAULT_CONFIG)
    assert fg.add_matched_factors([0], [1], *out, 0.0) is True
    assert fg.ii.tolist() == [0] and fg.jj.tolist() == [1]
    assert torch.equal(fg.idx_ii2jj, idx_i2j) and torch.equal(fg.idx_jj2ii, idx_j2i)
    assert fg.Q_ii2jj.shape == (1, hw, 1) and fg.Q_jj2ii.shape == (1, hw, 1)


def test_finish_heads_uses_config_downsample():
    from m3s import mast3r_utils as U
    from m3s.config import DEFAULT_CONFIG
    import copy
    import mast3r_slam_backends as mb

    ii, ji, _, _ = four_heads()
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["dataset"]["img_downsample"] = 2
    X, C, D, Q = U.finish_heads([ii, ji], cfg=cfg)
    assert X.shape == (2, 24, 32, 3) and D.shape == (2, 24, 32, 24)
    for k, h in enumerate((ii, ji)):
        for a, b in zip((X, C, D, Q), mb.head_finish(*h, downsample=2)):
            assert torch.equal(a[k:k + 1], b)


def test_errors_and_repeatability():
    import mast3r_slam_backends as mb

    c = case()
    pts, feat, planar = dev(c["pts"]), dev(c["feat"]), dev(c["planar"])
    zeros = lambda *s: torch.zeros(s, device=DEV)
    bad = [  # (call, a word of the message it must raise)
        (lambda: mb.head_finish(pts.cpu(), feat), "HIP"),                      # CPU tensors
        (lambda: mb.head_finish(pts, feat.cpu()), "HIP"),
        (lambda: mb.head_finish(pts.double(), feat), "Float"),                 # dtype
        (lambda: mb.head_finish(pts, feat.half()), "Float"),
        (lambda: mb.head_finish(pts.transpose(2, 3), feat), "contiguous"),     # inner layout
        (lambda: mb.head_finish(pts, planar[:, :, :, ::2], layout="planar"), "contiguous"),
        (lambda: mb.head_finish(pts, feat.transpose(1, 2)), "contiguous"),
        (lambda: mb.head_finish(pts[:, :3], feat), "must be"),                 # not 4 channels
        (lambda: mb.head_finish(pts[0], feat), "dims"),
        (lambda: mb.head_finish(zeros(2, 4, 24, 48), feat), "multiples of"),   # H % patch, tokens
        (lambda: mb.head_finish(zeros(2, 4, 32, 40), feat), "multiples of"),   # W % patch, tokens
        (lambda: mb.head_finish(pts, zeros(2, 6, 256)), "F must be"),          # F = 0
        (lambda: mb.head_finish(pts, zeros(2, 6, 34 * 256)), "F must be"),     # F = 33
        (lambda: mb.head_finish(pts, zeros(2, 34, 32, 48), layout="planar"), "F must be"),
        (lambda: mb.head_finish(pts, zeros(2, 6, 25 * 256 + 1)), "feat must be"),
        (lambda: mb.head_finish(pts, feat[:, :5]), "feat must be"),            # token count
        (lambda: mb.head_finish(pts, feat[:1]), "feat must be"),               # batch
        (lambda: mb.head_finish(pts, zeros(2, 25, 16, 48), layout="planar"), "feat must be"),
        (lambda: mb.head_finish(pts, feat, layout="nhwc"), "layout"),
        (lambda: mb.head_finish(pts, feat, patch=8), "patch"),
        (lambda: mb.head_finish(pts, feat, downsample=0), "downsample"),
    ]
    good = mb.head_finish(pts, feat, downsample=2)
    mk = lambda: [torch.empty_like(t) for t in good]

    def with_out(k, t):
        def f():
            out = mk()
            out[k] = t
            mb.head_finish(pts, feat, downsample=2, out=tuple(out))
        return f

    for k, shape in enumerate(((2, 16, 24, 4), (2, 16, 25), (2, 16, 24, 25), (1, 16, 24))):
        bad.append((with_out(k, torch.empty(shape, device=DEV)), f"out {NAMES[k]} must be"))
    bad += [
        (with_out(2, torch.empty((2, 16, 24, 48), device=DEV)[..., ::2]), "contiguous"),
        (with_out(1, torch.empty((2, 16, 24), device=DEV, dtype=torch.float64)), "Float"),
        (with_out(0, torch.empty((2, 16, 24, 3))), "HIP"),
        (with_out(3, None), "missing"),
        (lambda: mb.head_finish(pts, feat, downsample=2, out=tuple(mk()[:3])), "out must be"),
    ]
    for k, (f, word) in enumerate(bad):
        with pytest.raises(RuntimeError, match=word):
            f()
            pytest.fail(f"case {k} did not raise")
    # the op still works after the rejected calls, and two runs give the same bytes
    again = mb.head_finish(pts, feat, downsample=2)
    for a, b in zip(good, again):
        assert np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy()))
    empty = mb.head_finish(torch.zeros((0, 4, 32, 48), device=DEV), torch.zeros((0, 6, 6400), device=DEV))
    assert empty[0].shape == (0, 32, 48, 3) and empty[2].shape == (0, 32, 48, 24)
