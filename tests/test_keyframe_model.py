"""The host models of tests/keyframe_model.py against what they stand for, without a GPU:
fuse against the reference's Frame.update_pointmap (tests/golden/keyframe_golden.npz, generated
by make_keyframe_golden.py from the reference's Python), act64 against the oracle's Sim3 act,
act_bound against a plain f32 restatement of the transform (the bound is not vacuous), and the
edge model against the reference's add_factors store (tests/golden/edges_golden.npz)."""
import os

import numpy as np
import pytest

import keyframe_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "keyframe_golden.npz"))
EDGES = np.load(os.path.join(HERE, "golden", "edges_golden.npz"))


def transforms(n=200, seed=0):
    """Sim3 data with s in [e^-3, e^3], |t| in 1e-2..1e2 and a unit q normalised in f32."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        q = rng.standard_normal(4).astype(np.float32)
        q = q / np.sqrt((q * q).sum(dtype=np.float32))
        t = rng.standard_normal(3)
        t = t / np.linalg.norm(t) * 10.0 ** rng.uniform(-2, 2)
        out.append(np.concatenate([t, q, [np.exp(rng.uniform(-3, 3))]]).astype(np.float32))
    return out


def points(n=64, seed=1):
    """Points whose norms span 1e-2..1e2."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (d * 10.0 ** rng.uniform(-2, 2, (n, 1))).astype(np.float32)


@pytest.mark.parametrize("mode", M.MODES)
def test_fuse_is_the_reference_update_bitwise(mode):
    n = int(GOLD["ncalls"])
    for c in range(1, n):
        X, C = GOLD[f"{mode}_X_canon"][c - 1], GOLD[f"{mode}_C_canon"][c - 1]
        gX, gC = M.fuse(mode, X, C, GOLD[f"{mode}_X"][c], GOLD[f"{mode}_C"][c])
        assert gX.dtype == np.float32 and gC.dtype == np.float32
        assert M.same_bits(gX, GOLD[f"{mode}_X_canon"][c]), (mode, c)
        assert M.same_bits(gC, GOLD[f"{mode}_C_canon"][c]), (mode, c)


def test_fixture_holds_the_conditions_the_device_test_relies_on():
    assert int(GOLD["HW"]) == 300 and int(GOLD["ncalls"]) == 4
    for c in range(1, 4):
        prev, new = GOLD[f"indep_conf_C_canon"][c - 1], GOLD[f"indep_conf_C"][c]
        assert (new == prev).sum() >= 75 and (new > prev).sum() >= 75 and (new < prev).sum() >= 75
    for name in ("best_median", "best_mean"):
        r = GOLD[name + "_replaced"]
        assert r[0] and r[1:].any() and not r[1:].all()
        for c in range(1, 4):  # N_updates counts every call, N restarts at a replacement
            assert int(GOLD[f"{name}_N_updates"][c]) == c + 1 and int(GOLD[f"{name}_N"][c]) == 1
    assert [int(GOLD[f"weighted_pointmap_N"][c]) for c in range(4)] == [1, 2, 3, 4]
    assert [int(GOLD[f"first_N_updates"][c]) for c in range(4)] == [1, 2, 3, 4]
    # first: the second call replaces (N_updates == 1), later ones do not
    assert np.array_equal(GOLD["first_X_canon"][3], GOLD["first_X"][1])
    # get_average_conf is the correctly rounded f32 quotient C / N (N = 3 is not a power of two)
    for name in GOLD["names"]:
        for c in range(4):
            N = np.float32(GOLD[f"{name}_N"][c])
            assert M.same_bits(GOLD[f"{name}_avg_conf"][c], GOLD[f"{name}_C_canon"][c] / N), (name, c)
    assert GOLD["sph_dev"][0] == 0.0 and 0.0 < GOLD["sph_dev"][1:].max() < 1e-5


def test_act64_is_the_oracle_sim3_act():
    from oracle import track_oracle as TO

    p = points()
    for T in transforms(40):
        ref = TO.sim3_act(T.astype(np.float64), p.astype(np.float64))
        got = M.act64(T, p)
        assert got.dtype == np.float64
        assert np.abs(got - ref).max() <= 1e-12


def test_plain_f32_transform_stays_within_act_bound():
    p = points()
    worst = 0.0
    for T in transforms(200):
        err = np.abs(M.act32_plain(T, p).astype(np.float64) - M.act64(T, p))
        unit = M.act_bound(T, p, K=1)
        assert unit.shape == (len(p), 1) and np.all(unit > 0)
        assert np.all(err <= M.act_bound(T, p))
        worst = max(worst, float((err / unit).max()))
    print(f"plain f32 act: worst error {worst:.3f} of the K=1 unit (bound K={M.ACT_K})")
    # not vacuous: the honest f32 error is a sizeable part of the unit, and well inside K
    assert 0.2 < worst < 1.25
    # ... while a conjugated quaternion or swapped components miss by orders of magnitude
    T = transforms(1, seed=5)[0]
    Tc = T.copy()
    Tc[3:6] = -Tc[3:6]
    assert (np.abs(M.act64(Tc, p) - M.act64(T, p)) / M.act_bound(T, p)).max() > 1e3
    assert (np.abs(M.act64(T, p[:, ::-1]) - M.act64(T, p)) / M.act_bound(T, p)).max() > 1e3


def test_edge_model_is_the_reference_add_factors():
    """The rule of test_gpu_edges._sqrt_ref_store: the reference's CPU sqrt is not correctly
    rounded, so its stored Q is within 1 ulp of the model's; counts decide the same pairs."""
    names = ["idx_i2j", "idx_j2i", "valid_match_j", "valid_match_i", "Qii", "Qjj", "Qji", "Qij"]
    frac_min = float(EDGES["min_match_frac"])
    for c in range(int(EDGES["ncalls"])):
        m = [EDGES[f"c{c}_{n}"] for n in names]
        B, HW = m[0].shape
        Qj, Qi, counts = M.edge_confidence(*m, 1.5)
        assert Qj.shape == (B, HW, 1) and Qj.dtype == np.float32 and counts.dtype == np.int64
        bi = np.arange(B)[:, None]
        tQj = np.sqrt(m[4][bi, m[0]] * m[6])  # the torch expression with numpy's f32 sqrt
        assert np.abs(Qj.view(np.int32) - tQj.view(np.int32)).max() <= 1
        if bool(EDGES[f"c{c}_reloc"]) and not bool(EDGES[f"c{c}_ret"]):
            continue
        # the pairs the reference kept are those whose match fractions pass (global_opt.py:69-80),
        # consecutive keyframes always; their stored Q rows are the model's to 1 ulp
        prev = 0 if c == 0 else EDGES[f"c{c - 1}_store_ii"].shape[0]
        kept = list(zip(EDGES[f"c{c}_store_ii"][prev:], EDGES[f"c{c}_store_jj"][prev:]))
        ii, jj = EDGES[f"c{c}_ii"], EDGES[f"c{c}_jj"]
        sel = [k for k in range(B) if (ii[k], jj[k]) in kept]
        frac = counts.min(axis=1) / HW
        want = [k for k in range(B) if frac[k] >= frac_min or int(ii[k]) == int(jj[k]) - 1]
        assert sel == want, (c, sel, want)
        for store, q in (("Q_ii2jj", Qj), ("Q_jj2ii", Qi)):
            ref = EDGES[f"c{c}_store_{store}"][prev:]
            assert ref.shape == q[sel].shape
            assert np.abs(q[sel].view(np.int32) - ref.view(np.int32)).max() <= 1, (c, store)


def test_edge_model_clamps_and_ignores_nan():
    HW = 5
    Q = np.arange(1, HW + 1, dtype=np.float32).reshape(1, HW, 1) * 4
    idx = np.array([[-1, HW, 2 ** 40, -2 ** 63, 2]], np.int64)
    one = np.ones((1, HW, 1), np.float32)
    one[0, 4, 0] = np.nan
    vm = np.ones((1, HW, 1), bool)
    Qj, Qi, counts = M.edge_confidence(idx, idx, vm, vm, Q, Q, one, one, 1.5)
    assert np.array_equal(Qj[0, :4, 0], np.sqrt(np.float32([4, 20, 20, 4])))
    assert np.isnan(Qj[0, 4, 0]) and counts.tolist() == [[4, 4]]
