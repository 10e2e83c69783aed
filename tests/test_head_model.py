"""Host side of the head finish: the numpy model (tests/head_model.py) and
m3s.mast3r_utils.postprocess_torch on the CPU against the reference's own outputs
(tests/golden/make_head_golden.py -> head_golden.npz: Cat_MLP_LocalFeatures_DPT_Pts3d.forward and
mast3r_utils.downsample run as written), inside the derived bounds; and the C ABI's argument
checks, which return before any device work."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import head_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("X", "C", "D", "Q")


@functools.lru_cache(maxsize=None)
def gold():
    g = np.load(os.path.join(HERE, "golden", "head_golden.npz"))
    pts, feat, F = g["pts"], g["feat"], int(g["F"])
    B, _, H, W = pts.shape
    return dict(g=g, pts=pts, feat=feat, F=F, H=H, W=W, planar=M.shuffle(feat, H, W),
                T1=M.tol(g["T_expm1"]), T=M.tol(g["T_exp"]))


def bounds(G, ds):
    """Per-output relative bounds of an f32 evaluation against the f64 model."""
    dn = M.norm_f64(G["pts"], ds)[..., None]
    return (M.bound_X(dn, G["T1"]), M.bound_CQ(G["T"]), M.bound_D(G["F"]), M.bound_CQ(G["T"]))


def test_fixture_shape_and_recorded_terms():
    G = gold()
    assert G["pts"].shape == (1, 4, 32, 48) and G["feat"].shape == (1, 6, 25 * 256) and G["F"] == 24
    # the reference's own f32 exp / expm1 are within 1 u of f64 here, so the tests run with T = 2
    assert 0 < float(G["g"]["T_expm1"]) <= 1.0 and 0 < float(G["g"]["T_exp"]) <= 1.0
    assert G["T1"] == 2.0 and G["T"] == 2.0
    assert os.path.getsize(os.path.join(HERE, "golden", "head_golden.npz")) < 659 * 1024


def test_shuffle_is_pixel_shuffle():
    """The token layout's index identity against F.pixel_shuffle, on a 2x3 token grid."""
    rng = np.random.default_rng(0)
    feat = rng.standard_normal((2, 6, 5 * 256)).astype(np.float32)
    t = torch.from_numpy(feat)
    ref = torch.nn.functional.pixel_shuffle(t.transpose(-1, -2).reshape(2, -1, 2, 3), 16).numpy()
    got = M.shuffle(feat, 32, 48)
    assert np.array_equal(got, ref)
    assert np.array_equal(M.unshuffle(got), feat)


@pytest.mark.parametrize("ds", [1, 2])
def test_f64_model_agrees_with_reference(ds):
    G = gold()
    m64 = M.model_f64(G["pts"], G["planar"], ds)
    for n, m, bd in zip(NAMES, m64, bounds(G, ds)):
        ref = G["g"][f"ds{ds}_{n}"]
        assert ref.shape == m.shape
        assert np.all(M.rel_err_u(ref, m) * M.U <= bd), n


@pytest.mark.parametrize("ds", [1, 2])
def test_f32_model_agrees_with_reference(ds):
    """Two f32 evaluations differ by at most the sum of their bounds."""
    G = gold()
    m64 = M.model_f64(G["pts"], G["planar"], ds)
    m32 = M.model_f32(G["pts"], G["planar"], ds)
    for n, a, m, bd in zip(NAMES, m32, m64, bounds(G, ds)):
        assert a.dtype == np.float32
        ref = G["g"][f"ds{ds}_{n}"].astype(np.float64)
        assert np.all(M.rel_err_u(a, m) * M.U <= bd), n
        assert np.all(np.abs(a - ref) <= 2 * bd * np.abs(m)), n
        assert np.array_equal(np.isnan(a), np.isnan(ref)), n  # none, in the fixture


def test_f32_model_downsample_is_a_slice():
    G = gold()
    full = M.model_f32(G["pts"], G["planar"], 1)
    third = M.model_f32(G["pts"], G["planar"], 3)
    for a, b in zip(full, third):
        assert b.shape[1:3] == (11, 16)
        assert np.array_equal(a[:, ::3, ::3], b)


def test_f32_model_nan_where_reference_has():
    """A zero descriptor is 0 / 0 in the reference (no guard) and in the model; a NaN input stays."""
    pts, planar = M.make_inputs(1, 16, 16, 24, 3)
    planar[0, :24, 2, 5] = 0.0
    planar[0, 7, 9, 1] = np.nan
    pts[0, 1, 4, 4] = np.nan
    from m3s.mast3r_utils import postprocess_torch

    ref = postprocess_torch(torch.from_numpy(np.concatenate([pts, planar], axis=1)), 24)
    m32 = M.model_f32(pts, planar)
    for n, a, r in zip(NAMES, m32, ref):
        assert np.array_equal(np.isnan(a), np.isnan(r.numpy())), n
    assert np.isnan(m32[2][0, 2, 5]).all() and np.isnan(m32[2][0, 9, 1]).all()
    assert np.isnan(m32[2]).sum() == 48 and np.isnan(m32[0]).sum() == 3


@pytest.mark.parametrize("ds", [1, 2])
def test_postprocess_torch_cpu_within_bounds_of_fixture(ds):
    from m3s.mast3r_utils import postprocess_torch, shuffle_tokens

    G = gold()
    pts, feat = torch.from_numpy(G["pts"]), torch.from_numpy(G["feat"])
    planar = shuffle_tokens(feat, G["H"], G["W"])
    assert np.array_equal(planar.numpy(), G["planar"])
    got = postprocess_torch(torch.cat([pts, planar], dim=1), G["F"], downsample=ds)
    m64 = M.model_f64(G["pts"], G["planar"], ds)
    for n, a, m, bd in zip(NAMES, got, m64, bounds(G, ds)):
        assert a.is_contiguous() and a.dtype == torch.float32
        ref = G["g"][f"ds{ds}_{n}"].astype(np.float64)
        assert np.all(M.rel_err_u(a.numpy(), m) * M.U <= bd), n
        assert np.all(np.abs(a.numpy() - ref) <= 2 * bd * np.abs(m)), n


def test_finish_heads_cpu_path_stacks_heads():
    """CPU tensors go through postprocess_torch; head k fills rows k*B..(k+1)*B-1."""
    from m3s import mast3r_utils as U

    heads = []
    for k in range(2):
        pts, planar = M.make_inputs(1, 16, 32, 24, 40 + k)
        heads.append((torch.from_numpy(pts), torch.from_numpy(M.unshuffle(planar)), pts, planar))
    X, C, D, Q = U.finish_heads([(h[0], h[1]) for h in heads], downsample=2)
    assert X.shape == (2, 8, 16, 3) and C.shape == (2, 8, 16) and D.shape == (2, 8, 16, 24)
    for k, h in enumerate(heads):
        m64 = M.model_f64(h[2], h[3], 2)
        assert np.all(M.rel_err_u(D[k:k + 1].numpy(), m64[2]) * M.U <= M.bound_D(24))
        assert np.all(M.rel_err_u(Q[k:k + 1].numpy(), m64[3]) * M.U <= M.bound_CQ(2.0))
    Xm, Cm = U.mast3r_inference_mono_raw((heads[0][0], heads[0][1]), downsample=2)
    assert Xm.shape == (128, 3) and Cm.shape == (128, 1)
    assert torch.equal(Xm, X[0].view(-1, 3)) and torch.equal(Cm, C[0].view(-1, 1))
    from m3s.config import DEFAULT_CONFIG

    assert DEFAULT_CONFIG["dataset"]["img_downsample"] == 1


def test_traffic_model():
    """tools/head_probe.py: every raw value read once, every result written once."""
    import importlib.util

    spec = importlib.util.spec_from_file_location(
        "head_probe", os.path.join(os.path.dirname(HERE), "tools", "head_probe.py"))
    probe = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(probe)
    t = probe.traffic_bytes(1, 384, 512, 24)
    assert t == {"read": 384 * 512 * 29 * 4, "write": 384 * 512 * 29 * 4}
    assert round((t["read"] + t["write"]) / 1e6, 1) == 45.6
    assert probe.traffic_bytes(2, 32, 48, 24, ds=3)["write"] == 2 * 11 * 16 * 29 * 4
    assert probe.traffic_bytes(1, 32, 48, 24, desc=False) == {"read": 32 * 48 * 16, "write": 32 * 48 * 16}


def _args(backend, **kw):
    a = backend.HeadArgs()
    a.B, a.H, a.W, a.F, a.patch, a.downsample = 1, 32, 48, 24, 16, 1
    a.conf_vmin, a.conf_vmax, a.dconf_vmin, a.dconf_vmax = 1.0, float("inf"), 0.0, float("inf")
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("field,value,word", [
    ("depth_mode", 1, "depth mode"), ("depth_mode", 2, "depth mode"), ("conf_mode", 1, "conf mode"),
    ("desc_mode", 1, "desc mode"), ("single_conf", 1, "two_confs"), ("layout", 2, "layout"),
    ("patch", 8, "patch"), ("downsample", 0, "downsample"), ("B", -1, "negative"),
])
def test_abi_rejects_unbuilt_modes_and_bad_arguments(backend, field, value, word):
    """Checked before any pointer is used or any device call is made."""
    rc = backend.lib.m3s_head_finish(ctypes.byref(_args(backend, **{field: value})))
    assert rc == 1  # M3S_ERR_INVALID
    assert word in backend.lib.m3s_last_error().decode()


def test_abi_empty_is_ok_and_null_is_invalid(backend):
    for k in ("B", "H", "W"):
        assert backend.lib.m3s_head_finish(ctypes.byref(_args(backend, **{k: 0}))) == 0
    assert backend.lib.m3s_head_finish(ctypes.byref(_args(backend))) == 1  # null pts / X / C
    assert "null pointer" in backend.lib.m3s_last_error().decode()
    assert backend.lib.m3s_head_finish(None) == 1


def test_binding_checks_on_cpu(backend):
    pts = torch.zeros((1, 4, 32, 48))
    with pytest.raises(RuntimeError, match="HIP"):
        backend.head_finish(pts, None)
    with pytest.raises(RuntimeError, match="Float"):
        backend.head_finish(pts.double(), None)
    with pytest.raises(RuntimeError, match="layout"):
        backend.head_finish(pts, None, layout="nhwc")
    with pytest.raises(RuntimeError, match="patch"):
        backend.head_finish(pts, None, patch=8)
