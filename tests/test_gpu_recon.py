"""Map export (recon.hip via mast3r_slam_backends.reconstruct / ReconPass and
m3s.evaluate.save_reconstruction) against the host model (tests/recon_model.py), the existing
point-map op (for the bits of the transform) and the reference's save_reconstruction
(tests/golden/recon_golden.npz), at the shapes where the tiling and the 15-byte records can go
wrong: a ragged tail with every record boundary unaligned, tiles crossed inside and between
keyframes, one point, no keyframe."""
import functools
import os

import numpy as np
import pytest
import torch

import recon_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
THRESH = 1.5
ATOL = 2e-6  # the project's bound for this transform at these magnitudes (test_gpu_keyframe.py:62)


def _tile():
    import mast3r_slam_backends as mb

    return mb.recon_tile_points()


def _shape(name):
    """-> (N, height, width)"""
    return {"ragged": (3, 13, 19), "tiles": (4, 1, 2 * _tile() + 37), "one": (1, 1, 1),
            "empty": (0, 1, 5)}[name]


SHAPES = ["ragged", "tiles", "one", "empty"]


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs of one shape (host f32 arrays, made once), at the magnitudes of
    test_gpu_keyframe._inputs / _T.  Keyframe 1 has no point above THRESH, keyframe 2 has every
    point above it, the others about 60 %; one confidence of keyframe 0 is NaN."""
    N, h, w = _shape(name)
    HW = h * w
    g = torch.Generator().manual_seed(100 + SHAPES.index(name))
    X = torch.randn((N, HW, 3), generator=g)
    n_obs = torch.tensor([2.0, 1.0, 3.0, 5.0][:N])
    C = (1.0 + torch.rand((N, HW, 1), generator=g) * 5) * 0.5 * n_obs.reshape(N, 1, 1)
    if N > 1:
        C[1] = torch.rand((HW, 1), generator=g) * THRESH * 0.99
    if N > 2:
        C[2] = (THRESH * 1.01 + torch.rand((HW, 1), generator=g) * 5) * n_obs[2]
    if N > 0 and HW > 8:
        C[0, 5, 0] = float("nan")
        C[0, 6, 0] = THRESH * n_obs[0]  # equality: not kept
    if name == "one":
        C[0, 0, 0] = 4.0 * n_obs[0]
    T = torch.empty((N, 1, 8))
    for k in range(N):
        q = torch.randn(4, generator=g)
        T[k, 0] = torch.cat([torch.randn(3, generator=g) * 0.3, q / q.norm(),
                             torch.tensor([1.1 - 0.1 * k])])
    uimg = torch.rand((N, HW, 3), generator=g)
    f = 1.1 * max(h, w)  # rays of magnitude <= 1, as a camera's
    K = torch.tensor([[f, 0.0, 0.5 * w - 0.2], [0.0, f * 1.04, 0.5 * h - 0.1], [0.0, 0.0, 1.0]])
    return dict(N=N, h=h, w=w, HW=HW, X=X, C=C, n_obs=n_obs, T=T, rgb=M.quantize(uimg.numpy()), K=K)


@functools.lru_cache(maxsize=None)
def _device_case(name):
    c = _case(name)
    d = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
    d["rgb"] = torch.from_numpy(c["rgb"]).to(DEV)
    return d


@functools.lru_cache(maxsize=None)
def _op_points(name, calib):
    """[N,HW,3] f32: what the existing point-map op (keyframe.hip, not under test) returns for
    pointmap_update("recent", ..., T=T_WC[k]) on X[k], or on constrain_points_to_ray(X[k])."""
    import mast3r_slam_backends as mb
    from m3s.geometry import constrain_points_to_ray

    d = _device_case(name)
    out = torch.zeros_like(d["X"])
    zero = torch.zeros((d["HW"], 1), device=DEV)
    for k in range(d["N"]):
        Xk = d["X"][k]
        if calib:
            Xk = constrain_points_to_ray((d["h"], d["w"]), d["X"][k:k + 1], d["K"])[0].contiguous()
        mb.pointmap_update("recent", out[k], zero.clone(), Xk, zero, d["T"][k, 0])
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _model(name, calib, colour, thresh=THRESH):
    c = _case(name)
    return M.reconstruct(c["X"].numpy(), c["C"].numpy(), c["n_obs"].numpy(), c["T"].numpy(),
                         rgb=c["rgb"] if colour else None, K=c["K"].numpy() if calib else None,
                         img_size=(c["h"], c["w"]), thresh=thresh)


def _run(backend, name, calib, colour, thresh=THRESH, C=None):
    d = _device_case(name)
    return backend.reconstruct(d["X"], d["C"] if C is None else C, d["n_obs"], d["T"],
                               rgb=d["rgb"] if colour else None, K=d["K"] if calib else None,
                               img_size=(d["h"], d["w"]) if calib else None, thresh=thresh)


def _records(backend, body):
    assert body.dtype == torch.uint8 and body.dim() == 1 and body.numel() % 15 == 0
    return body.cpu().numpy().view(backend.RECON_DTYPE)


def _xyz(rec):
    return np.stack((rec["x"], rec["y"], rec["z"]), axis=-1)


def _rgb(rec):
    return np.stack((rec["red"], rec["green"], rec["blue"]), axis=-1)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("colour", [False, True], ids=["norgb", "rgb"])
@pytest.mark.parametrize("calib", [False, True], ids=["nocalib", "calib"])
@pytest.mark.parametrize("name", SHAPES)
def test_against_model_and_point_op(backend, name, calib, colour):
    m = _model(name, calib, colour)
    body, counts = _run(backend, name, calib, colour)
    rec = _records(backend, body)
    # 1. counts, the kept set in order, the colours: equal to the host model's
    assert counts.dtype == torch.int64 and counts.device.type == "cuda"
    assert np.array_equal(counts.cpu().numpy(), m["counts"])
    assert len(rec) == int(m["counts"].sum())
    assert np.array_equal(_rgb(rec), m["colors"])
    # 2. the points are bitwise the existing op's, in the model's (k, n) order
    want = _op_points(name, calib)[m["k"], m["n"]].reshape(-1, 3)
    assert _same_bits(_xyz(rec), want)
    # 3. and within the project's bound of the f64 model
    err = np.abs(_xyz(rec).astype(np.float64) - m["points"])
    print(f"{name} calib={calib}: {len(rec)} points, max |err| vs f64 = {err.max() if len(rec) else 0.0:.3e}")
    assert np.all(err <= ATOL)
    # 4. the none-kept and the all-kept keyframe
    if _case(name)["N"] >= 3:
        assert m["counts"][1] == 0 and m["counts"][2] == _case(name)["HW"]
    # 6. a second run gives the same bytes
    body2, counts2 = _run(backend, name, calib, colour)
    assert torch.equal(body, body2) and torch.equal(counts, counts2)


@pytest.mark.parametrize("name,where", [("ragged", "last"), ("tiles", "last"), ("tiles", "full_tile_end")])
def test_single_point_in_the_last_lane(backend, name, where):
    """A threshold that keeps exactly one point: the last point of the last keyframe (the last
    lane of the last, ragged tile), or the last lane of the last full tile."""
    d = _device_case(name)
    n = d["HW"] - 1 if where == "last" else 2 * _tile() - 1
    k = d["N"] - 1
    C = d["C"].clone()
    C[k, n, 0] = 100.0 * float(d["n_obs"][k])
    body, counts = _run(backend, name, True, True, thresh=50.0, C=C)
    rec = _records(backend, body)
    assert counts.cpu().tolist() == [0] * k + [1] and len(rec) == 1
    assert _same_bits(_xyz(rec), _op_points(name, True)[k, n].reshape(1, 3))
    assert np.array_equal(_rgb(rec)[0], _case(name)["rgb"][k, n])


@pytest.mark.parametrize("name", ["ragged", "tiles", "one"])
def test_emit_capacity_and_canary(backend, name):
    """emit never writes past capacity: with total - 1 (and other cuts: nothing, one record, the
    end of keyframe 0) the records before the cut are unchanged and the bytes after it keep the
    canary; so do the bytes after a full-capacity emit."""
    d = _device_case(name)
    full, counts = _run(backend, name, False, True)
    total = full.numel() // 15
    assert total >= 1
    p = backend.ReconPass(d["X"], d["C"], d["n_obs"], d["T"], rgb=d["rgb"], thresh=THRESH)
    c2, t2 = p.count()
    assert int(t2.item()) == total and torch.equal(c2, counts)
    pad = 64
    for cap in sorted({total - 1, total, 0, 1, int(counts[0].item())}):
        if cap > total:
            continue
        out = torch.full((15 * total + pad,), 0xA5, dtype=torch.uint8, device=DEV)
        p.emit(out, cap)
        assert torch.equal(out[:15 * cap], full[:15 * cap]), cap
        assert bool((out[15 * cap:] == 0xA5).all()), cap
    # a capacity above the total writes the total
    out = torch.full((15 * (total + 3) + pad,), 0xA5, dtype=torch.uint8, device=DEV)
    p.emit(out, total + 3)
    assert torch.equal(out[:15 * total], full) and bool((out[15 * total:] == 0xA5).all())
    # an output that starts at every byte phase
    for shift in (1, 2, 3):
        out = torch.full((15 * total + pad,), 0xA5, dtype=torch.uint8, device=DEV)
        p.emit(out[shift:], total)
        assert torch.equal(out[shift:shift + 15 * total], full)
        assert bool((out[:shift] == 0xA5).all()) and bool((out[shift + 15 * total:] == 0xA5).all())


def test_empty_inputs(backend):
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=DEV)
    body, counts = backend.reconstruct(z(0, 5, 3), z(0, 5), z(0), z(0, 8))
    assert body.numel() == 0 and counts.shape == (0,)
    body, counts = backend.reconstruct(z(2, 0, 3), z(2, 0), z(2) + 1, z(2, 8))
    assert body.numel() == 0 and counts.cpu().tolist() == [0, 0]


def test_argument_errors(backend):
    d = _device_case("ragged")
    with pytest.raises(RuntimeError):  # K without the image size
        backend.reconstruct(d["X"], d["C"], d["n_obs"], d["T"], K=d["K"])
    with pytest.raises(RuntimeError):  # image size that is not HW
        backend.reconstruct(d["X"], d["C"], d["n_obs"], d["T"], K=d["K"], img_size=(13, 20))
    with pytest.raises(RuntimeError):  # no CPU path
        backend.reconstruct(d["X"].cpu(), d["C"].cpu(), d["n_obs"].cpu(), d["T"].cpu())
    with pytest.raises(RuntimeError):  # colours of another shape
        backend.reconstruct(d["X"], d["C"], d["n_obs"], d["T"], rgb=d["rgb"][:2])


@pytest.mark.parametrize("case", [0, 1])
def test_golden_reference_save_reconstruction(backend, case):
    """The reference's own save_reconstruction (tests/golden/make_recon_golden.py): the same
    selection and colours, points within the bound."""
    from m3s.global_opt import quantize_uimg

    gold = np.load(os.path.join(HERE, "golden", "recon_golden.npz"))
    t = lambda key: torch.from_numpy(gold[f"c{case}_{key}"]).to(DEV)
    calib = bool(gold[f"c{case}_calib"])
    h, w = (int(v) for v in gold["img_size"])
    N = gold[f"c{case}_X"].shape[0]
    rgb = quantize_uimg(t("uimg")).reshape(N, h * w, 3).contiguous()
    body, counts = backend.reconstruct(t("X"), t("C"), t("n_obs"), t("T_WC"), rgb=rgb,
                                       K=t("K") if calib else None,
                                       img_size=(h, w) if calib else None,
                                       thresh=float(gold["thresh"]))
    rec = _records(backend, body)
    ref_p, ref_c = gold[f"c{case}_out_points"], gold[f"c{case}_out_colors"]
    assert counts.cpu().tolist()[1:] == [0, h * w]
    assert len(rec) == len(ref_p)
    assert np.array_equal(_rgb(rec), ref_c)
    # the kept set itself, from the reference's average confidences
    keep = (gold[f"c{case}_C"].reshape(N, -1) / gold[f"c{case}_n_obs"][:, None]) > gold["thresh"]
    assert np.array_equal(counts.cpu().numpy(), keep.sum(axis=1))
    err = np.abs(_xyz(rec).astype(np.float64) - ref_p.astype(np.float64))
    print(f"golden case {case}: max |err| vs the reference = {err.max():.3e}")
    assert np.all(err <= ATOL)


def _store(calib, N=5, h=13, w=19):
    from m3s.global_opt import KeyframeStore

    g = torch.Generator().manual_seed(77)
    K = torch.tensor([[21.0, 0.0, 9.3], [0.0, 21.5, 6.4], [0.0, 0.0, 1.0]], device=DEV)
    st = KeyframeStore(8, h, w, device=DEV, K=K if calib else None, keep_rgb=True)
    frames = []
    for k in range(N):
        q = torch.randn(4, generator=g)
        T = torch.cat([torch.randn(3, generator=g) * 0.3, q / q.norm(), torch.tensor([1.0 + 0.05 * k])])
        n_obs = float(k % 3 + 1)
        X = torch.randn((h * w, 3), generator=g)
        C = (1.0 + torch.rand((h * w, 1), generator=g) * 5) * 0.5 * n_obs
        if k == 3:
            C = C * 0.1  # a keyframe without a kept point, alone in its chunk of 1
        uimg = torch.rand((h, w, 3), generator=g)
        st.append(X.to(DEV), C.to(DEV), T.to(DEV), n_obs=n_obs, uimg=uimg, frame_id=10 * k)
        frames.append((X, C, T, n_obs, uimg))
    return st, frames, K


@pytest.mark.parametrize("calib", [False, True], ids=["nocalib", "calib"])
def test_save_reconstruction_store_chunks(backend, tmp_path, calib):
    from m3s.evaluate import read_ply, save_reconstruction
    from m3s.frame import Frame
    from m3s.global_opt import PoseBatch

    st, frames, K = _store(calib)
    N = len(st)
    body, counts = backend.reconstruct(st.X[:N], st.C[:N], st.n_obs[:N], st.T_WC[:N], rgb=st.rgb[:N],
                                       K=K if calib else None,
                                       img_size=(st.h, st.w) if calib else None, thresh=THRESH)
    rec = _records(backend, body)
    assert int(counts[3]) == 0 and len(rec) > 0
    X_before = st.X.clone()
    n2 = save_reconstruction(str(tmp_path), "c2.ply", st, THRESH, use_calib=calib, chunk_keyframes=2)
    n1 = save_reconstruction(str(tmp_path), "c1.ply", st, THRESH, use_calib=calib, chunk_keyframes=1)
    assert n1 == n2 == len(rec)
    assert torch.equal(st.X, X_before)  # the store's points are not overwritten
    pts, cols = read_ply(str(tmp_path / "c2.ply"))
    assert _same_bits(pts, _xyz(rec)) and np.array_equal(cols, _rgb(rec))
    assert (tmp_path / "c1.ply").read_bytes() == (tmp_path / "c2.ply").read_bytes()
    # a list of Frame takes the same path
    fl = []
    for k, (X, C, T, n_obs, uimg) in enumerate(frames):
        f = Frame(frame_id=10 * k, img=torch.zeros((1, 3, st.h, st.w)), T_WC=PoseBatch(T.reshape(1, 8).to(DEV)),
                  X_canon=X.to(DEV), C=C.to(DEV), K=K, uimg=uimg)
        f.N = int(n_obs)
        fl.append(f)
    n3 = save_reconstruction(str(tmp_path), "list.ply", fl, THRESH, use_calib=calib, chunk_keyframes=3)
    assert n3 == n2
    assert (tmp_path / "list.ply").read_bytes() == (tmp_path / "c2.ply").read_bytes()
