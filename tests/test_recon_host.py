"""Host side of the map export: the PLY subset of m3s.evaluate, the record dtype, the host model
(tests/recon_model.py) on a hand-made case, and KeyframeStore(keep_rgb=True) on the CPU."""
import os

import numpy as np
import pytest
import torch

import recon_model as M

HEADER = (b"ply\n"
          b"format binary_little_endian 1.0\n"
          b"element vertex %d\n"
          b"property float x\n"
          b"property float y\n"
          b"property float z\n"
          b"property uchar red\n"
          b"property uchar green\n"
          b"property uchar blue\n"
          b"end_header\n")


@pytest.mark.parametrize("n", [0, 1, 7])
def test_ply_round_trip_and_header(tmp_path, n):
    from m3s.evaluate import read_ply, save_ply

    rng = np.random.default_rng(n)
    pts = rng.standard_normal((n, 3)).astype(np.float32)
    col = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    path = str(tmp_path / "cloud.ply")
    save_ply(path, pts, col)
    raw = open(path, "rb").read()
    header = HEADER % n
    assert raw[:len(header)] == header
    assert os.path.getsize(path) == len(header) + 15 * n
    p2, c2 = read_ply(path)
    assert p2.dtype == np.float32 and c2.dtype == np.uint8
    assert p2.shape == (n, 3) and c2.shape == (n, 3)
    assert np.array_equal(p2, pts) and np.array_equal(c2, col)
    # the body is the packed record array
    rec = np.frombuffer(raw[len(header):], dtype=M.RECORD)
    assert np.array_equal(rec["y"], pts[:, 1]) and np.array_equal(rec["blue"], col[:, 2])


def test_read_ply_rejects_other_files(tmp_path):
    from m3s.evaluate import read_ply

    path = str(tmp_path / "bad.ply")
    with open(path, "wb") as f:
        f.write((HEADER % 2) + b"\0" * 29)  # one byte short of two vertices
    with pytest.raises(ValueError):
        read_ply(path)
    with open(path, "wb") as f:
        f.write(b"ply\nformat ascii 1.0\nelement vertex 0\nend_header\n")
    with pytest.raises(ValueError):
        read_ply(path)


def test_record_dtype(backend):
    from m3s.evaluate import PLY_VERTEX_DTYPE

    assert backend.RECON_DTYPE.itemsize == 15
    assert backend.RECON_DTYPE.names == ("x", "y", "z", "red", "green", "blue")
    assert backend.RECON_DTYPE == PLY_VERTEX_DTYPE == M.RECORD
    assert backend.recon_tile_points() > 0


def test_model_selection_hand_made():
    """2 keyframes x 6 points, thresh 1.5: NaN, equality at the threshold and n_obs = 3."""
    nan, inf = float("nan"), float("inf")
    C = np.array([[1.4, 1.5, np.nextafter(np.float32(1.5), np.float32(2)), nan, inf, -inf],
                  [4.5, np.nextafter(np.float32(4.5), np.float32(5)), 4.4999995, 9.0, 0.0, nan]],
                 np.float32)
    n_obs = np.array([1.0, 3.0], np.float32)
    keep = M.select(C, n_obs, 1.5)
    assert keep.tolist() == [[False, False, True, False, True, False],
                             [False, True, False, True, False, False]]
    X = np.arange(2 * 6 * 3, dtype=np.float32).reshape(2, 6, 3)
    T = np.tile(np.array([1, 2, 3, 0, 0, 0, 1, 2], np.float32), (2, 1))  # 2 p + (1,2,3)
    rgb = np.arange(2 * 6 * 3, dtype=np.uint8).reshape(2, 6, 3)
    m = M.reconstruct(X, C, n_obs, T, rgb=rgb, thresh=1.5)
    assert m["counts"].tolist() == [2, 2]
    assert m["k"].tolist() == [0, 0, 1, 1] and m["n"].tolist() == [2, 4, 1, 3]
    assert np.array_equal(m["points"], 2.0 * X[m["k"], m["n"]] + np.array([1.0, 2.0, 3.0]))
    assert np.array_equal(m["colors"], rgb[m["k"], m["n"]])
    # with K: the points move onto their pixel rays, the depth stays
    K = np.array([[2.0, 0, 1.0], [0, 4.0, 0.5], [0, 0, 1]], np.float32)
    mk = M.reconstruct(X, C, n_obs, T, K=K, img_size=(2, 3), thresh=1.5)
    z = X[0, 4, 2]  # pixel n = 4 of a 2x3 image: u = 1, v = 1
    assert np.array_equal(mk["points"][1], 2.0 * np.array([z * 0.0, z * 0.125, z]) + [1.0, 2.0, 3.0])
    assert np.array_equal(mk["colors"], np.zeros((4, 3), np.uint8))
    # nothing at all
    e = M.reconstruct(np.zeros((0, 5, 3), np.float32), np.zeros((0, 5)), np.zeros((0,)),
                      np.zeros((0, 8)))
    assert e["counts"].shape == (0,) and e["points"].shape == (0, 3)


def test_quantize_matches_reference_cast():
    from m3s.global_opt import quantize_uimg

    u = torch.tensor([0.0, 0.5, 1.0, 0.999, 1.0 / 255, 0.00392, 254.999 / 255, -0.2, 1.7, float("nan")])
    q = quantize_uimg(u).numpy()
    inside = u.numpy()[:7]
    assert np.array_equal(q[:7], (inside * 255).astype(np.uint8))  # evaluate.py:60
    assert q[7:].tolist() == [0, 255, 0]
    assert np.array_equal(q, M.quantize(u.numpy()))


def test_keyframe_store_keep_rgb_cpu(tmp_path):
    from m3s.evaluate import read_tum, save_traj
    from m3s.global_opt import KeyframeStore

    h, w = 3, 4
    g = torch.Generator().manual_seed(0)
    plain = KeyframeStore(4, h, w, device="cpu")
    assert plain.rgb is None and plain.frame_ids is None
    with pytest.raises(RuntimeError):
        plain.append(torch.zeros(h * w, 3), torch.ones(h * w, 1), torch.zeros(8), uimg=torch.zeros(h, w, 3))

    K = torch.tensor([[5.0, 0, 2.0], [0, 5.0, 1.5], [0, 0, 1.0]])
    st = KeyframeStore(4, h, w, device="cpu", K=K, keep_rgb=True)
    assert st.rgb.shape == (4, h * w, 3) and st.rgb.dtype == torch.uint8
    imgs, ids = [], [7, 2, 11]
    for i, fid in enumerate(ids):
        T = torch.tensor([0.1 * i, 0.2, 0.3, 0.0, 0.0, 0.0, 1.0, 1.5])
        uimg = torch.rand((h, w, 3), generator=g)
        if i == 1:
            uimg = uimg.reshape(h * w, 3)  # [HW,3] is accepted too
        imgs.append(uimg)
        k = st.append(torch.randn((h * w, 3), generator=g), torch.ones(h * w, 1), T, uimg=uimg,
                      frame_id=fid)
        assert k == i
    assert len(st) == 3 and st.frame_ids[:3] == ids
    for i in range(3):
        want = (imgs[i].numpy() * 255).astype(np.uint8).reshape(-1, 3)
        assert np.array_equal(st.rgb[i].numpy(), want)
        v = st[i]
        assert v.frame_id == ids[i] and v.K is K
        assert v.uimg.shape == (h, w, 3) and v.uimg.dtype == torch.float32
        assert np.array_equal((v.uimg.numpy() * 255).round().astype(np.uint8).reshape(-1, 3), want)
    st.set_keyframe(1, frame_id=5)
    assert st[1].frame_id == 5 and np.array_equal(
        st.rgb[1].numpy(), (imgs[1].numpy() * 255).astype(np.uint8))
    # save_traj runs on the store: timestamps[frame_id], pose with the scale dropped
    stamps = np.arange(12) * 0.5
    path = str(tmp_path / "traj.txt")
    save_traj(path, stamps, st)
    ts, xyz, quat = read_tum(path)
    assert ts.tolist() == [3.5, 2.5, 5.5]
    assert np.allclose(xyz, [[0.0, 0.2, 0.3], [0.1, 0.2, 0.3], [0.2, 0.2, 0.3]], atol=1e-7)
    assert np.allclose(quat, [[0, 0, 0, 1]] * 3)


def test_frame_keeps_uimg():
    from m3s.frame import Frame

    u = torch.rand(2, 2, 3)
    assert Frame(uimg=u).uimg is u and Frame().uimg is None


def test_c_abi_argument_errors(backend):
    """M3S_REQUIRE on the map-export entry points: rejected before anything touches a device."""
    import ctypes

    lib, tile = backend.lib, backend.recon_tile_points()
    ws_bytes = lib.m3s_recon_workspace_bytes
    assert ws_bytes(0, 0) == ws_bytes(3, 0) == ws_bytes(0, 7)
    # one i64 offset per tile and one more, one u32 count per tile; tiles never span keyframes
    assert ws_bytes(4, 2 * tile + 37) >= 8 * (4 * 3 + 1) + 4 * (4 * 3)
    assert ws_bytes(4, 2 * tile) < ws_bytes(400, 2 * tile + 1)

    host = np.zeros(64, np.float32)
    out = np.zeros(4, np.int64)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)

    def args(**kw):
        a = backend.ReconArgs(p(host), p(host), p(host), p(host), None, None, 1, 4, 0, 0, 1.5,
                              p(host), host.nbytes, None)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def rejected(rc, word):
        assert rc != 0
        assert word in lib.m3s_last_error().decode()

    rejected(lib.m3s_recon_count(None, p(out), p(out)), "null args")
    rejected(lib.m3s_recon_emit(None, p(out), 1), "null args")
    rejected(lib.m3s_recon_count(ctypes.byref(args(N=-1)), p(out), p(out)), "negative size")
    rejected(lib.m3s_recon_count(ctypes.byref(args()), p(out), None), "null output")
    rejected(lib.m3s_recon_count(ctypes.byref(args(X=None)), p(out), p(out)), "null pointer")
    rejected(lib.m3s_recon_count(ctypes.byref(args(ws_bytes=8)), p(out), p(out)), "workspace too small")
    rejected(lib.m3s_recon_count(ctypes.byref(args(ws=None)), p(out), p(out)), "workspace")
    rejected(lib.m3s_recon_count(ctypes.byref(args(K=p(host), height=2, width=3)), p(out), p(out)),
             "height * width")
    rejected(lib.m3s_recon_emit(ctypes.byref(args()), p(out), -1), "negative capacity")
    rejected(lib.m3s_recon_emit(ctypes.byref(args()), None, 1), "null output")
    rejected(lib.m3s_recon_emit(ctypes.byref(args(ws_bytes=8)), p(out), 1), "workspace too small")
    # nothing to write: no pointer is looked at
    assert lib.m3s_recon_emit(ctypes.byref(args(N=0, X=None, ws=None)), None, 5) == 0
    assert lib.m3s_recon_emit(ctypes.byref(args()), None, 0) == 0


def test_reconstruct_rejects_cpu_tensors(backend):
    z = torch.zeros
    with pytest.raises(RuntimeError, match="no CPU path"):
        backend.reconstruct(z(2, 6, 3), z(2, 6, 1), torch.ones(2), z(2, 1, 8))
    with pytest.raises(RuntimeError, match="expected scalar type Byte"):
        backend.reconstruct(z(2, 6, 3), z(2, 6), torch.ones(2), z(2, 8), rgb=z(2, 6, 3))
    with pytest.raises(RuntimeError, match="img_size"):
        backend.reconstruct(z(2, 6, 3), z(2, 6), torch.ones(2), z(2, 8), K=torch.eye(3))
