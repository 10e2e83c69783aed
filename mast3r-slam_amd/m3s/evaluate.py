"""Trajectory output and ATE-RMSE (BASELINE.json metric "ATE-RMSE vs ref").

* ``save_traj`` mirrors mast3r_slam/evaluate.py:23-44: one TUM line per keyframe,
  ``timestamp x y z qx qy qz qw`` of the keyframe pose with the Sim3 scale dropped
  (lietorch_utils.as_SE3, :6-13).
* ``ate_rmse`` is what the reference's evaluation runs (scripts/eval_tum.sh:44-51:
  ``evo_ape tum groundtruth.txt estimate.txt -as``): timestamp association
  (evo ``sync.associate_trajectories``, max_diff 0.01 s), Umeyama Sim(3) alignment with scale
  (evo ``geometry.umeyama_alignment(..., with_scale=True)``), then the RMSE of the translation
  errors.  evo is a pip dependency absent here (no pinned version); this restates its published
  algorithm and is checked by known-answer tests (tests/test_evaluate.py) -- parity with evo
  itself is unpinned.
* ``save_reconstruction`` replaces mast3r_slam/evaluate.py:47-70: the confidence-filtered world
  point cloud of every keyframe as a binary PLY.  The reference gathers it keyframe by keyframe on
  the host; here the device writes the file body directly (recon.hip via
  ``mast3r_slam_backends.ReconPass``) and the host only copies it to the file, a bounded number
  of keyframes at a time.  ``save_ply`` / ``read_ply`` cover the binary little-endian
  vertex-only subset the reference's ``save_ply`` (:88-106) produces through ``plyfile``.
  plyfile is a pip dependency absent here (no pinned version): the header below restates the
  PLY format as plyfile documents writing it, and parity with plyfile's exact header bytes is
  unpinned; the body is the packed structured array either way.
"""
from __future__ import annotations

import os

import numpy as np

import mast3r_slam_backends as mb


def read_tum(path):
    """TUM trajectory file -> (timestamps [n], xyz [n,3], quat xyzw [n,4]); '#' lines skipped."""
    rows = []
    with open(path) as f:
        for line in f:
            s = line.strip()
            if not s or s.startswith("#"):
                continue
            rows.append([float(v) for v in s.replace(",", " ").split()[:8]])
    a = np.asarray(rows, np.float64).reshape(-1, 8)
    return a[:, 0], a[:, 1:4], a[:, 4:8]


def write_tum(path, timestamps, xyz, quat):
    with open(path, "w") as f:
        for t, p, q in zip(timestamps, xyz, quat):
            f.write(f"{t} {p[0]} {p[1]} {p[2]} {q[0]} {q[1]} {q[2]} {q[3]}\n")


def save_traj(path, timestamps, frames):
    """evaluate.py:23-44 (uncalibrated branch): keyframe i -> timestamps[frame_id] and its
    T_WC as SE3 (t, q of the Sim3 data; scale dropped)."""
    with open(path, "w") as f:
        for i in range(len(frames)):
            kf = frames[i]
            d = kf.T_WC.data.detach().reshape(-1).cpu().numpy()
            x, y, z, qx, qy, qz, qw = d[:7]
            f.write(f"{timestamps[kf.frame_id]} {x} {y} {z} {qx} {qy} {qz} {qw}\n")


PLY_VERTEX_DTYPE = mb.RECON_DTYPE  # one vertex = one record of the map-export op


def ply_header(n):
    """Header of a binary little-endian PLY holding n x/y/z/red/green/blue vertices."""
    return ("ply\nformat binary_little_endian 1.0\n"
            f"element vertex {int(n)}\n"
            "property float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\n"
            "end_header\n").encode("ascii")


def save_ply(path, points, colors):
    """evaluate.py:88-106: points [n,3] (stored as f32), colors [n,3] (cast to u8) -> binary
    little-endian PLY, 15 bytes per vertex."""
    points = np.asarray(points).reshape(-1, 3)
    colors = np.asarray(colors).reshape(-1, 3).astype(np.uint8)
    if len(points) != len(colors):
        raise ValueError(f"save_ply: {len(points)} points but {len(colors)} colors")
    pcd = np.empty(len(points), dtype=PLY_VERTEX_DTYPE)
    pcd["x"], pcd["y"], pcd["z"] = points[:, 0], points[:, 1], points[:, 2]
    pcd["red"], pcd["green"], pcd["blue"] = colors[:, 0], colors[:, 1], colors[:, 2]
    with open(path, "wb") as f:
        f.write(ply_header(len(pcd)))
        f.write(pcd.tobytes())


def read_ply(path):
    """A file of the subset ``save_ply`` writes -> (points [n,3] f32, colors [n,3] u8)."""
    with open(path, "rb") as f:
        raw = f.read()
    end = raw.find(b"end_header\n")
    if not raw.startswith(b"ply\n") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    end += len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    if lines[1] != "format binary_little_endian 1.0":
        raise ValueError(f"{path}: only binary_little_endian 1.0 is supported ({lines[1]!r})")
    elements = [ln.split() for ln in lines if ln.startswith("element ")]
    props = [ln for ln in lines if ln.startswith("property ")]
    want = ply_header(0).decode("ascii").split("\n")[3:9]
    if len(elements) != 1 or elements[0][1] != "vertex" or props != want:
        raise ValueError(f"{path}: only one vertex element with float x y z, uchar red green blue")
    n = int(elements[0][2])
    if len(raw) - end != n * PLY_VERTEX_DTYPE.itemsize:
        raise ValueError(f"{path}: body holds {len(raw) - end} bytes, expected {n} vertices")
    pcd = np.frombuffer(raw, dtype=PLY_VERTEX_DTYPE, count=n, offset=end)
    points = np.stack((pcd["x"], pcd["y"], pcd["z"]), axis=-1) if n else np.zeros((0, 3), np.float32)
    colors = (np.stack((pcd["red"], pcd["green"], pcd["blue"]), axis=-1) if n
              else np.zeros((0, 3), np.uint8))
    return points, colors


def _stack_keyframes(keyframes, calib):
    """Any duck-typed keyframe sequence (a list of m3s.frame.Frame) -> the store's layout."""
    import torch

    from .global_opt import quantize_uimg

    kfs = [keyframes[i] for i in range(len(keyframes))]
    X = torch.stack([kf.X_canon.reshape(-1, 3) for kf in kfs]).contiguous()
    if all(hasattr(kf, "C") and hasattr(kf, "N") for kf in kfs):
        # the op divides C by N itself, as it does for a store
        C = torch.stack([kf.C.reshape(-1) for kf in kfs]).contiguous()
        n_obs = torch.tensor([float(kf.N) for kf in kfs], device=X.device)
    else:  # C / N of each keyframe; the op then divides by 1, which is exact
        C = torch.stack([kf.get_average_conf().reshape(-1) for kf in kfs]).contiguous()
        n_obs = torch.ones((len(kfs),), device=X.device)
    T_WC = torch.stack([kf.T_WC.data.reshape(8) for kf in kfs]).to(X.device).contiguous()
    uimgs = [getattr(kf, "uimg", None) for kf in kfs]
    rgb = None
    if all(u is not None for u in uimgs):
        rgb = torch.stack([quantize_uimg(u.to(X.device)).reshape(-1, 3) for u in uimgs]).contiguous()
    K, img_size = None, None
    if calib:
        K = kfs[0].K.to(X.device)
        if uimgs[0] is not None and uimgs[0].dim() == 3:
            img_size = tuple(uimgs[0].shape[:2])
        else:
            img_size = tuple(kfs[0].img.shape[-2:])
    return X, C, n_obs, T_WC, rgb, K, img_size


def save_reconstruction(savedir, filename, keyframes, c_conf_threshold, use_calib=None,
                        chunk_keyframes=32):
    """evaluate.py:47-70: every keyframe's points with average confidence above
    ``c_conf_threshold``, in the world frame (on their pixel rays through K when ``use_calib``;
    None reads config["use_calib"]), with their colours, as ``savedir/filename`` (binary PLY).

    With a ``KeyframeStore`` (``keep_rgb=True`` for colours, else 0,0,0) the store's buffers are
    read in place: one count over all keyframes sizes the header, then the body is emitted on the
    device and copied to the file ``chunk_keyframes`` keyframes at a time, so host memory stays
    bounded and no per-point work runs on the host.  Any other keyframe sequence (a list of
    ``Frame``) is stacked once and takes the same path.  Unlike the reference this does not
    overwrite ``keyframe.X_canon`` with the ray-constrained points.  Returns the number of points.
    """
    import torch

    from .config import config as _config
    from .global_opt import KeyframeStore

    calib = bool(_config["use_calib"] if use_calib is None else use_calib)
    os.makedirs(savedir, exist_ok=True)
    N = len(keyframes)
    if isinstance(keyframes, KeyframeStore):
        st = keyframes
        X, C, n_obs, T_WC = st.X[:N], st.C[:N], st.n_obs[:N], st.T_WC[:N]
        rgb = st.rgb[:N] if st.rgb is not None else None
        K, img_size = (st.K.to(X.device), (st.h, st.w)) if calib else (None, None)
    elif N > 0:
        X, C, n_obs, T_WC, rgb, K, img_size = _stack_keyframes(keyframes, calib)
    path = os.path.join(savedir, filename)
    if N == 0:
        save_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8))
        return 0
    thresh = float(c_conf_threshold)
    counts, _ = mb.ReconPass(X, C, n_obs, T_WC, rgb, K, img_size, thresh).count()
    counts = counts.cpu().numpy()  # the one synchronisation that sizes the file
    total = int(counts.sum())
    step = max(int(chunk_keyframes), 1)
    with open(path, "wb") as f:
        f.write(ply_header(total))
        for lo in range(0, N, step):
            hi = min(lo + step, N)
            n = int(counts[lo:hi].sum())
            if n == 0:
                continue
            p = mb.ReconPass(X[lo:hi], C[lo:hi], n_obs[lo:hi], T_WC[lo:hi],
                             rgb[lo:hi] if rgb is not None else None, K, img_size, thresh)
            p.count()
            body = torch.empty((mb.RECON_RECORD_BYTES * n,), dtype=torch.uint8, device=X.device)
            p.emit(body, n)
            f.write(body.cpu().numpy().tobytes())
    return total


def associate(stamps_ref, stamps_est, max_diff=0.01, offset=0.0):
    """evo sync.associate_trajectories: for every stamp of the SHORTER trajectory, the nearest
    stamp of the longer one (plus offset) if within max_diff.  Returns index arrays
    (into ref, into est)."""
    stamps_ref = np.asarray(stamps_ref, np.float64)
    stamps_est = np.asarray(stamps_est, np.float64)
    est_longer = len(stamps_est) > len(stamps_ref)
    short, long_ = (stamps_ref, stamps_est + offset) if est_longer else (stamps_est, stamps_ref - offset)
    i_s, i_l = [], []
    for k, s in enumerate(short):
        d = np.abs(long_ - s)
        j = int(np.argmin(d))
        if d[j] <= max_diff:
            i_s.append(k)
            i_l.append(j)
    i_s, i_l = np.asarray(i_s, int), np.asarray(i_l, int)
    return (i_s, i_l) if est_longer else (i_l, i_s)


def umeyama(x, y, with_scale=True):
    """evo geometry.umeyama_alignment: (R, t, c) minimising sum ||y - (c R x + t)||^2,
    x, y [3,n]."""
    m, n = x.shape
    mx, my = x.mean(axis=1), y.mean(axis=1)
    sigma_x = 1.0 / n * np.sum(np.linalg.norm(x - mx[:, None], axis=0) ** 2)
    cov = 1.0 / n * (y - my[:, None]) @ (x - mx[:, None]).T
    u, d, v = np.linalg.svd(cov)
    s = np.eye(m)
    if np.linalg.det(u) * np.linalg.det(v) < 0.0:
        s[m - 1, m - 1] = -1.0
    r = u @ s @ v
    c = 1.0 / sigma_x * np.trace(np.diag(d) @ s) if with_scale else 1.0
    t = my - c * (r @ mx)
    return r, t, c


def ate_rmse(ref, est, max_diff=0.01, offset=0.0, with_scale=True):
    """APE (translation part) RMSE after association and Sim(3) alignment, as
    ``evo_ape tum ref est -as``.  ref / est: (timestamps, xyz[, quat]) tuples or TUM paths.
    Returns (rmse, details dict)."""
    if isinstance(ref, str):
        ref = read_tum(ref)
    if isinstance(est, str):
        est = read_tum(est)
    i_r, i_e = associate(ref[0], est[0], max_diff, offset)
    if len(i_r) < 3:
        raise ValueError(f"only {len(i_r)} associated poses; need >= 3 for a Sim(3) alignment")
    P = np.asarray(ref[1], np.float64)[i_r].T
    Q = np.asarray(est[1], np.float64)[i_e].T
    r, t, c = umeyama(Q, P, with_scale)
    err = np.linalg.norm(P - (c * (r @ Q) + t[:, None]), axis=0)
    rmse = float(np.sqrt(np.mean(err ** 2)))
    return rmse, dict(n=len(i_r), R=r, t=t, scale=c, errors=err, mean=float(err.mean()),
                      max=float(err.max()))
