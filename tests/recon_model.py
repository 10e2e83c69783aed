"""Host model of the map export (recon.hip; include/m3s_backend.h "map export"), in numpy.

Selection and colour are evaluated in f32 exactly as the op states them, so they are compared
for equality; the points are evaluated in f64 from the f32 inputs, the yardstick for the op's
f32 arithmetic.
"""
from __future__ import annotations

import numpy as np

RECORD = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"),
                   ("red", "u1"), ("green", "u1"), ("blue", "u1")])


def select(C, n_obs, thresh):
    """kept[k,n] = C[k,n] / n_obs[k] > thresh: f32 divide, f32 compare; NaN is not kept."""
    C = np.asarray(C, np.float32).reshape(len(n_obs), -1)
    n_obs = np.asarray(n_obs, np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        avg = (C / n_obs[:, None]).astype(np.float32)
        return avg > np.float32(thresh)


def quantize(uimg):
    """(uimg * 255) truncated to u8 after clamping to [0,1]; f32 product."""
    u = np.clip(np.nan_to_num(np.asarray(uimg, np.float32), nan=0.0), 0.0, 1.0)
    return (u * np.float32(255.0)).astype(np.uint8)


def act(T, p):
    """s R(q) p + t of Sim3 data T = [t(3), q(xyzw), s], all in f64; p [n,3]."""
    T = np.asarray(T, np.float64).reshape(8)
    p = np.asarray(p, np.float64)
    t, u, w, s = T[0:3], T[3:6], T[6], T[7]
    uv = 2.0 * np.cross(np.broadcast_to(u, p.shape), p)
    return s * (p + w * uv + np.cross(np.broadcast_to(u, p.shape), uv)) + t


def ray_points(X, K, img_size):
    """z ((u - cx) / fx, (v - cy) / fy, 1) in f64; X [HW,3], u = n % W, v = n // W."""
    h, w = img_size
    X = np.asarray(X, np.float64)
    K = np.asarray(K, np.float64)
    n = np.arange(h * w)
    u, v = (n % w).astype(np.float64), (n // w).astype(np.float64)
    z = X[:, 2]
    return np.stack((z * ((u - K[0, 2]) / K[0, 0]), z * ((v - K[1, 2]) / K[1, 1]), z), axis=-1)


def reconstruct(X, C, n_obs, T_WC, rgb=None, K=None, img_size=None, thresh=1.5):
    """-> dict(counts [N] i64, k [total], n [total] (the kept set in order), points [total,3] f64,
    colors [total,3] u8)."""
    X = np.asarray(X, np.float32)
    N = X.shape[0]
    HW = X.shape[1] if N else 0
    T_WC = np.asarray(T_WC, np.float32).reshape(N, 8)
    keep = select(C, n_obs, thresh) if N and HW else np.zeros((N, HW), bool)
    ks, ns, pts, cols = [], [], [], []
    for k in range(N):
        idx = np.nonzero(keep[k])[0]
        p = ray_points(X[k], K, img_size) if K is not None else X[k].astype(np.float64)
        pts.append(act(T_WC[k], p[idx]))
        cols.append(np.asarray(rgb[k], np.uint8)[idx] if rgb is not None
                    else np.zeros((len(idx), 3), np.uint8))
        ks.append(np.full(len(idx), k, np.int64))
        ns.append(idx.astype(np.int64))
    cat = lambda a, shape, dt: np.concatenate(a) if a else np.zeros(shape, dt)
    return dict(counts=keep.sum(axis=1).astype(np.int64).reshape(N),
                k=cat(ks, (0,), np.int64), n=cat(ns, (0,), np.int64),
                points=cat(pts, (0, 3), np.float64), colors=cat(cols, (0, 3), np.uint8))
