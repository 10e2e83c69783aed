"""Host models of the keyframe point-map fusion (keyframe.hip; frame.py:58-77) and of the edge
confidences (edges.hip; global_opt.py:53-67), in numpy.

The fusion and the confidences are evaluated in f32 operation by operation as the reference
writes them, so the kernels are compared with them bit for bit: numpy on the host keeps
subnormals, rounds the f32 divide correctly, and a float64 sqrt rounded to f32 is the correctly
rounded f32 sqrt.  The Sim3 transform is evaluated in f64 from the f32 inputs and the kernel's
f32 arithmetic is held to ``act_bound`` of it.
"""
from __future__ import annotations

import numpy as np

import recon_model

MODES = ("weighted_pointmap", "indep_conf", "recent")


def fuse(mode, X, C, Xn, Cn):
    """One per-point update of a keyframe (X [HW,3], C [HW,1]) with an observation (Xn, Cn):
    returns the new (X, C), f32, every product, sum and quotient rounded to f32.
      weighted_pointmap  X <- ((C X) + (Cn Xn)) / (C + Cn),  C <- C + Cn   (frame.py:74-77)
      indep_conf         where Cn > C (strictly; NaN is not greater): X <- Xn, C <- Cn  (:69-73)
      recent             X <- Xn, C <- Cn                                 (:58-61)"""
    X, Xn = (np.asarray(a, np.float32).reshape(-1, 3) for a in (X, Xn))
    C, Cn = (np.asarray(a, np.float32).reshape(-1, 1) for a in (C, Cn))
    with np.errstate(all="ignore"):
        if mode == "weighted_pointmap":
            den = C + Cn
            return ((C * X) + (Cn * Xn)) / den, den
        if mode == "indep_conf":
            m = Cn > C
            return np.where(m, Xn, X), np.where(m, Cn, C)
        if mode == "recent":
            return Xn.copy(), Cn.copy()
    raise ValueError(f"not a per-point filtering mode: {mode!r}")


def act64(T, p):
    """s R(q) p + t of Sim3 data T = [t(3), q(xyzw), s] in f64 from the f32 inputs; p [n,3]."""
    return recon_model.act(np.asarray(T, np.float32), np.asarray(p, np.float32))


ACT_K = 8


def act_bound(T, p, K=ACT_K):
    """Per-point bound [n,1] on |f32 act - act64| for a unit quaternion:
        K * 2**-24 * (5 |s| ||p||_2 + max|t|),  K = 8.

    Derivation.  The transform is uv = 2 (u x p), r = (p + w uv) + (u x uv), y = s r + t.  With
    |q| = 1 every product of a quaternion component and a point component is at most ||p||, so
    |uv| <= 2 ||p||, |p + w uv| <= 3 ||p||, |u x uv| <= 2 ||p|| and |r| <= 5 ||p||: every
    intermediate of y is bounded by M = 5 |s| ||p|| + max|t| (the rotation's, scaled by |s|, which
    is how their errors reach y).  A rounding of an intermediate adds at most 2**-24 of its
    magnitude, so at most 2**-24 M, to an output component; no output component passes through
    more than 8 roundings however the products are fused (uv: product, product, difference -- the
    doubling is exact; u x uv: product, difference; the sum; s r; + t), hence K = 8.  A plain
    unfused f32 restatement stays below 1.25 of the K = 1 unit over random T with s in
    [e^-3, e^3] and |t|, |p| in 1e-2..1e2 (tests/test_keyframe_model.py checks that on its own
    inputs), so K = 8 leaves about a 6x margin for a kernel that fuses differently, while a wrong
    sign, a conjugated quaternion or a wrong component order misses by orders of magnitude."""
    T = np.asarray(T, np.float64).reshape(8)
    p = np.asarray(p, np.float64).reshape(-1, 3)
    norm = np.sqrt((p * p).sum(axis=1, keepdims=True))
    return K * 2.0 ** -24 * (5.0 * abs(T[7]) * norm + np.abs(T[0:3]).max())


def act32_plain(T, p):
    """The transform in plain f32, one rounding per operation and nothing fused (the restatement
    that shows act_bound is not vacuous; not the kernel's contraction)."""
    T = np.asarray(T, np.float32).reshape(8)
    p = np.asarray(p, np.float32).reshape(-1, 3)
    t, u, w, s = T[0:3], T[3:6], T[6], T[7]
    two = np.float32(2.0)

    def cross(a, b):
        return np.stack((a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                         a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                         a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]), axis=-1)

    ub = np.broadcast_to(u, p.shape)
    uv = two * cross(ub, p)
    r = (p + w * uv) + cross(ub, uv)
    out = s * r + t
    assert out.dtype == np.float32
    return out


def edge_confidence(idx_i2j, idx_j2i, vm_j, vm_i, Qii, Qjj, Qji, Qij, Q_conf):
    """global_opt.py:53-67 for B pairs: Qj = sqrt(Qii[b, idx_i2j] * Qji), Qi = sqrt(Qjj[b, idx_j2i]
    * Qij) as the f32 product then the correctly rounded f32 sqrt (f64 sqrt rounded), and counts
    [B,2] int64 = (#(vm_j & Qj > Q_conf), #(vm_i & Qi > Q_conf)) with an f32 compare (NaN is not
    counted).  Indices clamp to [0, HW-1].  Returns (Qj [B,HW,1], Qi [B,HW,1], counts)."""
    idx_i2j = np.asarray(idx_i2j, np.int64)
    idx_j2i = np.asarray(idx_j2i, np.int64)
    B, HW = idx_i2j.shape
    bi = np.arange(B)[:, None]
    thr = np.float32(Q_conf)
    out = []
    counts = np.zeros((B, 2), np.int64)
    for k, (idx, vm, Qg, Qo) in enumerate(((idx_i2j, vm_j, Qii, Qji), (idx_j2i, vm_i, Qjj, Qij))):
        Qg = np.asarray(Qg, np.float32).reshape(B, HW)
        Qo = np.asarray(Qo, np.float32).reshape(B, HW)
        vm = np.asarray(vm).reshape(B, HW) != 0
        if HW == 0:
            out.append(np.zeros((B, 0, 1), np.float32))
            continue
        with np.errstate(all="ignore"):
            prod = Qg[bi, np.clip(idx, 0, HW - 1)] * Qo
            assert prod.dtype == np.float32
            q = np.sqrt(prod.astype(np.float64)).astype(np.float32)
            counts[:, k] = (vm & (q > thr)).sum(axis=1)
        out.append(q.reshape(B, HW, 1))
    return out[0], out[1], counts


def same_bits(a, b):
    """Equal f32 arrays: NaN compares as NaN (any payload), everything else by its bits."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb]))
