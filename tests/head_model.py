"""Host model of the head finish (include/m3s_backend.h, "head finish"; csrc/head.hip): numpy.

* ``model_f32``: the op's f32 operations one by one, the descriptor's sum of squares sequential.
  D is the op's D bit for bit (IEEE multiply, add, sqrt and divide only); X, C, Q carry numpy's own
  f32 expm1 / exp and agree with the op to a tolerance.
* ``model_f64``: the same formulas in f64 on the same f32 inputs: what the bounds are relative to.
* ``bound_*``: componentwise relative bounds against ``model_f64``, in units of u = 2^-24.
* ``shuffle``: the token layout's index identity; ``make_inputs``: raw heads of the tested kind.
"""
import numpy as np

U = 2.0 ** -24
P = 16
CLIP = np.float32(1e-8)
CONF = (1.0, float("inf"))
DESC_CONF = (0.0, float("inf"))


def shuffle(feat, H, W, p=P):
    """[B,S,(F+1)*p*p] tokens -> [B,F+1,H,W]: pixel (v,u), channel c is token (v/p)(W/p) + u/p,
    offset c p^2 + (v%p) p + (u%p)."""
    B, S, width = feat.shape
    C1 = width // (p * p)
    t = feat.reshape(B, H // p, W // p, C1, p, p)       # b, ty, tx, c, i, j
    return np.ascontiguousarray(t.transpose(0, 3, 1, 4, 2, 5)).reshape(B, C1, H, W)


def unshuffle(planar, p=P):
    """[B,F+1,H,W] -> tokens [B,S,(F+1)*p*p], the inverse of ``shuffle``."""
    B, C1, H, W = planar.shape
    t = planar.reshape(B, C1, H // p, p, W // p, p)     # b, c, ty, i, tx, j
    return np.ascontiguousarray(t.transpose(0, 2, 4, 1, 3, 5)).reshape(B, (H // p) * (W // p), C1 * p * p)


def _conf(a, vmin, vmax, dt):
    with np.errstate(all="ignore"):
        e = np.exp(a.astype(dt))
        lim = dt(vmax) - dt(vmin)
        return (dt(vmin) + np.where(e > lim, lim, e)).astype(dt)  # a NaN stays NaN


def _model(pts, planar, ds, conf, desc_conf, dt):
    """pts [B,4,H,W], planar [B,F+1,H,W] or None, f32 -> X, C, D, Q in dtype dt at [::ds]."""
    with np.errstate(all="ignore"):
        p = pts[:, :, ::ds, ::ds].astype(dt)
        x, y, z, a = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
        s = (x * x + y * y) + z * z
        d = np.sqrt(s)
        m = np.where(d < dt(CLIP), dt(CLIP), d)             # a NaN d stays NaN
        g = np.expm1(d)
        X = np.stack([(x / m) * g, (y / m) * g, (z / m) * g], axis=-1)
        C = _conf(a, conf[0], conf[1], dt)
        if planar is None:
            return X.astype(dt), C, None, None
        f = planar[:, :, ::ds, ::ds].astype(dt)
        F = f.shape[1] - 1
        acc = f[:, 0] * f[:, 0]
        for c in range(1, F):
            acc = acc + f[:, c] * f[:, c]
        n = np.sqrt(acc)
        D = np.stack([f[:, c] / n for c in range(F)], axis=-1)
        Q = _conf(planar[:, F, ::ds, ::ds], desc_conf[0], desc_conf[1], dt)
        return X.astype(dt), C, D.astype(dt), Q


def model_f32(pts, planar, ds=1, conf=CONF, desc_conf=DESC_CONF):
    return _model(pts, planar, ds, conf, desc_conf, np.float32)


def model_f64(pts, planar, ds=1, conf=CONF, desc_conf=DESC_CONF):
    return _model(pts, planar, ds, conf, desc_conf, np.float64)


def tol(recorded):
    """The exp / expm1 term of a bound, in u: twice what the reference's own f32 function showed
    against f64 (recorded in the fixture), at least 2."""
    return max(2.0 * float(recorded), 2.0)


def kappa(d):
    """Condition number of expm1 at d: d e^d / (e^d - 1), -> 1 as d -> 0."""
    d = np.asarray(d, np.float64)
    with np.errstate(all="ignore"):
        k = d * np.exp(d) / np.expm1(d)
    return np.where(d > 0, k, 1.0)


def bound_D(F):
    """A sum of F rounded squares in any order is off by at most F u relative; the sqrt halves
    that and adds u; the divide adds u."""
    return (F / 2.0 + 2.0) * U


def bound_X(d, T_expm1):
    """3.5 u for the direction (d's 2.5 u and the divide), 1 u for the product, d's own 2.5 u
    through expm1, and expm1's T_expm1.  d: the f64 model's norm at each pixel ([...], broadcast
    over the 3 components by the caller)."""
    return (4.5 + 2.5 * kappa(d) + T_expm1) * U


def bound_CQ(T_exp):
    return (1.0 + T_exp) * U


def norm_f64(pts, ds=1):
    p = pts[:, :3, ::ds, ::ds].astype(np.float64)
    return np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])


def rel_err_u(got, ref64):
    """|got - ref| / |ref| in u over the finite entries of ref (0 where both are 0)."""
    got = np.asarray(got, np.float64)
    with np.errstate(all="ignore"):
        e = np.abs(got - ref64) / np.abs(ref64) / U
    e = np.where((got == ref64), 0.0, e)
    return np.where(np.isfinite(ref64), e, 0.0)


def same_specials(got, ref):
    """NaN positions, inf positions and inf signs agree."""
    got, ref = np.asarray(got), np.asarray(ref)
    return (np.array_equal(np.isnan(got), np.isnan(ref))
            and np.array_equal(np.isposinf(got), np.isposinf(ref))
            and np.array_equal(np.isneginf(got), np.isneginf(ref)))


def make_inputs(B, H, W, F, seed):
    """Raw heads of the kind the bounds were checked on: random directions, |xyz| log-uniform in
    [1e-3, 4], both logits uniform in [-4, 4], standard-normal descriptors.
    -> pts [B,4,H,W], planar [B,F+1,H,W] (f32)."""
    rng = np.random.default_rng(seed)
    dirs = rng.standard_normal((B, 3, H, W))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    d = np.exp(rng.uniform(np.log(1e-3), np.log(4.0), (B, 1, H, W)))
    pts = np.concatenate([dirs * d, rng.uniform(-4, 4, (B, 1, H, W))], axis=1).astype(np.float32)
    planar = np.concatenate([rng.standard_normal((B, F, H, W)), rng.uniform(-4, 4, (B, 1, H, W))],
                            axis=1).astype(np.float32)
    return pts, planar
