"""Host model of RoPE2D (include/m3s_backend.h, "RoPE2D"; csrc/rope.hip): numpy.

tokens [B,N,H,D], pos [B,N,2] int64 (y, x).  With Q = D/4 a head is [u_Y | v_Y | u_X | v_X]; for
axis A and i < Q:  theta = float(pos_A) * (F0 / base^(i/Q)),  u' = u cos(theta) - v sin(theta),
v' = v cos(theta) + u sin(theta).

* ``model_f64``: the formula in f64 on the given (f32 or f16) inputs: what the bounds are relative to.
* ``bound``: with u = 2^-24 and S = |u_in| + |v_in|,

      |got - model_f64| <= S u (|theta| Ta + Tc + 2)          (+ half an f16 ulp of the model value)

  An f32 angle Ta u relatively off moves cos and sin by at most |theta| Ta u; the f32 cos / sin add
  Tc u; the two products and the sum add at most (0.5 + 0.5 + 0.5) u S, rounded up to 2.
  Ta and Tc are those of the REFERENCE's own f32 run, recorded in the fixture
  (tests/golden/make_rope_golden.py); ``tol`` doubles them, at least 2.
* ``grid_positions`` / ``wild_positions`` / ``make_inputs``: inputs of the tested kind.
"""
import numpy as np

U = 2.0 ** -24
BASE = 100.0


def tol(recorded):
    """A recorded term of the bound, in u: twice what the reference's own f32 run showed, at
    least 2."""
    return max(2.0 * float(recorded), 2.0)


def grid_positions(B, gh, gw, step=(0, 0)):
    """(y, x) of a gh x gw patch grid, row-major, as the reference's PositionGetter lists them;
    batch item b is shifted by b * step so that batch items differ.  -> [B, gh*gw, 2] int64."""
    y, x = np.meshgrid(np.arange(gh), np.arange(gw), indexing="ij")
    p = np.stack([y.ravel(), x.ravel()], axis=-1).astype(np.int64)
    return np.stack([p + b * np.asarray(step, np.int64) for b in range(B)])


def wild_positions(B, N, seed):
    """Arbitrary int64 positions in [-300, 300], with 0, 200 and a negative one placed."""
    rng = np.random.default_rng(seed)
    p = rng.integers(-300, 301, (B, N, 2)).astype(np.int64)
    p[0, 0] = (0, 200)
    p[-1, -1] = (-7, 0)
    return p


def make_inputs(B, N, H, D, seed, dtype=np.float32):
    """Standard-normal tokens of ``dtype`` [B,N,H,D], none of them zero."""
    rng = np.random.default_rng(seed)
    t = rng.standard_normal((B, N, H, D))
    t = np.where(np.abs(t) < 1e-3, 1e-3, t)
    return t.astype(dtype)


def inv_freq_f64(D, base=BASE, F0=1.0):
    Q = D // 4
    return float(F0) / np.power(float(np.float32(base)), np.arange(Q, dtype=np.float64) / Q)


def angles_f64(pos, D, base=BASE, F0=1.0):
    """theta [B,N,2,Q] in f64; float(pos) is the f32 conversion the op makes."""
    return pos.astype(np.float32).astype(np.float64)[..., None] * inv_freq_f64(D, base, F0)


def _split(tokens):
    B, N, H, D = tokens.shape
    t = tokens.astype(np.float64).reshape(B, N, H, 2, 2, D // 4)  # axis, u|v, i
    return t[..., 0, :], t[..., 1, :]


def model_f64(tokens, pos, base=BASE, F0=1.0):
    u, v = _split(tokens)
    th = angles_f64(pos, tokens.shape[3], base, F0)[:, :, None]   # B,N,1,2,Q
    c, s = np.cos(th), np.sin(th)
    return np.stack([u * c - v * s, v * c + u * s], axis=-2).reshape(tokens.shape)


def round_to(x64, dtype):
    """The one rounding of the f64 model to the token dtype."""
    return np.asarray(x64, np.float64).astype(dtype)


def half_ulp_f16(x64):
    a = np.abs(np.asarray(x64, np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return 0.5 * 2.0 ** (e - 10)


def bound(tokens, pos, Ta, Tc, base=BASE, F0=1.0, dtype=np.float32, model=None):
    """Elementwise bound of |got - model_f64| for a result of ``dtype`` ([B,N,H,D], f64)."""
    u, v = _split(tokens)
    S = np.abs(u) + np.abs(v)
    th = np.abs(angles_f64(pos, tokens.shape[3], base, F0))[:, :, None]
    b = S * U * (th * Ta + Tc + 2.0)
    b = np.stack([b, b], axis=-2).reshape(tokens.shape)
    if np.dtype(dtype) == np.float16:
        if model is None:
            model = model_f64(tokens, pos, base, F0)
        b = b + half_ulp_f16(model)
    return b
