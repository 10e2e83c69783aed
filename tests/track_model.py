"""Host models of one iteration of the frame tracker's accumulate (csrc/track.hip,
track_accum_kernel, both modes): numpy.  TEST INFRASTRUCTURE ONLY.

* ``sums_f64``: the float64 sums H = A^T A, g = -A^T b, cost = 0.5 b^T b of the oracle's solve
  (oracle/track_oracle.py, ``_solve`` up to H, g, cost with the residual / Jacobian code of
  opt_pose_ray_dist_sim3 / opt_pose_calib_sim3), evaluated at a given T_CkCf.  What the bounds
  are relative to.
* ``sums_f32``: the kernel's per-point arithmetic in float32, element-wise and in the kernel's
  expression order, without FMA contraction; the per-row products a_i a_j, -a_i b, b b are formed
  in float32, cast to float64 and summed there.  ``mutate`` applies one deliberate error (MUTATIONS)
  to show that the bound separates a wrong kernel from a right one.
* ``errors``: the normalised differences the tests bound (TOL):
      |H_ij - Ho_ij| / sqrt(Ho_ii Ho_jj),  |g_i - go_i| / sqrt(Ho_ii 2 co),  |c - co| / co
  By Cauchy-Schwarz each normaliser bounds the sum of the absolute values of the entry's terms.
* ``unpack36`` / ``pack36``: the kernel's 36 sums (H upper triangle row-major 28, g 7, sum b^2 1).
* ``start_pose``, ``truncate``, ``anisotropic``, ``unit_scale``: test inputs on top of
  track_oracle.make_tracking_pair.
"""
import numpy as np

from oracle import track_oracle as TO

TOL = 2e-5
CHUNK = 1 << 16

# name -> modes it applies to
MUTATIONS = {
    "neg_j4": ("rays", "calib"),        # negate the m2*x - m0*z Jacobian entry
    "swap_j3_j5": ("rays", "calib"),    # swap J[3] and J[5]
    "huber_one": ("rays", "calib"),     # huber weight = 1
    "dist_s0": ("rays", "calib"),       # whiten the distance (log-depth) row with s0 instead of s1
    "drop_last": ("rays", "calib"),     # drop the last point
    "dup_first": ("rays", "calib"),     # count point 0 twice
    "ignore_ok": ("calib",),            # no validity mask at all (w2 = 1)
    "ignore_vmeas": ("calib",),         # ok without valid_meas_k
    "fx_for_v": ("calib",),             # the v row uses fx
    "no_zinv_logz": ("calib",),         # the log-z row's Jacobian without zinv
}


def sigmas(mode, cfg):
    return (cfg["sigma_ray"], cfg["sigma_dist"]) if mode == "rays" else (cfg["sigma_pixel"], cfg["sigma_depth"])


# ----------------------------------------------------------------------------- float64 sums


def _rows_f64(mode, p, T, cfg, hw, sl):
    """sqrt information [n,R], residual [n,R], Jacobian [n,R,7] of the points in slice sl."""
    Xf = np.asarray(p["Xf"][sl], np.float64)
    Qk = np.asarray(p["Qk"][sl], np.float64)
    v = np.asarray(p["valid"][sl], np.float64)
    sq = np.sqrt(Qk)
    X = TO.sim3_act(T, Xf)
    if mode == "rays":
        si = np.concatenate([np.repeat((1.0 / cfg["sigma_ray"]) * v * sq, 3, axis=1),
                             (1.0 / cfg["sigma_dist"]) * v * sq], axis=1)
        rd_k = TO.point_to_ray_dist(np.asarray(p["Xk"][sl], np.float64))
        rd_f, drd = TO.point_to_ray_dist(X, jacobian=True)
        r = rd_k - rd_f
        J = -drd @ TO.act_jac(X)
        aux = dict(X=X)
    else:
        si = np.concatenate([np.repeat((1.0 / cfg["sigma_pixel"]) * v * sq, 2, axis=1),
                             (1.0 / cfg["sigma_depth"]) * v * sq], axis=1)
        K = np.asarray(p["K"], np.float64)
        vm = np.asarray(p["valid_meas_k"][sl], bool)
        pz, D, vp = TO.project_calib(X, K, hw, cfg["pixel_border"], cfg["depth_eps"])
        si = (vp[:, None] & vm).astype(np.float64) * si
        r = np.asarray(p["meas_k"][sl], np.float64) - pz
        J = -D @ TO.act_jac(X)
        aux = dict(X=X, uv=pz[:, :2], ok=(vp[:, None] & vm)[:, 0])
    return si, r, J, aux


def sums_f64(mode, p, T, cfg, hw=None):
    """(H [7,7], g [7], cost, aux) at T_CkCf = T (float64 of the given values).  aux: ``wr`` the
    whitened residuals si*r [n,R], ``si`` [n,R], ``X`` the transformed points, and for calib ``uv``
    and ``ok`` (project_calib's mask and valid_meas_k)."""
    T = np.asarray(T, np.float64).reshape(8)
    n = p["Xf"].shape[0]
    H = np.zeros((7, 7))
    g = np.zeros(7)
    bb = 0.0
    auxs = []
    with np.errstate(all="ignore"):
        for s in range(0, n, CHUNK):
            si, r, J, aux = _rows_f64(mode, p, T, cfg, hw, slice(s, min(n, s + CHUNK)))
            wr = si * r
            ris = si * np.sqrt(TO.huber(wr, cfg["huber"]))
            A = (ris[..., None] * J).reshape(-1, 7)
            b = (ris * r).reshape(-1, 1)
            H += A.T @ A
            g += (-A.T @ b).reshape(-1)
            bb += float((b.T @ b)[0, 0])
            aux.update(wr=wr, si=si)
            auxs.append(aux)
    aux = {k: np.concatenate([a[k] for a in auxs]) for k in auxs[0]}
    return H, g, 0.5 * bb, aux


# ----------------------------------------------------------------------------- float32 model

F = np.float32


def _act_so3_f32(q, X):
    uv0 = F(2) * (q[1] * X[2] + (-q[2]) * X[1])
    uv1 = F(2) * (q[2] * X[0] + (-q[0]) * X[2])
    uv2 = F(2) * (q[0] * X[1] + (-q[1]) * X[0])
    y0 = (q[3] * uv0 + X[0]) + (q[1] * uv2 + (-q[2]) * uv1)
    y1 = (q[3] * uv1 + X[1]) + (q[2] * uv0 + (-q[0]) * uv2)
    y2 = (q[3] * uv2 + X[2]) + (q[0] * uv1 + (-q[1]) * uv0)
    return y0, y1, y2


def _jrow(m0, m1, m2, x, y, z, mutate):
    J = [-m0, -m1, -m2, m1 * z - m2 * y, m2 * x - m0 * z, m0 * y - m1 * x,
         -((m0 * x + m1 * y) + m2 * z)]
    if mutate == "neg_j4":
        J[4] = -J[4]
    if mutate == "swap_j3_j5":
        J[3], J[5] = J[5], J[3]
    return J


def _robust(si, r, k, mutate):
    wr = np.abs(si * r)
    w = np.where(wr < k, F(1), k / wr)
    if mutate == "huber_one":
        w = np.ones_like(wr)
    return si * np.sqrt(w)


def _row(S, J, ris, r, cnt):
    """One residual row of every point into the 36 float64 sums (cnt: how often a point counts)."""
    a = [ris * J[c] for c in range(7)]
    b = ris * r
    k = 0
    for i in range(7):
        for j in range(i, 7):
            S[k] += np.dot((a[i] * a[j]).astype(np.float64), cnt)
            k += 1
    for i in range(7):
        S[28 + i] += np.dot(((-a[i]) * b).astype(np.float64), cnt)
    S[35] += np.dot((b * b).astype(np.float64), cnt)


def sums_f32(mode, p, T, cfg, hw=None, mutate=None):
    """(H, g, cost) of the float32 restatement of track_accum_kernel<mode> at T_CkCf = T."""
    assert mutate is None or mode in MUTATIONS[mutate], (mutate, mode)
    T = [F(t) for t in np.asarray(T, np.float32).reshape(8)]
    n = p["Xf"].shape[0]
    Xf = np.asarray(p["Xf"], np.float32)
    cnt = np.ones(n)
    if mutate == "drop_last":
        cnt[n - 1] = 0.0
    if mutate == "dup_first":
        cnt[0] = 2.0
    sig0, sig1 = sigmas(mode, cfg)
    s0, s1, k = F(1.0 / sig0), F(1.0 / sig1), F(cfg["huber"])
    if mutate == "dist_s0":
        s1 = s0
    one, zero = F(1), F(0)
    S = np.zeros(36)
    with np.errstate(all="ignore"):
        r0, r1, r2 = _act_so3_f32(T[3:7], (Xf[:, 0], Xf[:, 1], Xf[:, 2]))
        x, y, z = T[7] * r0 + T[0], T[7] * r1 + T[1], T[7] * r2 + T[2]
        sq = np.sqrt(np.asarray(p["Qk"], np.float32)[:, 0])
        v = np.where(np.asarray(p["valid"])[:, 0], one, zero)
        if mode == "rays":
            d = np.sqrt((x * x + y * y) + z * z)
            dinv = one / d
            rf0, rf1, rf2 = dinv * x, dinv * y, dinv * z
            Xk = np.asarray(p["Xk"], np.float32)
            k0, k1, k2 = Xk[:, 0], Xk[:, 1], Xk[:, 2]
            dk = np.sqrt((k0 * k0 + k1 * k1) + k2 * k2)
            dkinv = one / dk
            e0, e1, e2 = dkinv * k0 - rf0, dkinv * k1 - rf1, dkinv * k2 - rf2
            e3 = dk - d
            dinv2 = dinv * dinv
            si_r, si_d = (s0 * v) * sq, (s1 * v) * sq
            J = _jrow(dinv * (one - dinv2 * (x * x)), dinv * (zero - dinv2 * (x * y)),
                      dinv * (zero - dinv2 * (x * z)), x, y, z, mutate)
            _row(S, J, _robust(si_r, e0, k, mutate), e0, cnt)
            J = _jrow(dinv * (zero - dinv2 * (y * x)), dinv * (one - dinv2 * (y * y)),
                      dinv * (zero - dinv2 * (y * z)), x, y, z, mutate)
            _row(S, J, _robust(si_r, e1, k, mutate), e1, cnt)
            J = _jrow(dinv * (zero - dinv2 * (z * x)), dinv * (zero - dinv2 * (z * y)),
                      dinv * (one - dinv2 * (z * z)), x, y, z, mutate)
            _row(S, J, _robust(si_r, e2, k, mutate), e2, cnt)
            J = _jrow(rf0, rf1, rf2, x, y, z, mutate)
            _row(S, J, _robust(si_d, e3, k, mutate), e3, cnt)
        else:
            K = np.asarray(p["K"], np.float32)
            fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
            pb = cfg["pixel_border"]
            pb_lo, pb_hi_u, pb_hi_v = F(pb), F(hw[1] - 1 - pb), F(hw[0] - 1 - pb)
            z_eps = F(cfg["depth_eps"])
            u = (fx * x + cx * z) / z
            vv = (fy * y + cy * z) / z
            valid_z = z > z_eps
            vmeas = np.asarray(p["valid_meas_k"])[:, 0].astype(bool)
            ok = (u > pb_lo) & (u < pb_hi_u) & (vv > pb_lo) & (vv < pb_hi_v) & valid_z
            if mutate != "ignore_vmeas":
                ok = ok & vmeas
            if mutate == "ignore_ok":
                ok = np.ones_like(ok)
            logz = np.where(valid_z, np.log(np.where(valid_z, z, one)), zero)
            m = np.asarray(p["meas_k"], np.float32)
            e0, e1, e2 = m[:, 0] - u, m[:, 1] - vv, m[:, 2] - logz
            zinv = one / z
            w2 = np.where(ok, one, zero)
            si_p, si_z = w2 * ((s0 * v) * sq), w2 * ((s1 * v) * sq)
            o = np.zeros_like(x)
            J = _jrow(fx * zinv, o, ((-fx * x) * zinv) * zinv, x, y, z, mutate)
            _row(S, J, _robust(si_p, e0, k, mutate), e0, cnt)
            fv = fx if mutate == "fx_for_v" else fy
            J = _jrow(o, fv * zinv, ((-fv * y) * zinv) * zinv, x, y, z, mutate)
            _row(S, J, _robust(si_p, e1, k, mutate), e1, cnt)
            J = _jrow(o, o, np.ones_like(x) if mutate == "no_zinv_logz" else zinv, x, y, z, mutate)
            _row(S, J, _robust(si_z, e2, k, mutate), e2, cnt)
    return unpack36(S)


# ----------------------------------------------------------------------------- comparison


def unpack36(S):
    """The kernel's 36 sums -> (H [7,7] symmetric, g [7], cost = 0.5 S[35])."""
    S = np.asarray(S, np.float64)
    H = np.zeros((7, 7))
    iu = np.triu_indices(7)
    H[iu] = S[:28]
    H = H + np.triu(H, 1).T
    return H, S[28:35].copy(), 0.5 * float(S[35])


def pack36(H, g, cost):
    return np.concatenate([np.asarray(H)[np.triu_indices(7)], g, [2.0 * cost]])


def errors(H, g, c, Ho, go, co):
    """The worst normalised differences (H, g, cost); a non-finite value gives inf."""
    d = np.sqrt(np.diag(Ho))
    with np.errstate(all="ignore"):
        eH = np.abs(H - Ho) / np.outer(d, d)
        eg = np.abs(g - go) / (d * np.sqrt(2.0 * co))
        ec = abs(c - co) / co
    out = []
    for e in (eH, eg, ec):
        e = np.asarray(e, np.float64)
        out.append(float(e.max()) if np.isfinite(e).all() else float("inf"))
    return tuple(out)


# ----------------------------------------------------------------------------- inputs


def true_pose(p):
    """The generating T_CkCf of a make_tracking_pair dict (float64 of its float32 poses)."""
    return TO.sim3_mul(TO.sim3_inv(np.asarray(p["T_WCk"], np.float64)), np.asarray(p["T_WCf_true"], np.float64))


def start_pose(p, pert, seed):
    """The generating T_CkCf retracted by pert * (7 standard normals), rounded to float32: the
    pose both models and, under an identity keyframe pose, the kernel evaluate at."""
    xi = pert * np.random.default_rng(seed).standard_normal(7)
    return TO.sim3_retr(true_pose(p), xi).astype(np.float32)


def truncate(p, n):
    """The first n points of a pair (poses and K kept)."""
    per_point = ("Xf", "Xk", "Qk", "valid", "meas_k", "valid_meas_k")
    return {k: (np.ascontiguousarray(v[:n]) if k in per_point else v) for k, v in p.items()}


def shape_for(n):
    """An image shape (h, w), w about 4/3 h, with more than n pixels: a pair truncated to n keeps
    points from several image rows (a well-posed pose problem at any n)."""
    w = max(4, int(np.ceil(np.sqrt(n * 4.0 / 3.0))))
    return (n + w - 1) // w + 1, w


def anisotropic(p, fy_scale, noise, seed):
    """The same keyframe pixels, depths and relative pose under a camera with fy = fy_scale * fx
    (make_tracking_pair has fx == fy, which hides a mixed-up focal length)."""
    rng = np.random.default_rng(seed)
    q = dict(p)
    K = np.array(p["K"], np.float64)
    K[1, 1] *= fy_scale
    Xk = np.asarray(p["Xk"], np.float64) * np.array([1.0, 1.0 / fy_scale, 1.0])
    Xf = TO.sim3_act(TO.sim3_inv(true_pose(p)), Xk) + noise * rng.standard_normal(Xk.shape)
    q.update(K=K.astype(np.float32), Xk=Xk.astype(np.float32), Xf=Xf.astype(np.float32))
    return q


def with_outliers(p, frac, size, seed):
    """Gross errors of standard deviation ``size`` on a share ``frac`` of the frame points, and
    points 0 and n-1 valid: the huber weight is on both branches whatever the start pose, and
    the first and the last point count."""
    rng = np.random.default_rng(seed)
    q = dict(p)
    n = p["Xf"].shape[0]
    out = rng.random(n) < frac
    out[0] = out[n - 1] = False
    Xf = np.asarray(p["Xf"], np.float64) + size * out[:, None] * rng.standard_normal((n, 3))
    valid = np.array(p["valid"])
    valid[0] = valid[n - 1] = True
    q.update(Xf=Xf.astype(np.float32), valid=valid)
    return q


MASK_GROUPS = ("kept", "behind", "left", "right", "top", "bottom", "no_meas", "invalid")


def masked_calib(p, hw, T, border, seed, share=0.06):
    """A calib pair whose frame points, seen from the keyframe camera at T_CkCf = T, fall into
    disjoint groups (MASK_GROUPS; ``share`` of the points each but "kept"): behind the camera
    (z = -1), outside each of the four borders by 1 to 6 px, valid_meas_k false, valid false.
    Points 0 and n-1 stay "kept".  Returns the pair and the group index of every point."""
    rng = np.random.default_rng(seed)
    T = np.asarray(T, np.float64).reshape(8)
    n = p["Xf"].shape[0]
    h, w = hw
    K = np.asarray(p["K"], np.float64)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    grp = rng.choice(len(MASK_GROUPS), size=n, p=[1.0 - 7 * share] + [share] * 7)
    grp[0] = grp[n - 1] = 0
    X = TO.sim3_act(T, np.asarray(p["Xf"], np.float64))
    z = X[:, 2].copy()
    u = (fx * X[:, 0] + cx * z) / z
    v = (fy * X[:, 1] + cy * z) / z
    # every point at least 1 px inside the border (a large start error pushes some out on its
    # own), then the groups out of it
    u = np.clip(u, border + 1.0, w - 1 - border - 1.0)
    v = np.clip(v, border + 1.0, h - 1 - border - 1.0)
    off = 1.0 + 5.0 * rng.random(n)
    u = np.where(grp == 2, border - off, u)
    u = np.where(grp == 3, w - 1 - border + off, u)
    v = np.where(grp == 4, border - off, v)
    v = np.where(grp == 5, h - 1 - border + off, v)
    z = np.where(grp == 1, -1.0, z)
    X = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], axis=-1)
    q = dict(p)
    vm = np.array(p["valid_meas_k"])
    vm[grp == 6] = False
    valid = np.array(p["valid"])
    valid[grp == 7] = False
    valid[0] = valid[n - 1] = True
    q.update(Xf=TO.sim3_act(TO.sim3_inv(T), X).astype(np.float32), valid_meas_k=vm, valid=valid)
    return q, grp


def border_distance(uv, hw, border):
    """Distance in px of every projected point to the nearest of the four border lines."""
    h, w = hw
    return np.minimum.reduce([np.abs(uv[:, 0] - border), np.abs(uv[:, 0] - (w - 1 - border)),
                              np.abs(uv[:, 1] - border), np.abs(uv[:, 1] - (h - 1 - border))])


def model_case(mode, hw, pert, cfg, seed=11, noise=0.003):
    """The input of tests/test_track_model.py: a noisy pair with 10 % gross outliers, the start
    pose ``pert`` away from the truth, and for calib fy = 0.85 fx and the mask groups of
    ``masked_calib`` -- every error of MUTATIONS changes its sums.  Returns (pair, T float32)."""
    p = TO.make_tracking_pair(hw, seed=seed, mode=mode, noise=noise)
    if mode == "calib":
        p = anisotropic(p, 0.85, noise, seed + 1)
    p = with_outliers(p, 0.1, 0.2, seed + 2)
    T = start_pose(p, pert, seed + 3)
    if mode == "calib":
        p, _ = masked_calib(p, hw, T, cfg["pixel_border"], seed + 4)
    return p, T


def unit_scale(p):
    """A noise-free pair whose generating T_CkCf has scale exactly 1 (returns the pair and that
    pose): a start at scale 1 then takes a first step with sigma ~ 0."""
    T = true_pose(p)
    T[7] = 1.0
    q = dict(p)
    Xf = TO.sim3_act(TO.sim3_inv(T), np.asarray(p["Xk"], np.float64))
    q.update(Xf=Xf.astype(np.float32))
    return q, T
