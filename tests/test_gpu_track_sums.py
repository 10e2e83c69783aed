"""One iteration of the frame tracker on the GPU (track.hip), off the fixed point: the 36 sums of
track_accum_kernel read back from a caller-owned workspace (mast3r_slam_backends.
track_workspace_layout), and the step kernel's chain sum, solve and retraction.

tests/test_gpu_track.py compares converged poses, which only g = 0 decides: a wrong H entry, huber
weight, mask or a dropped point slows the iteration without moving its end.  Here every call runs
max_iters = 1 with the convergence test off and T_WCk = identity, so track_init_kernel's T_CkCf is
bitwise the float32 T_WCf and the float64 reference (tests/track_model.py, sums_f64: the oracle's
solve up to H, g, cost) evaluates at exactly the kernel's pose.

Bound on the sums, with Ho, go, co the float64 sums (track_model.errors, TOL):
    |H_ij - Ho_ij| <= 2e-5 sqrt(Ho_ii Ho_jj),  |g_i - go_i| <= 2e-5 sqrt(Ho_ii 2 co),
    |c - co| <= 2e-5 co
Each normaliser bounds the sum of the absolute values of its entry's terms (Cauchy-Schwarz), so
the kernel's float32 lane, wave and 4-wave sums add about 10 levels x 2^-24 = 6e-7; the float32
restatement of the per-point arithmetic (track_model.sums_f32) reaches 4.1e-6 (H), 1.4e-6 (g),
1.1e-7 (cost) on the host (tests/test_track_model.py), and the smallest deliberate error there is
1.1e-4 (one point of 12288 counted twice; one dropped: 3.0e-4), every other one 0.1 or more.

Bound on the step: the GPU's own sums solved in float64 and retracted with the oracle's sim3_retr
from the float32 start give the GPU's T_CkCf to 2e-6 absolute per component (both sides solve the
same system; what remains is the float32 cast of tau and about 30 float32 operations of retr_sim3
on O(1) values: derived, not fitted).  The returned cost is 0.5 S[35] to 1e-12 relative, and
T_WCf_out is T_CkCf_out bitwise under the identity keyframe pose.

A point with a non-finite Xf poisons the sums even when its ``valid`` is false (0 * NaN), and the
call raises CholeskyError at iteration 1: torch.linalg.cholesky does the same in the reference
tracker, and the float64 sums here are non-finite too.

Measured on an MI355X (worst over the cases of each test; sums as H / g / cost against the bound
2e-5, step against 2e-6):
    test_sums_walk_the_reduction        8.5e-6 / 1.7e-6 / 2.0e-6
        H: rays at 64 and 65 points (7 points: 5.0e-6; from 28672 points on below 6e-7); g and
        cost: calib at 1048876 points, 1.4e-7 / 2.2e-7 without that case.  The float32 restatement
        shows the same on the same inputs: 8.5e-6 (rays, 7 points) / 1.8e-6 / 1.9e-6 (calib,
        1048876 points, where it gives H 3.3e-6 like the kernel's 3.2e-6).
    test_step_walks_the_chain_sum       3.7e-7   (rays 1.6e-7 .. 3.7e-7 from 257 points on, calib
        below 1.1e-7; a float32 restatement of retr_sim3 without FMA scatters the same way on these
        inputs, 2e-8 .. 2.9e-7: the error sits in the translation, from the cancelling
        1 - s cos(theta) in Exp's A and B coefficients)
    test_sums_huber_on_both_branches    4.8e-7 / 1.9e-7 / 4.3e-8, step 7.7e-8
    test_sums_calib_masks               2.4e-7 / 2.2e-7 / 5.8e-8, step 8.6e-8
    test_sums_rays_invalid_points_...   3.4e-6 / 2.0e-7 / 8.2e-8, step 3.0e-8
    test_step_retraction_branches       2.3e-8 (|sigma| = 2e-8), 1.2e-7 (general)
    test_zero_iterations_relative_pose  4.6e-8 against 1e-6
No case came near its bound and no test here found an error in track.hip.
"""
import numpy as np
import pytest
import torch

import track_model as TM
from oracle import track_oracle as TO

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = TO.TRACKING_CFG
CFG1 = dict(CFG, rel_error=0.0, delta_norm=0.0)  # convergence test off
IDENT = np.array([0, 0, 0, 0, 0, 0, 1, 1], np.float32)
STEP_TOL = 2e-6
NOISE = 0.003
# a partial wave; 1 block; 2 blocks with a 1-thread tail; 255 / 256 / 257; 5 blocks (3 padded
# columns); 112 and 113 blocks (chain length 4 and 8); 898 blocks (chain length 36: a second batch
# of loads); the 4096-block cap with a ragged second trip of the grid-stride loop
HWS = [7, 64, 65, 255, 256, 257, 1279, 28672, 28673, 229633, 4096 * 256 + 300]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(be, mode, p, T, hw, cfg, max_iters=1, fill=0, T_WCk=IDENT, check_every=4):
    """track_sim3 on a caller-owned workspace filled with the byte ``fill``.  Returns the 36 sums
    of the written partial columns (float64), those columns (float32), both poses, the iteration
    count and the cost."""
    n = p["Xf"].shape[0]
    kw = {}
    if mode == "calib":
        kw = dict(meas_k=_t(p["meas_k"]), valid_meas_k=_t(p["valid_meas_k"]), K=_t(p["K"]), img_size=hw,
                  pixel_border=cfg["pixel_border"], z_eps=cfg["depth_eps"])
    s0, s1 = TM.sigmas(mode, cfg)
    ws = torch.full((be.lib.m3s_track_workspace_bytes(n),), fill, dtype=torch.uint8, device=DEV)
    Xk = _t(p["Xk"]) if mode == "rays" else None
    Tf, Tr, it, cost = be.track_sim3(mode, _t(p["Xf"]), Xk, _t(np.asarray(T, np.float32)).reshape(1, 8),
                                     _t(np.asarray(T_WCk, np.float32)).reshape(1, 8), _t(p["Qk"]), _t(p["valid"]),
                                     s0, s1, cfg["huber"], max_iters, cfg["rel_error"], cfg["delta_norm"],
                                     check_every=check_every, ws=ws, **kw)
    off, nblk, ld = be.track_workspace_layout(n)
    part = ws[off:].view(torch.float32)[:36 * ld].view(36, ld)[:, :nblk]
    return dict(S=part.double().sum(1).cpu().numpy(), part=part.cpu().numpy(), Tf=Tf.cpu().numpy().reshape(8),
                Tr=Tr.cpu().numpy().reshape(8), it=it, cost=cost)


def _check_sums(tag, r, Ho, go, co):
    assert r["it"] == 1
    e = TM.errors(*TM.unpack36(r["S"]), Ho, go, co)
    print(f"{tag}: sums vs f64 H {e[0]:.2e} g {e[1]:.2e} cost {e[2]:.2e}")
    assert max(e) <= TM.TOL, e


def _check_step(tag, r, T):
    """Chain sum, solve and retraction against the GPU's own sums; returns the float64 tau."""
    H, g, c = TM.unpack36(r["S"])
    tau = np.linalg.solve(H, g)
    Tref = TO.sim3_retr(np.asarray(T, np.float32).astype(np.float64), tau)
    d = float(np.abs(r["Tr"].astype(np.float64) - Tref).max())
    print(f"{tag}: step vs f64 solve of the GPU's sums {d:.2e}, |tau| {np.linalg.norm(tau):.2e}")
    assert d <= STEP_TOL, (d, r["Tr"], Tref)
    assert abs(r["cost"] - c) <= 1e-12 * abs(c), (r["cost"], c)
    assert np.array_equal(r["Tf"], r["Tr"])
    return tau


def _pair(mode, hw, seed):
    p = TO.make_tracking_pair(hw, seed=seed, mode=mode, noise=NOISE)
    return TM.anisotropic(p, 0.85, NOISE, seed + 1) if mode == "calib" else p


def _huber_share(aux):
    act = aux["si"] != 0
    return float((np.abs(aux["wr"][act]) >= CFG["huber"]).mean())


# ----------------------------------------------------------------------------- the reduction walk

_WALK = {}


def _walk(be, mode, HW):
    """Input, float64 sums and the GPU's one iteration at HW points (shared by the tests below)."""
    if (mode, HW) not in _WALK:
        hw = TM.shape_for(HW)
        p = TM.truncate(_pair(mode, hw, 41), HW)
        T = TM.start_pose(p, 0.05, 42)
        Ho, go, co, aux = TM.sums_f64(mode, p, T, CFG1, hw)
        r = _run(be, mode, p, T, hw, CFG1)
        _WALK[mode, HW] = dict(p=p, T=T, hw=hw, ref=(Ho, go, co), share=_huber_share(aux), r=r)
    return _WALK[mode, HW]


@pytest.mark.parametrize("HW", HWS)
@pytest.mark.parametrize("mode", ["rays", "calib"])
def test_sums_walk_the_reduction(backend, mode, HW):
    c = _walk(backend, mode, HW)
    off, nblk, ld = backend.track_workspace_layout(HW)
    assert c["r"]["part"].shape == (36, nblk) and nblk == min((HW + 255) // 256, 4096)
    _check_sums(f"{mode} HW {HW} ({nblk} blocks, huber share {c['share']:.2f})", c["r"], *c["ref"])


@pytest.mark.parametrize("HW", HWS)
@pytest.mark.parametrize("mode", ["rays", "calib"])
def test_step_walks_the_chain_sum(backend, mode, HW):
    """A block the step's chain sum drops or counts twice moves the pose away from the solve of the
    partials' plain sum."""
    c = _walk(backend, mode, HW)
    _check_step(f"{mode} HW {HW}", c["r"], c["T"])


# ----------------------------------------------------------------------------- weights and masks


@pytest.mark.parametrize("pert", [0.02, 0.1])
@pytest.mark.parametrize("mode", ["rays", "calib"])
def test_sums_huber_on_both_branches(backend, mode, pert):
    hw = (96, 128)
    p = _pair(mode, hw, 55)
    T = TM.start_pose(p, pert, 56)
    Ho, go, co, aux = TM.sums_f64(mode, p, T, CFG1, hw)
    share = _huber_share(aux)
    assert 0.2 <= share <= 0.8, share
    r = _run(backend, mode, p, T, hw, CFG1)
    _check_sums(f"{mode} pert {pert} huber share {share:.2f}", r, Ho, go, co)
    _check_step(f"{mode} pert {pert}", r, T)


@pytest.mark.parametrize("border", [-10, 3])
def test_sums_calib_masks(backend, border):
    """Disjoint groups of points behind the camera, outside each of the four borders, without a
    keyframe measurement and invalid: each must drop out of the sums, and nothing else."""
    hw = (37, 53)
    cfg = dict(CFG1, pixel_border=border)
    p0 = _pair("calib", hw, 61)
    T = TM.start_pose(p0, 0.05, 62)
    p, grp = TM.masked_calib(p0, hw, T, border, 63)
    Ho, go, co, aux = TM.sums_f64("calib", p, T, cfg, hw)
    # preconditions, through the reference only: the groups are what they are named, and no
    # comparison is close enough for float32 and float64 to decide it differently
    names = TM.MASK_GROUPS
    assert all((grp == k).sum() > 0 for k in range(len(names)))
    u, v, z = aux["uv"][:, 0], aux["uv"][:, 1], aux["X"][:, 2]
    assert np.all(z[grp == names.index("behind")] < -0.5) and np.all(z[grp != names.index("behind")] > 0.5)
    assert np.all(u[grp == names.index("left")] <= border - 1 + 1e-3)
    assert np.all(u[grp == names.index("right")] >= hw[1] - 1 - border + 1 - 1e-3)
    assert np.all(v[grp == names.index("top")] <= border - 1 + 1e-3)
    assert np.all(v[grp == names.index("bottom")] >= hw[0] - 1 - border + 1 - 1e-3)
    moved = (grp >= 1) & (grp <= 5)
    assert not aux["ok"][moved].any() and not aux["ok"][grp == names.index("no_meas")].any()
    assert aux["ok"][(grp == 0) | (grp == names.index("invalid"))].all()
    assert not np.asarray(p["valid"])[grp == names.index("invalid"), 0].any()
    assert TM.border_distance(aux["uv"], hw, border).min() > 1e-2
    assert np.abs(z).min() > 1e-3
    masked = 1.0 - float((aux["ok"] & np.asarray(p["valid"])[:, 0]).mean())
    assert 0.2 <= masked <= 0.6, masked
    r = _run(backend, "calib", p, T, hw, cfg)
    _check_sums(f"calib masks border {border} masked share {masked:.2f}", r, Ho, go, co)
    _check_step(f"calib masks border {border}", r, T)


def test_sums_rays_invalid_points_and_wide_weights(backend):
    """30 % of the points invalid and Qk from 1e-2 to 1e2."""
    hw = (61, 83)
    rng = np.random.default_rng(71)
    p = dict(_pair("rays", hw, 72))
    n = hw[0] * hw[1]
    p["valid"] = rng.random((n, 1)) > 0.3
    p["Qk"] = (10.0 ** rng.uniform(-2.0, 2.0, (n, 1))).astype(np.float32)
    assert 0.25 < 1.0 - p["valid"].mean() < 0.35 and p["Qk"].min() < 0.02 and p["Qk"].max() > 50.0
    T = TM.start_pose(p, 0.05, 73)
    Ho, go, co, _ = TM.sums_f64("rays", p, T, CFG1, hw)
    r = _run(backend, "rays", p, T, hw, CFG1)
    _check_sums("rays 30 % invalid, wide Qk", r, Ho, go, co)
    _check_step("rays 30 % invalid, wide Qk", r, T)


# ----------------------------------------------------------------------------- the workspace


@pytest.mark.parametrize("HW", [1279, 28673])
@pytest.mark.parametrize("mode", ["rays", "calib"])
def test_workspace_contents_do_not_matter(backend, mode, HW):
    """The padded columns of the partial table are never written: a workspace of 0xFF bytes (NaN
    as float32) must give, bitwise, the sums, cost and poses of a zero-filled one."""
    c = _walk(backend, mode, HW)
    off, nblk, ld = backend.track_workspace_layout(HW)
    assert ld > nblk  # there are padded columns
    a = c["r"]
    b = _run(backend, mode, c["p"], c["T"], c["hw"], CFG1, fill=0xFF)
    assert np.array_equal(a["part"].view(np.int32), b["part"].view(np.int32))
    assert np.isfinite(b["part"]).all()
    assert a["cost"] == b["cost"] and a["it"] == b["it"] == 1
    assert np.array_equal(a["Tr"].view(np.int32), b["Tr"].view(np.int32))
    assert np.array_equal(a["Tf"].view(np.int32), b["Tf"].view(np.int32))


@pytest.mark.parametrize("mode", ["rays", "calib"])
def test_non_finite_point_fails_the_first_cholesky(backend, mode):
    hw = (24, 32)
    p = dict(_pair(mode, hw, 81))
    p["Xf"] = p["Xf"].copy()
    p["valid"] = p["valid"].copy()
    p["Xf"][100] = np.nan
    p["valid"][100] = False
    T = TM.start_pose(p, 0.05, 82)
    Ho, _, _, _ = TM.sums_f64(mode, p, T, CFG1, hw)
    assert not np.isfinite(Ho).all()  # the reference's system is poisoned too
    with pytest.raises(backend.CholeskyError, match="iteration 1"):
        _run(backend, mode, p, T, hw, CFG1)


# ----------------------------------------------------------------------------- the step


@pytest.mark.parametrize("branch", ["small_sigma", "general"])
def test_step_retraction_branches(backend, branch):
    """retr_sim3's translation coefficients: the |sigma| < 1e-6 branch with a finite rotation (a
    noise-free pair of true scale 1, started at scale 1 with a small rotation error), and the
    general one.  The reference says which branch a start takes, with a margin of 2."""
    hw = (48, 64)
    p, T1 = TM.unit_scale(TO.make_tracking_pair(hw, seed=91, mode="rays"))
    if branch == "small_sigma":
        xi = np.array([0, 0, 0, 2e-4, -3e-4, 1e-4, 0], np.float64)
    else:
        xi = 0.05 * np.random.default_rng(92).standard_normal(7)
    T = TO.sim3_retr(T1, xi).astype(np.float32)
    if branch == "small_sigma":
        assert T[7] == np.float32(1.0)
    Ho, go, co, _ = TM.sums_f64("rays", p, T, CFG1, hw)
    tau_o = np.linalg.solve(Ho, go)
    r = _run(backend, "rays", p, T, hw, CFG1)
    tau = _check_step(f"retraction {branch}", r, T)
    for t in (tau_o, tau):
        sigma, theta = abs(t[6]), float(np.linalg.norm(t[3:6]))
        print(f"  sigma {sigma:.2e} theta {theta:.2e}")
        assert theta > 2e-6
        assert sigma < 5e-7 if branch == "small_sigma" else sigma > 2e-6


@pytest.mark.parametrize("mode", ["rays", "calib"])
def test_check_every_does_not_change_the_result(backend, mode):
    """How often the host reads the done flag (every iteration, every 4th, never before
    max_iters) changes neither the poses, the iteration count nor the cost, bitwise."""
    hw = (96, 128)
    p = _pair(mode, hw, 101)
    runs = [_run(backend, mode, p, p["T_WCf"], hw, CFG, max_iters=CFG["max_iters"], T_WCk=p["T_WCk"],
                 check_every=ce) for ce in (1, 4, 50)]
    a = runs[0]
    assert 1 < a["it"] < CFG["max_iters"]  # the convergence test ended it
    for b in runs[1:]:
        assert a["it"] == b["it"] and a["cost"] == b["cost"]
        assert np.array_equal(a["Tf"].view(np.int32), b["Tf"].view(np.int32))
        assert np.array_equal(a["Tr"].view(np.int32), b["Tr"].view(np.int32))


def test_zero_iterations_relative_pose(backend):
    """max_iters = 0 under a keyframe pose that is not the identity: T_CkCf_out is
    inv(T_WCk) T_WCf (track_init_kernel), to 1e-6 absolute of the float64 product."""
    hw = (24, 32)
    p = _pair("rays", hw, 111)
    r = _run(backend, "rays", p, p["T_WCf"], hw, CFG1, max_iters=0, T_WCk=p["T_WCk"])
    Tk, Tf = np.asarray(p["T_WCk"], np.float64), np.asarray(p["T_WCf"], np.float64)
    assert np.abs(Tk - IDENT).max() > 0.05
    Tr = TO.sim3_mul(TO.sim3_inv(Tk), Tf)
    assert r["it"] == 0
    d = float(np.abs(r["Tr"] - Tr).max())
    print(f"max_iters 0: T_CkCf vs f64 {d:.2e}")
    assert d <= 1e-6, d
