"""Record the packed accumulate's results (dx, Twc) on a set of small graphs, bit for bit.

Run on a machine with a HIP device, from the root of a BUILT tree of the commit whose results are
to be pinned (the parent of the change under test):

    python tests/golden/make_accum_trim_golden.py [out.npz]

Writes tests/golden/accum_trim_golden.npz (a few KB: per call the poses and the last update, plus
a digest of the call's inputs).  tests/test_gpu_accum_trim.py imports this file for the graphs
and the calls and requires `array_equal` with the recording: the kernel's sums have a fixed order,
so a change that keeps every floating-point operation, its operands and its order reproduces them.

Two families of graphs (m3s.synth.make_graph, the GN tests' helper):

* SMALL -- 6 keyframes, 10 directed edges, every image size of the list below.  With so few edges
  the planner cuts every image into workgroup chunks of at most 1024 points (it wants ~4096 tasks
  per launch, gn_plan.hip: choose_nchunks), so a workgroup runs ONE step of its loop, full or
  partial, whatever the image size.
* DEEP -- 65 keyframes and 4096 directed edges on the same image sizes: the planner's task target
  is met by the edges alone, a chunk is the whole image, and the step loop runs 3 steps (2 full and
  a partial one: 36x64, 40x52), exactly 3 (48x64) and exactly 4 (64x64) at 4 points per lane, and 5
  (4 full and a partial one: 36x64) at the 2 points per lane of the rays and points modes.  Width
  64 divides the 1024 points of a step (a lane keeps its columns from step to step), width 52 does
  not.

Every graph has unmatched points, one Q below the threshold and (calib) matches that project
outside the image.  Calls: 3 iterations (the first accumulate builds the packed records, the later
ones read them), and 1 iteration with M3S_GN_PACK=2 (the packed stream forced).
"""
from __future__ import annotations

import contextlib
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, "mast3r-slam_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

GOLDEN = os.path.join(HERE, "accum_trim_golden.npz")

LOCAL = dict(sigma_ray=0.003, sigma_dist=10.0, sigma_pixel=1.0, sigma_depth=10.0, sigma_point=0.05,
             C_conf=0.0, Q_conf=1.5, pixel_border=-10, depth_eps=1e-6)

# (name, N keyframes, E undirected edges, H, W, seed)
SMALL_SIZES = [(24, 32), (36, 64), (48, 64), (64, 64), (40, 52)]
DEEP_SIZES = [(36, 64), (48, 64), (64, 64), (40, 52)]
GRAPHS = ([(f"small{h}x{w}", 6, 5, h, w, 11) for h, w in SMALL_SIZES] +
          [(f"deep{h}x{w}", 65, 2048, h, w, 12) for h, w in DEEP_SIZES])
# modes run on a graph: calib = ray-constrained points (the depth-only stream), calib_pos = the
# same points moved off their rays (the positional stream)
MODES = {name: ["calib"] for name, *_ in GRAPHS}
MODES["small36x64"] = ["calib", "calib_pos", "rays", "points"]
MODES["deep36x64"] = ["calib", "calib_pos", "rays", "points"]
# (tag, iterations, environment)
CALLS = [("it3", 3, {}), ("pack2_it1", 1, {"M3S_GN_PACK": "2"})]


def make_graph(spec):
    from m3s import synth

    name, N, E, H, W, seed = spec
    g = synth.make_graph(dict(N=N, E=E), H=H, W=W, seed=seed)
    HW = H * W
    g.valid[1, 10:90] = False                 # a run of unmatched points
    g.valid[3, HW - 5:] = False               # ... and the last points of an edge
    g.valid[g.E_directed - 1, ::97] = False   # ... and scattered ones
    g.Q[0, 37] = 1.0                          # one Q below Q_conf
    return g


def mode_inputs(g, mode):
    """(op mode, Xs) of a graph for one of MODES."""
    from m3s.geometry import constrain_points_to_ray

    if mode == "calib":
        return "calib", constrain_points_to_ray((g.H, g.W), g.Xs, g.K).contiguous()
    if mode == "calib_pos":
        return "calib", (constrain_points_to_ray((g.H, g.W), g.Xs, g.K) * 1.0001).contiguous()
    return mode, g.Xs


def digest(g, Xs):
    h = hashlib.sha256()
    for t in (g.Twc, Xs, g.Cs, g.K, g.ii, g.jj, g.idx, g.valid.to(torch.uint8), g.Q):
        h.update(t.contiguous().numpy().tobytes())
    return np.frombuffer(h.digest()[:8], dtype=np.uint8).copy()


@contextlib.contextmanager
def environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run_graph(backend, g, modes):
    """{key: array} of every mode and call on one graph (inputs uploaded once per mode)."""
    L = LOCAL
    out = {}
    dev = torch.device("cuda", 0)
    ii, jj, idx, valid, Q, Cs, K = (t.to(dev) for t in (g.ii, g.jj, g.idx, g.valid, g.Q, g.Cs, g.K))
    for mode in modes:
        op, Xs_h = mode_inputs(g, mode)
        Xs = Xs_h.to(dev)
        out[f"{mode}/inputs"] = digest(g, Xs_h)
        for tag, iters, env in CALLS:
            Twc = g.Twc.clone().to(dev)
            with environment(env):
                if op == "calib":
                    (dx,) = backend.gauss_newton_calib(Twc, Xs, Cs, K, ii, jj, idx, valid, Q, g.H, g.W,
                                                       L["pixel_border"], L["depth_eps"], L["sigma_pixel"],
                                                       L["sigma_depth"], L["C_conf"], L["Q_conf"], iters, 0.0)
                elif op == "rays":
                    (dx,) = backend.gauss_newton_rays(Twc, Xs, Cs, ii, jj, idx, valid, Q, L["sigma_ray"],
                                                      L["sigma_dist"], L["C_conf"], L["Q_conf"], iters, 0.0)
                else:
                    (dx,) = backend.gauss_newton_points(Twc, Xs, Cs, ii, jj, idx, valid, Q, L["sigma_point"],
                                                        L["C_conf"], L["Q_conf"], iters, 0.0)
                torch.cuda.synchronize()
            out[f"{mode}/{tag}/Twc"] = Twc.cpu().numpy()
            out[f"{mode}/{tag}/dx"] = dx.cpu().numpy()
    return out


def main():
    import time

    import mast3r_slam_backends as mb

    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    out = {}
    for spec in GRAPHS:
        t0 = time.time()
        g = make_graph(spec)
        t1 = time.time()
        for k, v in run_graph(mb, g, MODES[spec[0]]).items():
            out[f"{spec[0]}/{k}"] = v
        print(f"{spec[0]}: graph {t1 - t0:.2f} s, calls {time.time() - t1:.2f} s", flush=True)
    bad = [k for k, v in out.items() if v.dtype != np.uint8 and not np.isfinite(v).all()]
    assert not bad, f"non-finite results: {bad}"
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
