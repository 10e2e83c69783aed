"""Generate the map-export golden fixtures from the REFERENCE Python (dev container only).

Run from the repo root:  python tests/golden/make_recon_golden.py
Writes tests/golden/recon_golden.npz (inputs + reference outputs, small shapes).

Pinned (reference file:line): save_reconstruction (evaluate.py:47-70) run as written, on a list of
the reference's own Frame objects (frame.py:17-108: get_average_conf), with
constrain_points_to_ray / backproject / get_pixel_coords (geometry.py:37-42, 107-123) in the
use_calib case, in float32 torch on CPU.  The (points, colors) it hands to save_ply are captured;
plyfile is absent, so the file writer itself (evaluate.py:88-106) is not run.  lietorch is absent:
T_WC.act goes through oracle.track_oracle's Sim3T, a restatement of lietorch's Sim3 group, so the
group action itself stays unpinned (see oracle/track_oracle.py).  cv2, natsort, pyrealsense2 and
mast3r_slam.mast3r_utils are import-time dependencies of the reference modules only and are
stubbed empty.

Two cases (uncalibrated, use_calib), each N = 3 keyframes of 12x16: keyframe 0 mixed (C summed
over 2 observations), keyframe 1 with no point above the threshold, keyframe 2 with every point
above it.  Inputs at the magnitudes of tests/test_gpu_keyframe.py (_inputs, _T).

The reference is read from /root/reference at generation time only; nothing under tests/
imports it at run time, and no reference source is copied.
"""
from __future__ import annotations

import os
import sys
import tempfile
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mast3r-slam_amd")]

from oracle import track_oracle as TO  # noqa: E402

H, W, N, THRESH = 12, 16, 3, 1.5


def install_stubs():
    lt = types.ModuleType("lietorch")
    lt.Sim3 = TO._torch_sim3()
    sys.modules["lietorch"] = lt
    mu = types.ModuleType("mast3r_slam.mast3r_utils")
    mu.mast3r_match_asymmetric = None
    mu.mast3r_match_symmetric = None
    mu.resize_img = None
    sys.modules["mast3r_slam.mast3r_utils"] = mu
    for name in ("cv2", "pyrealsense2"):
        sys.modules[name] = types.ModuleType(name)
    ns = types.ModuleType("natsort")
    ns.natsorted = sorted
    sys.modules["natsort"] = ns
    pf = types.ModuleType("plyfile")
    pf.PlyData = pf.PlyElement = None
    sys.modules["plyfile"] = pf
    sys.path.insert(0, REF)
    return lt.Sim3


def make_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    HW = H * W
    X = torch.randn((N, HW, 3), generator=g)
    n_obs = torch.tensor([2.0, 1.0, 3.0])
    C = torch.empty((N, HW, 1))
    C[0] = (1.0 + torch.rand((HW, 1), generator=g) * 5) * 0.5 * n_obs[0]  # C / N in [0.5, 3)
    C[1] = torch.rand((HW, 1), generator=g) * THRESH * 0.99               # none above
    C[2] = (THRESH * 1.01 + torch.rand((HW, 1), generator=g) * 5) * n_obs[2]  # all above
    T = torch.empty((N, 8))
    for k in range(N):
        q = torch.randn(4, generator=g)
        T[k] = torch.cat([torch.randn(3, generator=g) * 0.3, q / q.norm(),
                          torch.tensor([1.1 - 0.15 * k])])
    uimg = torch.rand((N, H, W, 3), generator=g)
    uimg[0, 0, 0] = torch.tensor([0.0, 1.0, 0.5])
    K = torch.tensor([[18.5, 0.0, 7.7], [0.0, 19.25, 5.6], [0.0, 0.0, 1.0]])
    return X, C, n_obs, T, uimg, K


def main():
    Sim3 = install_stubs()
    from mast3r_slam import config as rcfg
    from mast3r_slam import evaluate as rev
    from mast3r_slam import frame as rfr

    rcfg.load_config(os.path.join(REF, "config", "base.yaml"))
    captured = []
    rev.save_ply = lambda filename, points, colors: captured.append((points, colors))
    out = {}
    for case, (calib, seed) in enumerate(((False, 11), (True, 12))):
        X, C, n_obs, T, uimg, K = make_inputs(seed)
        rcfg.config["use_calib"] = calib
        frames = []
        for k in range(N):
            f = rfr.Frame(k, torch.zeros((1, 3, H, W)), torch.tensor([[H, W]]), torch.tensor([[H, W]]),
                          uimg[k].clone(), Sim3(T[k].reshape(1, 8).clone()))
            f.X_canon, f.C, f.N, f.K = X[k].clone(), C[k].clone(), int(n_obs[k]), K.clone()
            frames.append(f)
        del captured[:]
        rev.save_reconstruction(tempfile.mkdtemp(), "unused.ply", frames, THRESH)
        (points, colors), = captured
        out[f"c{case}_calib"] = np.array(calib)
        out[f"c{case}_X"] = X.numpy()
        out[f"c{case}_C"] = C.numpy()
        out[f"c{case}_n_obs"] = n_obs.numpy()
        out[f"c{case}_T_WC"] = T.numpy()
        out[f"c{case}_uimg"] = uimg.numpy()
        out[f"c{case}_K"] = K.numpy()
        out[f"c{case}_out_points"] = np.asarray(points, np.float32)
        out[f"c{case}_out_colors"] = np.asarray(colors, np.uint8)
        print(f"case {case}: calib={calib} kept {len(points)} of {N * H * W}")
    out["ncases"] = np.array(2)
    out["thresh"] = np.array(THRESH, np.float32)
    out["img_size"] = np.array([H, W])
    np.savez_compressed(os.path.join(HERE, "recon_golden.npz"), **out)
    print("wrote", os.path.join(HERE, "recon_golden.npz"), len(out), "arrays")


if __name__ == "__main__":
    main()
