"""Map-export measurement (DESIGN.md "Map export"): kernel time and implied traffic of
m3s_recon_count / m3s_recon_emit, and the reference-shaped host path on the same data.

    python profiles/recon_traffic.py [--keyframes 128] [--height 384] [--width 512] [--out FILE]

Needs a HIP device.  Kernel times are HIP events around the call on the current stream, the
median of --runs runs after --warmup warm-ups.  GB/s are against the algorithmic bytes: 16 B read
per point in count (X and C of every candidate, the figure the streaming bound is stated in; the
kernel itself reads only C, 4 B) and 31 B read + 15 B written per kept point in emit.  The host
path restates evaluate.py:47-106 of the reference: per keyframe the transform on the device, a
.cpu().numpy() of the points, the confidences and the image, a boolean gather, then one
concatenate and the interleave into the vertex array save_ply hands to plyfile.
Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mast3r-slam_amd")]


def act(T, p):
    t, q, s = T[0:3], T[3:7], T[7]
    u, w = q[:3].expand_as(p), q[3]
    uv = 2.0 * torch.cross(u, p, dim=-1)
    return s * (p + w * uv + torch.cross(u, uv, dim=-1)) + t


def host_path(X, C, n_obs, T, uimg_host, thresh, dtype):
    pts, cols = [], []
    for k in range(X.shape[0]):
        pW = act(T[k], X[k]).cpu().numpy().reshape(-1, 3)
        color = (uimg_host[k].numpy() * 255).astype(np.uint8).reshape(-1, 3)
        valid = (C[k] / n_obs[k]).cpu().numpy().astype(np.float32).reshape(-1) > thresh
        pts.append(pW[valid])
        cols.append(color[valid])
    pts = np.concatenate(pts, axis=0)
    cols = np.concatenate(cols, axis=0)
    pcd = np.empty(len(pts), dtype=dtype)
    pcd["x"], pcd["y"], pcd["z"] = pts.T
    pcd["red"], pcd["green"], pcd["blue"] = cols.T
    return pcd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=128)
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("recon_traffic: needs a HIP device")
    import mast3r_slam_backends as mb

    dev = torch.device("cuda", 0)
    N, HW = a.keyframes, a.height * a.width
    g = torch.Generator().manual_seed(0)
    X = torch.randn((N, HW, 3), generator=g).to(dev)
    n_obs = (1.0 + torch.arange(N) % 3).float().to(dev)
    # C / n_obs uniform in [1, 2): thresh 1.5 keeps about half the points
    C = ((1.0 + torch.rand((N, HW, 1), generator=g)).to(dev) * n_obs.reshape(N, 1, 1)).contiguous()
    q = torch.randn((N, 4), generator=g)
    T = torch.cat([torch.randn((N, 3), generator=g) * 0.3, q / q.norm(dim=1, keepdim=True),
                   torch.full((N, 1), 1.1)], dim=1).to(dev)
    uimg_host = torch.rand((N, a.height, a.width, 3), generator=g)
    rgb = (uimg_host * 255).to(torch.uint8).reshape(N, HW, 3).to(dev)
    thresh = 1.5

    p = mb.ReconPass(X, C, n_obs, T, rgb=rgb, thresh=thresh)
    counts, total = p.count()
    kept = int(total.item())
    body = torch.empty((15 * kept,), dtype=torch.uint8, device=dev)

    def timed(fn):
        ms = []
        for i in range(a.warmup + a.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), min(ms), max(ms)

    count_ms = timed(p.count)
    emit_ms = timed(lambda: p.emit(body, kept))

    def device_path():
        b, _ = mb.reconstruct(X, C, n_obs, T, rgb=rgb, thresh=thresh)
        return b.cpu().numpy()

    def wall(fn, runs):
        ts = []
        out = None
        for _ in range(runs + 1):  # the first run warms up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts[1:]), out

    dev_ms, dev_body = wall(device_path, a.host_runs)
    host_ms, host_pcd = wall(lambda: host_path(X, C, n_obs, T, uimg_host, thresh, mb.RECON_DTYPE),
                             a.host_runs)
    dev_pcd = dev_body.view(mb.RECON_DTYPE)
    same_set = len(dev_pcd) == len(host_pcd) and bool(
        np.array_equal(dev_pcd["red"], host_pcd["red"]) and np.array_equal(dev_pcd["blue"], host_pcd["blue"]))
    max_diff = float(max(np.abs(dev_pcd[f] - host_pcd[f]).max() for f in "xyz")) if same_set and kept else None

    points = N * HW
    res = {
        "keyframes": N, "height": a.height, "width": a.width, "points": points, "kept": kept,
        "tile_points": mb.recon_tile_points(), "runs": a.runs, "warmup": a.warmup,
        "count_ms_median_min_max": count_ms, "emit_ms_median_min_max": emit_ms,
        "count_GBps_16B_per_point": 16.0 * points / (count_ms[0] * 1e-3) / 1e9,
        "count_GBps_actual_4B_per_point": 4.0 * points / (count_ms[0] * 1e-3) / 1e9,
        "emit_GBps_46B_per_kept": 46.0 * kept / (emit_ms[0] * 1e-3) / 1e9,
        "emit_GBps_actual": (4.0 * points + 30.0 * kept) / (emit_ms[0] * 1e-3) / 1e9,
        "device_path_ms_count_emit_d2h": dev_ms, "host_path_ms": host_ms,
        "host_over_device": host_ms / dev_ms,
        "same_selection_and_colours_as_host_path": same_set, "max_abs_xyz_diff_vs_host_path": max_diff,
        "device": torch.cuda.get_device_name(0),
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
