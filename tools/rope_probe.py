"""RoPE2D timing probe at the SLAM shapes: N = 768 tokens (512x384 at patch 16), (H, D) = (16, 64)
(encoder) and (12, 64) (decoder), B in {1, 2}, f32, q and k as the thirds of a [B,N,3,H,D] qkv
buffer (seeded inputs, PositionGetter-style grid positions).

Times with device events, after warm-up, alternating in one process, what one attention spends on
rotating q and k:
  torch   m3s.rope.rope2d_torch on q and on k (the torch expressions, out of place) -- the yardstick,
  two     two mast3r_slam_backends.rope_2d calls (two launches, in place),
  pair    one mast3r_slam_backends.rope_2d_pair call (one launch, in place).
Every variant is timed call by call (events around one q+k rotation, ending in a synchronise:
launch included) and in back-to-back windows of --window rotations (the steady-state cost).  Calls
rotate through --sets buffers; a buffer is a few MB, so like the real network's qkv (just written
by the projection GEMM) it is read from cache, not HBM: the pass is launch- and latency-bound, and
the byte count (2 B N H D sizeof for one tensor, read + write) over the time is reported as a
rate, not as a share of a bandwidth peak.
Needs a HIP device: there is no CPU fallback.  Writes --out and prints the result as one line.

usage: python tools/rope_probe.py [--out profiles/rope2d.json] [--calls 200]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mast3r-slam_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

BASE = 100.0


def traffic_bytes(B, N, H, D, itemsize=4):
    """Bytes one q+k rotation must move: every value of q and k read once and written once."""
    return 2 * (2 * B * N * H * D * itemsize)


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(a)), "p10_ms": float(a[int(0.1 * (len(a) - 1))]),
            "p90_ms": float(a[int(0.9 * (len(a) - 1))]), "min_ms": float(a[0]), "calls": int(len(a))}


def timed(fn, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(reps):
        fn(k)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rope2d.json"))
    ap.add_argument("--grid", type=int, nargs=2, default=[24, 32], help="patch grid (rows, columns)")
    ap.add_argument("--heads", type=int, nargs="+", default=[16, 12])
    ap.add_argument("--D", type=int, default=64)
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--window", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sets", type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rope_probe: needs a HIP device (no CPU fallback)")

    import mast3r_slam_backends as mb
    from m3s.rope import rope2d_torch

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1234)
    gh, gw = args.grid
    N, D = gh * gw, args.D
    result = {"grid": [gh, gw], "N": N, "D": D, "dtype": "float32", "layout": "qkv slices",
              "sets": args.sets, "window": args.window, "device": torch.cuda.get_device_name(0),
              "library": mb.version(), "shapes": {}}
    for B in args.batch:
        pos = torch.cartesian_prod(torch.arange(gh), torch.arange(gw)).view(1, N, 2).expand(B, -1, 2)
        pos = pos.contiguous().to(dev)
        for H in args.heads:
            sets = [torch.randn((B, N, 3, H, D), generator=g, device=dev) for _ in range(args.sets)]
            n = len(sets)

            def chain(k):
                qkv = sets[k % n]
                return rope2d_torch(qkv[:, :, 0], pos, BASE), rope2d_torch(qkv[:, :, 1], pos, BASE)

            def two(k):
                qkv = sets[k % n]
                mb.rope_2d(qkv[:, :, 0], pos, BASE, 1.0)
                mb.rope_2d(qkv[:, :, 1], pos, BASE, 1.0)

            def pair(k):
                qkv = sets[k % n]
                mb.rope_2d_pair(qkv[:, :, 0], qkv[:, :, 1], pos, pos, BASE, 1.0)

            variants = (("torch", chain), ("two", two), ("pair", pair))
            # the paths agree (the tests hold the kernel to the model; this is a sanity line)
            want = chain(0)
            check = sets[0].clone()
            mb.rope_2d_pair(check[:, :, 0], check[:, :, 1], pos, pos, BASE, 1.0)
            err = max(float((check[:, :, i] - want[i]).abs().max()) for i in range(2))

            t = {f"{name}_{kind}": [] for name, _ in variants for kind in ("call", "window")}
            k = 0
            for it in range(args.warmup + args.calls):
                for name, fn in variants:
                    ms = timed(lambda j: fn(k + j))
                    if it >= args.warmup:
                        t[f"{name}_call"].append(ms)
                k += 1
            for it in range(max(args.calls // args.window, 5)):
                for name, fn in variants:
                    t[f"{name}_window"].append(timed(lambda j: fn(k + j), args.window))
                k += args.window
            r = {name: stats(v) for name, v in t.items()}
            nbytes = traffic_bytes(B, N, H, D)
            r["traffic_model_bytes"] = nbytes
            r["pair_model_Bps"] = nbytes / (r["pair_window"]["median_ms"] * 1e-3)
            for kind in ("call", "window"):
                r[f"torch_over_pair_{kind}"] = r[f"torch_{kind}"]["median_ms"] / r[f"pair_{kind}"]["median_ms"]
                r[f"two_over_pair_{kind}"] = r[f"two_{kind}"]["median_ms"] / r[f"pair_{kind}"]["median_ms"]
            r["max_abs_diff_pair_vs_torch"] = err
            result["shapes"][f"B{B}_H{H}"] = r
            del sets
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
