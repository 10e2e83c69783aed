"""Head-finish timing probe at the user's size: 384x512, F = 24, tokens layout, downsample 1,
B in {1, 2} (seeded inputs).

Times with device events, after warm-up, over --calls calls each, alternating in one process:
  kernel  mast3r_slam_backends.head_finish into preallocated outputs (one launch),
  torch   the reference's chain on the device on the same tensors: transpose / view / pixel_shuffle
          / cat (catmlp_dpt_head.py:83-87), then m3s.mast3r_utils.postprocess_torch -- the yardstick.
Every call is timed on its own (events around one call, ending in a synchronise: launch included),
and in back-to-back windows of --window calls (the steady-state cost per call).  Calls rotate
through --sets input / output sets so that the bytes between two uses of a set exceed the 256 MiB
Infinity Cache and the reads come from HBM.

The traffic model (traffic_bytes below) is what the algorithm must move: every raw value read once,
every result written once.  Reported: model bytes over the window time per call, and that rate's
share of the 8 TB/s HBM peak (MI355X_MICROARCH.md; about 6.3 TB/s is achievable).  The kernel is
bandwidth-bound: bytes / peak is its floor.  The kernel's own time comes from a separate
`rocprofv3 --kernel-trace --stats -- python tools/head_probe.py --only-kernel` run.
Needs a HIP device: there is no CPU fallback.  Writes --out and prints the result as one line.

usage: python tools/head_probe.py [--out profiles/head_finish.json] [--calls 200]
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

HBM_PEAK = 8.0e12        # bytes/s, spec
HBM_ACHIEVABLE = 6.3e12  # bytes/s, measured streaming ceiling


def traffic_bytes(B, H, W, F, ds=1, desc=True):
    """Bytes the op must move: 4 + (F + 1) f32 read per kept input pixel, 3 + 1 + F + 1 written
    per output pixel.  With ds > 1 the skipped pixels are not read (at dword granularity: the
    memory system still fetches whole lines, so this is the floor, not the fetch)."""
    h, w = -(-H // ds), -(-W // ds)
    per_in = 4 + (F + 1 if desc else 0)
    per_out = 3 + 1 + (F + 1 if desc else 0)
    return {"read": B * h * w * per_in * 4 if ds > 1 else B * H * W * per_in * 4,
            "write": B * h * w * per_out * 4}


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_finish.json"))
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--F", type=int, default=24)
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--window", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--only-kernel", action="store_true", help="head_finish alone (profiling)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("head_probe: needs a HIP device (no CPU fallback)")

    import mast3r_slam_backends as mb
    from m3s.mast3r_utils import postprocess_torch, shuffle_tokens

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(4321)
    H, W, F = args.height, args.width, args.F
    S = (H // 16) * (W // 16)
    result = {"height": H, "width": W, "F": F, "layout": "tokens", "downsample": 1, "sets": args.sets,
              "window": args.window, "device": torch.cuda.get_device_name(0), "library": mb.version(),
              "hbm_peak_Bps": HBM_PEAK, "hbm_achievable_Bps": HBM_ACHIEVABLE, "batches": {}}
    for B in args.batch:
        sets = []
        for _ in range(args.sets):
            pts = torch.randn((B, 4, H, W), generator=g, device=dev)
            feat = torch.randn((B, S, (F + 1) * 256), generator=g, device=dev)
            out = (torch.empty((B, H, W, 3), device=dev), torch.empty((B, H, W), device=dev),
                   torch.empty((B, H, W, F), device=dev), torch.empty((B, H, W), device=dev))
            sets.append((pts, feat, out))
        n = len(sets)

        def kernel(k):
            pts, feat, out = sets[k % n]
            return mb.head_finish(pts, feat, out=out)

        def chain(k):
            pts, feat, _ = sets[k % n]
            return postprocess_torch(torch.cat([pts, shuffle_tokens(feat, H, W)], dim=1), F)

        tb = traffic_bytes(B, H, W, F)
        nbytes = tb["read"] + tb["write"]
        t = {"kernel_call": [], "torch_call": [], "kernel_window": [], "torch_window": []}
        k = 0
        for it in range(args.warmup + args.calls):
            ms_k = timed(lambda j: kernel(k + j))
            if args.only_kernel:
                k += 1
                continue
            ms_t = timed(lambda j: chain(k + j))
            k += 1
            if it >= args.warmup:
                t["kernel_call"].append(ms_k)
                t["torch_call"].append(ms_t)
        if args.only_kernel:
            continue
        for it in range(max(args.calls // args.window, 5)):
            t["kernel_window"].append(timed(lambda j: kernel(k + j), args.window))
            t["torch_window"].append(timed(lambda j: chain(k + j), args.window))
            k += args.window
        # the two paths agree (the tests hold the kernel to the model; this is a sanity line)
        ref = chain(0)
        got = kernel(0)
        err = [float(((a - b).abs() / b.abs().clamp_min(1e-30)).max()) for a, b in zip(got, ref)]
        r = {name: stats(v) for name, v in t.items()}
        r["traffic_model_bytes"] = dict(tb, total=nbytes)
        sec = r["kernel_window"]["median_ms"] * 1e-3
        r["kernel_model_Bps"] = nbytes / sec
        r["kernel_share_of_hbm_peak"] = nbytes / sec / HBM_PEAK
        r["kernel_share_of_hbm_achievable"] = nbytes / sec / HBM_ACHIEVABLE
        r["floor_ms_at_hbm_peak"] = nbytes / HBM_PEAK * 1e3
        r["torch_over_kernel_window"] = r["torch_window"]["median_ms"] / r["kernel_window"]["median_ms"]
        r["torch_over_kernel_call"] = r["torch_call"]["median_ms"] / r["kernel_call"]["median_ms"]
        r["max_rel_diff_kernel_vs_torch_XCDQ"] = err
        result["batches"][str(B)] = r
        del sets
        torch.cuda.empty_cache()
    if not args.only_kernel:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
