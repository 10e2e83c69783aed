"""Retrieval timing probe at the user's size: n = 300 local features, D = 1024, K = 65,536
centroids, a database of 128 and of 1,024 images (seeded inputs).

Times with device events, after warm-up, over --calls calls each, alternating in one process:
  update   RetrievalDatabase.update(add_after_query=False) end to end (its device-to-host copy of
           the scores and the host topk included),
  quantize the fused MFMA quantise stage alone (mast3r_slam_backends.retrieval_quantize, ma = 5),
  torch    the reference's formulation of that stage in torch-ROCm on the same tensors
           (retrieval_database.py:96-105: norms, @, topk) -- the yardstick.
Reports medians and spread, quantise's achieved f32 FLOP/s (2 n D K per call, over the stage's
event time: launches included, so a lower bound of the kernel's own rate) as a share of the
157.3 TF f32-matrix peak, and the ids' agreement with the torch path.  Needs a HIP device: there
is no CPU fallback.  Writes <out>/retrieval_probe.json and prints it as one line.

usage: python tools/retrieval_probe.py [--out profiles/retrieval] [--calls 200]
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

PEAK_F32_MATRIX = 157.3e12


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(a)), "p10_ms": float(a[int(0.1 * (len(a) - 1))]),
            "p90_ms": float(a[int(0.9 * (len(a) - 1))]), "min_ms": float(a[0]), "calls": int(len(a))}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retrieval"))
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--D", type=int, default=1024)
    ap.add_argument("--K", type=int, default=65536)
    ap.add_argument("--images", type=int, nargs="+", default=[128, 1024])
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--only-quantize", action="store_true", help="the quantise stage alone (profiling)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("retrieval_probe: needs a HIP device (no CPU fallback)")

    import mast3r_slam_backends as mb
    from m3s.retrieval_database import ASMK_PARAMS, RetrievalDatabase

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1234)
    n, D, K = args.n, args.D, args.K
    cent = torch.randn((K, D), generator=g, device=dev)
    pool = torch.randint(0, K, (4096,), generator=g, device=dev)

    def image():
        w = pool[torch.randint(0, pool.numel(), (n,), generator=g, device=dev)]
        return (cent[w] + 0.6 * torch.randn((n, D), generator=g, device=dev)).contiguous()

    def torch_quantize(q):
        l2 = torch.sum(q ** 2, dim=1)[:, None] + torch.sum(cent ** 2, dim=1)[None, :] - 2 * (q @ cent.mT)
        return torch.topk(l2, 5, dim=1, largest=False).indices

    rd = RetrievalDatabase(cent, device=dev, max_feat=n)
    result = {"n": n, "D": D, "K": K, "device": torch.cuda.get_device_name(0), "library": mb.version(),
              "flop_per_quantize": 2.0 * n * D * K, "databases": {}}
    queries = [image() for _ in range(8)]
    for size in sorted(args.images):
        while len(rd) < size:
            rd.add_to_database(image())
        torch.cuda.synchronize()
        t = {"update": [], "quantize": [], "torch": []}
        same_rows = same_sets = rows = 0
        for it in range(args.warmup + args.calls):
            q = queries[it % len(queries)]
            ms_q, ids = timed(lambda: mb.retrieval_quantize(rd._db, q, 5))
            if args.only_quantize:
                continue
            ms_u, _ = timed(lambda: rd.update(q, False, 3, 5e-3))
            ms_t, ids_t = timed(lambda: torch_quantize(q))
            if it >= args.warmup:
                t["update"].append(ms_u)
                t["quantize"].append(ms_q)
                t["torch"].append(ms_t)
            if it < len(queries):
                a, b = ids.long().cpu().numpy(), ids_t.cpu().numpy()
                same_rows += int((a == b).all(axis=1).sum())
                same_sets += int((np.sort(a, axis=1) == np.sort(b, axis=1)).all(axis=1).sum())
                rows += n
        if args.only_quantize:
            continue
        r = {k: stats(v) for k, v in t.items()}
        med = r["quantize"]["median_ms"] * 1e-3
        r["quantize"]["achieved_f32_flops"] = result["flop_per_quantize"] / med
        r["quantize"]["share_of_f32_matrix_peak"] = result["flop_per_quantize"] / med / PEAK_F32_MATRIX
        r["torch"]["achieved_f32_flops"] = result["flop_per_quantize"] / (r["torch"]["median_ms"] * 1e-3)
        r["quantize_over_torch_median"] = r["quantize"]["median_ms"] / r["torch"]["median_ms"]
        r["ids_rows_equal_to_torch"] = same_rows / rows
        r["ids_sets_equal_to_torch"] = same_sets / rows
        result["databases"][str(size)] = r
    result["params"] = ASMK_PARAMS["query_ivf"]["similarity"]
    if not args.only_quantize:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "retrieval_probe.json"), "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
