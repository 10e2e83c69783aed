"""Generate the Frame.update_pointmap golden fixture from the REFERENCE Python (dev container only).

Run from the repo root:  python tests/golden/make_keyframe_golden.py
Writes tests/golden/keyframe_golden.npz; a rerun reproduces the file byte for byte (the archive
members carry a fixed date).

Pinned (reference file:line): Frame.update_pointmap and get_average_conf
(mast3r_slam/frame.py:33-108) run as written on the CPU, one sequence of 4 calls at HW = 300 per
filtering mode (first, recent, best_score with the median and with the mean score, indep_conf,
weighted_pointmap, weighted_spherical).  Every call's inputs are stored and, after every call,
X_canon, C, N, N_updates, get_average_conf() and (best_score) the score, each as one array with
the calls along axis 0.  lietorch is the torch stand-in of oracle/track_oracle.py (frame.py needs
Sim3.Identity at import); mast3r_utils and the backend are empty stubs (unused on this path).

For weighted_spherical the file also holds, per call, the largest deviation of the reference's
f32 result from a float64 evaluation of the same formula chained over the calls (``sph_dev``):
the unit of the tolerance the device test gives the torch expression.

The reference is read from /root/reference at generation time only; nothing under tests/
imports it at run time, and no reference source is copied.
"""
from __future__ import annotations

import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
HW = 300
NCALLS = 4
# (sequence name, filtering_mode, filtering_score)
SEQS = [("first", "first", "median"), ("recent", "recent", "median"),
        ("best_median", "best_score", "median"), ("best_mean", "best_score", "mean"),
        ("indep_conf", "indep_conf", "median"), ("weighted_pointmap", "weighted_pointmap", "median"),
        ("weighted_spherical", "weighted_spherical", "median")]
# per-call confidence scales of the best_score sequences: call 1 and 3 replace, call 2 does not
BEST_SCALE = [1.0, 1.5, 0.7, 2.2]


def sph_fuse64(X, C, Xn, Cn):
    """frame.py:78-102 in float64 (numpy)."""
    def to_sph(P):
        r = np.sqrt((P * P).sum(axis=-1, keepdims=True))
        return np.concatenate((r, np.arctan2(P[:, 1:2], P[:, 0:1]), np.arccos(P[:, 2:3] / r)), axis=-1)

    s = ((C * to_sph(X)) + (Cn * to_sph(Xn))) / (C + Cn)
    r, phi, theta = s[:, 0:1], s[:, 1:2], s[:, 2:3]
    return np.concatenate((r * np.sin(theta) * np.cos(phi), r * np.sin(theta) * np.sin(phi),
                           r * np.cos(theta)), axis=-1), C + Cn


def inputs(name, c, frame, g):
    """Call c's (X, C) of sequence `name`; `frame` is the reference Frame before the call."""
    if name == "weighted_spherical":
        X = 0.2 + 1.8 * torch.rand((HW, 3), generator=g)  # off the atan2 cut, |z/r| < 0.99
    else:
        X = torch.randn((HW, 3), generator=g) * 2.0
    C = 1.0 + 5.0 * torch.rand((HW, 1), generator=g)
    if name.startswith("best_"):
        C = C * BEST_SCALE[c]
    if not name.startswith("weighted_"):
        # these modes only compare and copy: values on a 1/32 grid lose nothing as a check and
        # keep the file small (the weighted modes' arithmetic gets full-mantissa inputs)
        X, C = torch.round(X * 32) / 32, torch.round(C * 32) / 32
    if name == "indep_conf" and c > 0:
        # a third of the rows tie the keyframe's confidence exactly, a third exceed it, a third
        # fall short of it
        k = torch.arange(HW)[:, None] % 3
        C = torch.where(k == 0, frame.C, torch.where(k == 1, frame.C * 1.25, frame.C * 0.75))
    return X, C


def write_npz(path, out):
    """np.savez_compressed with a fixed member date, so that a rerun gives the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(out[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from oracle.track_oracle import _torch_sim3

    lt = types.ModuleType("lietorch")
    lt.Sim3 = _torch_sim3()
    sys.modules["lietorch"] = lt
    sys.modules["mast3r_slam.mast3r_utils"] = types.ModuleType("mast3r_slam.mast3r_utils")
    sys.modules["mast3r_slam.mast3r_utils"].resize_img = None
    sys.modules["mast3r_slam_backends"] = types.ModuleType("mast3r_slam_backends")
    sys.path.insert(0, REF)
    from mast3r_slam import config as rcfg
    from mast3r_slam import frame as rframe

    rcfg.load_config(os.path.join(REF, "config", "base.yaml"))

    out = {"HW": np.array(HW), "ncalls": np.array(NCALLS), "names": np.array([s[0] for s in SEQS]),
           "modes": np.array([s[1] for s in SEQS]), "scores": np.array([s[2] for s in SEQS])}
    for si, (name, mode, score) in enumerate(SEQS):
        rcfg.config["tracking"]["filtering_mode"] = mode
        rcfg.config["tracking"]["filtering_score"] = score
        g = torch.Generator().manual_seed(100 + si)
        f = rframe.Frame(0, None, None, None, None)
        replaced = []
        seq = {}
        X64 = C64 = None
        dev = []
        for c in range(NCALLS):
            X, C = inputs(name, c, f, g)
            if name == "indep_conf" and c > 0:
                assert (C == f.C).sum() >= HW // 4 and (C > f.C).sum() >= HW // 4 \
                    and (C < f.C).sum() >= HW // 4
            if mode == "best_score" and c > 0:
                new, old = float(f.get_score(C)), float(f.score)
                assert abs(new - old) >= 0.01 * max(abs(new), abs(old)), (name, c, new, old)
                replaced.append(new > old)
            if name == "weighted_spherical":
                assert float(X.min()) >= 0.2 and float(X.max()) <= 2.0
                assert float((X[:, 2] / X.norm(dim=-1)).abs().max()) < 0.99
            f.update_pointmap(X, C)
            rec = {"X": X, "C": C, "X_canon": f.X_canon, "C_canon": f.C, "N": f.N,
                   "N_updates": f.N_updates, "avg_conf": f.get_average_conf()}
            if mode == "best_score":
                rec["score"] = f.score
            for k, v in rec.items():  # one array per quantity, the calls stacked along axis 0
                seq.setdefault(k, []).append(np.array(v.numpy() if torch.is_tensor(v) else v))
            if name == "weighted_spherical":
                Xd, Cd = X.numpy().astype(np.float64), C.numpy().astype(np.float64)
                X64, C64 = (Xd, Cd) if c == 0 else sph_fuse64(X64, C64, Xd, Cd)
                dev.append(np.abs(f.X_canon.numpy().astype(np.float64) - X64).max())
        for k, v in seq.items():
            out[f"{name}_{k}"] = np.stack(v)
        if mode == "best_score":
            assert any(replaced) and not all(replaced), (name, replaced)
            out[name + "_replaced"] = np.array([True] + replaced)
        if name == "weighted_spherical":
            out["sph_dev"] = np.array(dev)
            print("weighted_spherical: reference f32 deviation from float64 per call", dev)
    path = os.path.join(HERE, "keyframe_golden.npz")
    write_npz(path, out)
    print("wrote", path, len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
