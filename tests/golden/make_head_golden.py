"""Generate the head-finish golden fixture from the REFERENCE Python (dev container only).

Run from the repo root:  python tests/golden/make_head_golden.py
Writes tests/golden/head_golden.npz (inputs + reference outputs + the measured exp / expm1 terms).

Pinned (reference file:line), in float32 torch on the CPU, as written:
* Cat_MLP_LocalFeatures_DPT_Pts3d.forward (thirdparty/mast3r/mast3r/catmlp_dpt_head.py:71-96) is
  called unbound on a stand-in object whose two sub-heads (``dpt``, ``head_local_features``) return
  the synthetic raw tensors, so its transpose / view / F.pixel_shuffle / torch.cat (:83-87) and its
  postprocess call (:88-95 -> :25-39, reg_desc :17-22, reg_dense_depth / reg_dense_conf of
  dust3r/heads/postprocess.py:22-58) run as they are, with the checkpoint's modes
  (thirdparty/mast3r/README.md:297: depth exp unbounded, conf exp (1, inf), desc norm,
  two_confs, desc_conf exp (0, inf));
* mast3r_slam.mast3r_utils.downsample (mast3r_utils.py:43-52) with
  config["dataset"]["img_downsample"] = 2.
mast3r.catmlp_dpt_head needs only the three thirdparty paths.  mast3r_slam.mast3r_utils also
imports the network, the retrieval database, the matcher and dust3r's image transforms
(torchvision is absent): import-time dependencies only, stubbed empty.

Inputs: B=1, H=32, W=48, F=24 (tests/head_model.py make_inputs: random directions, |xyz|
log-uniform in [1e-3, 4], logits uniform in [-4, 4], standard-normal descriptors).

T_expm1 / T_exp: the largest distance, in u = 2^-24 relative, of the reference's own f32
torch.expm1 / torch.exp from f64 on the fixture's arguments; the tests' bounds use twice these
(at least 2 u).  The generator asserts that the reference's f32 outputs are inside those bounds of
the f64 model.

The reference is read from /root/reference at generation time only; nothing under tests/ imports
it at run time, and no reference source is copied.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import head_model as M  # noqa: E402

B, H, W, F, SEED = 1, 32, 48, 24, 20
INF = float("inf")


def install_stubs():
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m

    tp = os.path.join(REF, "thirdparty", "mast3r")
    sys.path[:0] = [REF, tp, os.path.join(tp, "dust3r"), os.path.join(tp, "dust3r", "croco")]
    import mast3r  # noqa: F401  (the real package; only mast3r.model is replaced)
    import dust3r.utils  # noqa: F401

    stub("mast3r.model", AsymmetricMASt3R=None)
    stub("dust3r.utils.image", ImgNorm=None)
    stub("mast3r_slam.retrieval_database", RetrievalDatabase=None)
    stub("mast3r_slam.matching")


def rel_u(got32, ref64):
    return float((np.abs(got32.astype(np.float64) - ref64) / np.abs(ref64)).max() / M.U)


def main():
    install_stubs()
    from mast3r import catmlp_dpt_head as rhead
    from mast3r_slam import config as rcfg
    from mast3r_slam import mast3r_utils as rmu

    rcfg.load_config(os.path.join(REF, "config", "base.yaml"))
    pts, planar = M.make_inputs(B, H, W, F, SEED)
    feat = M.unshuffle(planar)
    S = feat.shape[1]

    head = types.SimpleNamespace(
        dpt=lambda decout, image_size: torch.from_numpy(pts),
        head_local_features=lambda cat: torch.from_numpy(feat),
        patch_size=M.P, postprocess=rhead.postprocess, local_feat_dim=F,
        depth_mode=("exp", -INF, INF), conf_mode=("exp", 1, INF), desc_mode="norm",
        two_confs=True, desc_conf_mode=("exp", 0, INF))
    decout = [torch.zeros((B, S, 1)), torch.zeros((B, S, 1))]
    with torch.no_grad():
        res = rhead.Cat_MLP_LocalFeatures_DPT_Pts3d.forward(head, decout, (H, W))
        full = (res["pts3d"], res["conf"], res["desc"], res["desc_conf"])
        rcfg.config["dataset"]["img_downsample"] = 2
        half = rmu.downsample(*full)
        rcfg.config["dataset"]["img_downsample"] = 1
        assert all(a is b for a, b in zip(rmu.downsample(*full), full))

        # the reference's own f32 functions against f64 on this fixture's arguments
        xyz = torch.from_numpy(pts).permute(0, 2, 3, 1)[..., 0:3]
        d32 = xyz.norm(dim=-1)
        T_expm1 = rel_u(torch.expm1(d32).numpy(), np.expm1(d32.numpy().astype(np.float64)))
        logits = torch.from_numpy(np.concatenate([pts[:, 3].ravel(), planar[:, F].ravel()]))
        T_exp = rel_u(torch.exp(logits).numpy(), np.exp(logits.numpy().astype(np.float64)))

    out = {"pts": pts, "feat": feat, "F": np.array(F), "T_expm1": np.array(T_expm1),
           "T_exp": np.array(T_exp)}
    names = ("X", "C", "D", "Q")
    for ds, ref in ((1, full), (2, half)):
        m64 = M.model_f64(pts, planar, ds)
        dn = M.norm_f64(pts, ds)[..., None]
        bounds = (M.bound_X(dn, M.tol(T_expm1)), M.bound_CQ(M.tol(T_exp)), M.bound_D(F),
                  M.bound_CQ(M.tol(T_exp)))
        for n, r, m, bd in zip(names, ref, m64, bounds):
            r = np.ascontiguousarray(r.numpy())
            assert r.dtype == np.float32 and r.shape == m.shape
            e = M.rel_err_u(r, m)
            print(f"ds={ds} {n} {r.shape}: reference f32 within {e.max():.2f} u of f64 "
                  f"(bound {np.max(bd) / M.U:.1f} u)")
            assert np.all(e * M.U <= bd), (ds, n)
            out[f"ds{ds}_{n}"] = r
    print(f"T_expm1 = {T_expm1:.3f} u, T_exp = {T_exp:.3f} u")
    m32 = M.model_f32(pts, planar, 1)
    print("torch norm == sequential model (D bitwise): "
          f"{np.mean(m32[2] == out['ds1_D']) * 100:.1f} % of values")
    path = os.path.join(HERE, "head_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
