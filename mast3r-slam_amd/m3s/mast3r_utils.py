"""From the raw outputs of the two MASt3R heads to what matching, the tracker and the factor graph
consume -- the model-free part of mast3r_slam/mast3r_utils.py:43-231.

The reference runs each head to the end in torch (``Cat_MLP_LocalFeatures_DPT_Pts3d.forward``,
thirdparty/mast3r/mast3r/catmlp_dpt_head.py:71-96: transpose, view, pixel_shuffle, cat,
postprocess), then stacks, downsamples and concatenates the heads' X, C, D, Q.  Here a *raw head*
is the pair ``(pts, feat)`` of the two sub-heads' outputs,

* ``pts``  [B,4,H,W]            ``head.dpt(...)``                (catmlp_dpt_head.py:73)
* ``feat`` [B,S,(F+1)*patch^2]  ``head.head_local_features(...)`` (catmlp_dpt_head.py:82)

(``raw_head`` below gets it from a loaded network), and ``mast3r_slam_backends.head_finish``
turns it into X, C, D, Q in one launch per head, written straight into the stacked buffers:

* ``finish_heads``                   the stacked X, C, D, Q of n heads     (:73-79, :129-134, :200-206)
* ``mast3r_inference_mono_raw``      Xii, Cii                              (:119-139)
* ``mast3r_match_asymmetric_raw``    the tracker's 8-tuple                 (:209-231)
* ``mast3r_match_symmetric_raw``     add_factors' 8-tuple                  (:142-180)
* ``postprocess_torch``              the reference's expressions in torch: the CPU path of
                                     ``finish_heads`` and the comparison of the HIP op
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .config import config as _global_config

INF = float("inf")
# (vmin, vmax) of the checkpoint's conf_mode and desc_conf_mode, both 'exp'
# (thirdparty/mast3r/README.md:297)
CONF = (1.0, INF)
DESC_CONF = (0.0, INF)
PATCH = 16


def shuffle_tokens(feat, H, W, patch=PATCH):
    """[B,S,(F+1)*patch^2] -> [B,F+1,H,W] (catmlp_dpt_head.py:83-84)."""
    B, S, width = feat.shape
    grid = feat.transpose(-1, -2).reshape(B, width, H // patch, W // patch)
    return F.pixel_shuffle(grid, patch)


def postprocess_torch(out, desc_dim=None, conf=CONF, desc_conf=DESC_CONF, downsample=1):
    """``out`` [B,4,H,W] or [B,4+desc_dim+1,H,W], channel-planar, -> (X, C, D, Q) as the reference
    computes them (depth 'exp', conf 'exp', desc 'norm', two_confs; catmlp_dpt_head.py:17-39,
    dust3r/heads/postprocess.py:22-58), then ``[::downsample]`` (mast3r_utils.py:43-52).  D and Q
    are None without desc_dim."""
    fmap = out.permute(0, 2, 3, 1)  # B,H,W,channels
    xyz = fmap[..., 0:3]
    d = xyz.norm(dim=-1, keepdim=True)
    X = xyz / d.clip(min=1e-8) * torch.expm1(d)
    C = conf[0] + fmap[..., 3].exp().clip(max=conf[1] - conf[0])
    D = Q = None
    if desc_dim is not None:
        desc = fmap[..., 4:4 + desc_dim]
        D = desc / desc.norm(dim=-1, keepdim=True)
        Q = desc_conf[0] + fmap[..., 4 + desc_dim].exp().clip(max=desc_conf[1] - desc_conf[0])
    ds = int(downsample)
    if ds > 1:
        X, C = X[..., ::ds, ::ds, :], C[..., ::ds, ::ds]
        if D is not None:
            D, Q = D[..., ::ds, ::ds, :], Q[..., ::ds, ::ds]
    return (X.contiguous(), C.contiguous(), None if D is None else D.contiguous(),
            None if Q is None else Q.contiguous())


def raw_head(head, decout, img_shape):
    """The raw head of a loaded network: ``head`` is ``model.downstream_head1`` / ``2``,
    ``decout`` the decoder's token list in f32 and ``img_shape`` (H, W), as in
    ``model._downstream_head`` (mast3r_utils.py:34-40).  Calls the two sub-heads of
    ``head.forward`` (catmlp_dpt_head.py:73-82) and stops before the shuffle and postprocess."""
    pts = head.dpt(decout, image_size=(int(img_shape[0]), int(img_shape[1])))
    feat = head.head_local_features(torch.cat([decout[0], decout[-1]], dim=-1))
    return pts, feat


def _downsample(downsample, cfg):
    if downsample is None:
        downsample = (cfg if cfg is not None else _global_config)["dataset"]["img_downsample"]
    return max(int(downsample), 1)


def finish_heads(raw_heads, downsample=None, cfg=None):
    """n raw heads of equal shape -> stacked X [n*B,h,w,3], C [n*B,h,w], D [n*B,h,w,F],
    Q [n*B,h,w]; head k fills rows k*B..(k+1)*B-1, so for B = 1 this is the reference's
    ``torch.stack`` over the heads followed by ``downsample``.  One ``head_finish`` per head, each
    writing its slice.  Heads whose ``feat`` is None give D = Q = None (all or none).
    ``downsample`` defaults to ``config["dataset"]["img_downsample"]``.  CPU tensors go through
    ``postprocess_torch``."""
    ds = _downsample(downsample, cfg)
    n = len(raw_heads)
    pts0, feat0 = raw_heads[0]
    B, _, H, W = pts0.shape
    with_desc = feat0 is not None
    for pts, feat in raw_heads:
        if tuple(pts.shape) != (B, 4, H, W) or (feat is not None) != with_desc or (
                with_desc and feat.shape != feat0.shape):
            raise ValueError("finish_heads: the raw heads differ in shape")
    Fd = feat0.shape[2] // (PATCH * PATCH) - 1 if with_desc else 0
    h, w = -(-H // ds), -(-W // ds)
    new = lambda *s: torch.empty(s, dtype=torch.float32, device=pts0.device)
    X, C = new(n * B, h, w, 3), new(n * B, h, w)
    D, Q = (new(n * B, h, w, Fd), new(n * B, h, w)) if with_desc else (None, None)
    for k, (pts, feat) in enumerate(raw_heads):
        sl = slice(k * B, (k + 1) * B)
        if pts.device.type == "cuda":
            import mast3r_slam_backends

            mast3r_slam_backends.head_finish(
                pts, feat, layout="tokens", patch=PATCH, downsample=ds, conf=CONF,
                desc_conf=DESC_CONF, out=(X[sl], C[sl], D[sl] if with_desc else None,
                                          Q[sl] if with_desc else None))
        else:
            planar = torch.cat([pts, shuffle_tokens(feat, H, W)], dim=1) if with_desc else pts
            res = postprocess_torch(planar, Fd if with_desc else None, CONF, DESC_CONF, ds)
            X[sl], C[sl] = res[0], res[1]
            if with_desc:
                D[sl], Q[sl] = res[2], res[3]
    return X, C, D, Q


def mast3r_inference_mono_raw(raw_ii, downsample=None, cfg=None):
    """mast3r_inference_mono (mast3r_utils.py:119-139) after the network: Xii [hw,3], Cii [hw,1]
    of a one-image raw head.  Only the points head is read."""
    X, C, _, _ = finish_heads([(raw_ii[0], None)], downsample, cfg)
    if X.shape[0] != 1:
        raise ValueError("mast3r_inference_mono_raw: one image at a time")
    return X[0].view(-1, 3), C[0].view(-1, 1)


def mast3r_match_asymmetric_raw(raw_ii, raw_ji, idx_i2j_init=None, downsample=None, cfg=None):
    """mast3r_match_asymmetric (mast3r_utils.py:209-231) after the network ->
    (idx_i2j, valid_match_j, Xii, Cii, Qii, Xji, Cji, Qji)."""
    from . import matching

    X, C, D, Q = finish_heads([raw_ii, raw_ji], downsample, cfg)
    b = X.shape[0] // 2
    if b != 1:  # the reference unpacks the two heads from the leading dimension
        raise ValueError("mast3r_match_asymmetric_raw: one image pair at a time")
    idx_i2j, valid_match_j = matching.match(X[:b], X[b:], D[:b], D[b:],
                                            idx_1_to_2_init=idx_i2j_init, cfg=cfg)
    Xii, Xji = X.view(2, -1, 3)
    Cii, Cji = C.view(2, -1, 1)
    Qii, Qji = Q.view(2, -1, 1)
    return idx_i2j, valid_match_j, Xii, Cii, Qii, Xji, Cji, Qji


def mast3r_match_symmetric_raw(raw_ii, raw_ji, raw_jj, raw_ij, downsample=None, cfg=None):
    """mast3r_match_symmetric (mast3r_utils.py:142-180) after the network, for b keyframe pairs
    (each raw head [b,...]) -> (idx_i2j, idx_j2i, valid_match_j, valid_match_i, Qii, Qjj, Qji, Qij),
    the arguments of ``FactorGraph.add_matched_factors``.  The heads are written directly into
    X11 / D11 = [ii; jj] and X21 / D21 = [ji; ij]; nothing is stacked or concatenated."""
    from . import matching

    X11, _, D11, Q11 = finish_heads([raw_ii, raw_jj], downsample, cfg)
    X21, _, D21, Q21 = finish_heads([raw_ji, raw_ij], downsample, cfg)
    b = X11.shape[0] // 2
    idx_1_to_2, valid_match_2 = matching.match(X11, X21, D11, D21, cfg=cfg)
    return (idx_1_to_2[:b], idx_1_to_2[b:], valid_match_2[:b], valid_match_2[b:],
            Q11[:b].view(b, -1, 1), Q11[b:].view(b, -1, 1),
            Q21[:b].view(b, -1, 1), Q21[b:].view(b, -1, 1))
