"""Generate the RoPE2D golden fixture from the REFERENCE Python (dev container only).

Run from the repo root:  python tests/golden/make_rope_golden.py
Writes tests/golden/rope_golden.npz (inputs + reference outputs + the measured Ta / Tc).

Pinned (reference file:line), in float32 torch on the CPU, as written: ``RoPE2D`` of
thirdparty/mast3r/dust3r/croco/models/pos_embed.py:112-159 -- the class the reference runs when its
compiled ``curope`` extension does not import (:106-110), which is the case here and on ROCm -- with
freq = 100, on the positions of ``PositionGetter`` (croco/models/blocks.py:195-207) for a 5 x 7
patch grid.  Only ``croco/`` is put on ``sys.path`` (never this repository's package directory,
whose own ``curope`` would otherwise be picked up).

Cases, all B = 2, H = 3, N = 35: ``d64`` (D = 64), ``d20`` (D = 20: a head run with no 16-byte
alignment), ``far`` (D = 64, positions 9 p + 3, up to 57).  Tokens: tests/rope_model.py make_inputs.
The reference's f16 path computes its angles in f16 and is no yardstick: f32 only.

Ta: the largest relative distance, in u = 2^-24, of the reference's own f32 angle (position times
f32 inverse frequency, :122-124) from the f64 angle.  Tc: the largest absolute distance, in u, of
its f32 cos / sin table (:126-127) from f64 cos / sin of that same f32 angle.  The angle expression
is restated here and checked to give the reference's tables bit for bit.  The tests' bounds use twice
each (at least 2 u); the generator asserts that the reference's outputs are inside that bound of the
f64 model.

The reference is read from /root/reference at generation time only; nothing under tests/ imports
it at run time, and no reference source is copied.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import rope_model as M  # noqa: E402

B, H, GH, GW, SEED = 2, 3, 5, 7, 30
CASES = (("d64", 64, 1, 0), ("d20", 20, 1, 0), ("far", 64, 9, 3))  # name, D, pos scale, pos offset


def main():
    sys.path.insert(0, os.path.join(REF, "thirdparty", "mast3r", "dust3r", "croco"))
    from models.blocks import PositionGetter
    from models.pos_embed import RoPE2D

    assert RoPE2D.__module__ == "models.pos_embed", "the compiled path was picked up"
    out = {}
    Ta = Tc = 0.0
    per_case = []
    with torch.no_grad():
        for k, (name, D, scale, off) in enumerate(CASES):
            pos = PositionGetter()(B, GH, GW, "cpu") * scale + off          # B,N,2 int64
            tok = M.make_inputs(B, GH * GW, H, D, SEED + k)                 # B,N,H,D f32
            rope = RoPE2D(freq=M.BASE)
            ref = rope(torch.from_numpy(tok).transpose(1, 2), pos)         # B,H,N,D
            ref = np.ascontiguousarray(ref.transpose(1, 2).numpy())
            assert ref.dtype == np.float32 and ref.shape == tok.shape

            # the reference's f32 angles and tables on this case's arguments
            half = D // 2
            inv32 = 1.0 / (M.BASE ** (torch.arange(0, half, 2).float() / half))
            t = torch.arange(int(pos.max()) + 1, dtype=torch.float32)
            ang32 = t[:, None] * inv32[None, :]
            (cos_t, sin_t), = rope.cache.values()
            Q = D // 4
            assert torch.equal(cos_t[:, :Q], ang32.cos()) and torch.equal(sin_t[:, :Q], ang32.sin())
            a32 = ang32.numpy().astype(np.float64)
            a64 = t.numpy().astype(np.float64)[:, None] * M.inv_freq_f64(D)
            nz = a64 != 0
            ta = float((np.abs(a32 - a64)[nz] / np.abs(a64)[nz]).max() / M.U)
            tc = float(max(np.abs(cos_t[:, :Q].numpy() - np.cos(a32)).max(),
                           np.abs(sin_t[:, :Q].numpy() - np.sin(a32)).max()) / M.U)
            Ta, Tc = max(Ta, ta), max(Tc, tc)
            per_case.append((name, tok, pos.numpy(), ref, ta, tc))
            out[f"{name}_tokens"], out[f"{name}_pos"], out[f"{name}_ref"] = tok, pos.numpy(), ref

    for name, tok, pos, ref, ta, tc in per_case:
        m64 = M.model_f64(tok, pos)
        bd = M.bound(tok, pos, M.tol(Ta), M.tol(Tc))
        err = np.abs(ref.astype(np.float64) - m64)
        print(f"{name} {ref.shape}: Ta {ta:.3f} u, Tc {tc:.3f} u; reference f32 within "
              f"{err.max():.2e} of f64 (largest err/bound {np.max(err / bd):.3f})")
        assert np.all(err <= bd), name
    out["Ta"], out["Tc"] = np.array(Ta), np.array(Tc)
    out["base"] = np.array(M.BASE)
    print(f"Ta = {Ta:.3f} u, Tc = {Tc:.3f} u")
    path = os.path.join(HERE, "rope_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
