"""RoPE2D of the MASt3R attention on the HIP kernel -- mirror of the reference's
``croco/models/curope/curope2d.py`` and of the two attention forwards that call it
(``croco/models/blocks.py:94-112``, ``:149-169``).

The reference's ``pos_embed.py:106-110`` takes ``cuRoPE2D`` when the compiled extension imports and
a torch fallback (``:112-159``) otherwise; on ROCm the fallback runs: a host wait on
``positions.max()`` and about a dozen launches per call, two calls per attention.  Here

* ``cuRoPE2D_func`` / ``cuRoPE2D`` (``RoPE2D``)  the reference module on
  ``mast3r_slam_backends.rope_2d`` (csrc/rope.hip): one launch, in place, no host wait
* ``rope2d_torch``                  the formula as out-of-place torch expressions: the CPU path and
                                    the comparison of the HIP op
* ``attention_forward`` / ``cross_attention_forward``  the reference forwards with q and k rotated
                                    by ONE ``rope_2d_pair`` launch
* ``install``                       swaps these into a loaded network

``install`` has not run against the real network here (no checkpoint): the stand-in modules of the
tests have the attributes the reference's ``Attention`` / ``CrossAttention`` have.
"""
from __future__ import annotations

import types

import torch

import mast3r_slam_backends


def rope2d_torch(tokens, positions, base, F0=1.0):
    """``tokens`` [B,N,H,D], ``positions`` [B,N,2] int64 -> the rotated tokens, a new tensor of the
    same dtype.  With Q = D/4 a head is [u_Y | v_Y | u_X | v_X] and, for axis A and i < Q,
    theta = float(pos_A) * inv_freq_i, u' = u cos - v sin, v' = v cos + u sin, in f32;
    inv_freq_i = F0 / base^(i/Q) is computed in f64 and rounded to f32, as the HIP op's host side
    does.  No table indexed by position, so any int64 position is accepted and nothing waits for
    ``positions.max()``."""
    B, N, H, D = tokens.shape
    if D % 4:
        raise RuntimeError(f"token dim must be multiple of 4, got {D}")
    Q = D // 4
    i = torch.arange(Q, dtype=torch.float64)
    inv_freq = (float(F0) / torch.tensor(float(base), dtype=torch.float64) ** (i / Q)).to(torch.float32)
    theta = positions.to(torch.float32)[..., None] * inv_freq.to(tokens.device)   # B,N,2,Q
    c, s = theta.cos()[:, :, None], theta.sin()[:, :, None]                       # B,N,1,2,Q
    t = tokens.to(torch.float32).reshape(B, N, H, 2, 2, Q)                        # axis, u|v, i
    u, v = t[..., 0, :], t[..., 1, :]
    out = torch.stack((u * c - v * s, v * c + u * s), dim=-2)
    return out.reshape(B, N, H, D).to(tokens.dtype)


def _rope_inplace(tokens, positions, base, F0):
    if tokens.device.type == "cuda":
        mast3r_slam_backends.rope_2d(tokens, positions, base, F0)
    else:
        tokens.copy_(rope2d_torch(tokens, positions, base, F0))


class cuRoPE2D_func(torch.autograd.Function):
    """curope2d.py:12-29.  ``tokens`` is the [B,N,H,D] view; rotated in place.  The backward pass
    is the same rotation with -F0, on a copy of the incoming gradient (the reference rotates the
    gradient buffer itself, which autograd may share)."""

    @staticmethod
    def forward(ctx, tokens, positions, base, F0=1):
        ctx.save_for_backward(positions)
        ctx.saved_base = base
        ctx.saved_F0 = F0
        _rope_inplace(tokens, positions, base, F0)
        ctx.mark_dirty(tokens)
        return tokens

    @staticmethod
    def backward(ctx, grad_res):
        positions, base, F0 = ctx.saved_tensors[0], ctx.saved_base, ctx.saved_F0
        grad = grad_res.clone(memory_format=torch.contiguous_format)
        _rope_inplace(grad, positions, base, -F0)
        return grad, None, None, None


class cuRoPE2D(torch.nn.Module):
    """curope2d.py:32-40: ``tokens`` [B,H,N,D] is a view whose ``transpose(1, 2)`` has H, D strides
    (D, 1) -- what ``blocks.py:97-98`` and ``:154-155`` produce; it is rotated in place and
    returned.  CPU tensors take ``rope2d_torch``."""

    def __init__(self, freq=100.0, F0=1.0):
        super().__init__()
        self.base = freq
        self.F0 = F0

    def forward(self, tokens, positions):
        cuRoPE2D_func.apply(tokens.transpose(1, 2), positions, self.base, self.F0)
        return tokens


RoPE2D = cuRoPE2D


def _rotate_pair(rope, q, k, qpos, kpos):
    """q, k: [B,N,H,D] views, rotated in place -- by one launch where nothing needs a gradient."""
    needs_grad = torch.is_grad_enabled() and (q.requires_grad or k.requires_grad)
    if q.device.type == "cuda" and not needs_grad:
        mast3r_slam_backends.rope_2d_pair(q, k, qpos, kpos, rope.base, rope.F0)
    else:
        cuRoPE2D_func.apply(q, qpos, rope.base, rope.F0)
        cuRoPE2D_func.apply(k, kpos, rope.base, rope.F0)


def _same(x):
    return x


def attention_forward(attn, x, xpos):
    """``Attention.forward`` (blocks.py:94-112) with one ``rope_2d_pair`` for q and k."""
    B, N, C = x.shape

    qkv = attn.qkv(x).reshape(B, N, 3, attn.num_heads, C // attn.num_heads)
    if attn.rope is not None:
        _rotate_pair(attn.rope, qkv[:, :, 0], qkv[:, :, 1], xpos, xpos)
    qkv = qkv.transpose(1, 3)
    q, k, v = [qkv[:, :, i] for i in range(3)]

    a = (q @ k.transpose(-2, -1)) * attn.scale
    a = a.softmax(dim=-1)
    a = getattr(attn, "attn_drop", _same)(a)

    x = (a @ v).transpose(1, 2).reshape(B, N, C)
    x = attn.proj(x)
    x = getattr(attn, "proj_drop", _same)(x)
    return x


def cross_attention_forward(attn, query, key, value, qpos, kpos):
    """``CrossAttention.forward`` (blocks.py:149-169) with one ``rope_2d_pair`` for q and k."""
    B, Nq, C = query.shape
    Nk = key.shape[1]
    Nv = value.shape[1]

    q = attn.projq(query).reshape(B, Nq, attn.num_heads, C // attn.num_heads)
    k = attn.projk(key).reshape(B, Nk, attn.num_heads, C // attn.num_heads)
    v = attn.projv(value).reshape(B, Nv, attn.num_heads, C // attn.num_heads).permute(0, 2, 1, 3)
    if attn.rope is not None:
        _rotate_pair(attn.rope, q, k, qpos, kpos)
    q = q.permute(0, 2, 1, 3)
    k = k.permute(0, 2, 1, 3)

    a = (q @ k.transpose(-2, -1)) * attn.scale
    a = a.softmax(dim=-1)
    a = getattr(attn, "attn_drop", _same)(a)

    x = (a @ v).transpose(1, 2).reshape(B, Nq, C)
    x = attn.proj(x)
    x = getattr(attn, "proj_drop", _same)(x)
    return x


_SELF_ATTRS = ("qkv", "proj", "num_heads", "scale", "rope")
_CROSS_ATTRS = ("projq", "projk", "projv", "proj", "num_heads", "scale", "rope")


def install(model, fuse=True):
    """Replace every non-None ``rope`` attribute in ``model``'s module tree by one ``cuRoPE2D``
    with the old object's ``base`` and ``F0`` (one per distinct pair), and, with ``fuse``, bind
    ``attention_forward`` / ``cross_attention_forward`` onto the modules that have the reference's
    ``Attention`` / ``CrossAttention`` attributes.  Returns the number of modules changed."""
    made = {}
    changed = 0
    for m in list(model.modules()):
        old = getattr(m, "rope", None)
        if old is None:
            continue
        key = (float(old.base), float(old.F0))
        if key not in made:
            made[key] = cuRoPE2D(freq=old.base, F0=old.F0)
        m.rope = made[key]
        if fuse:
            if all(hasattr(m, a) for a in _CROSS_ATTRS):
                m.forward = types.MethodType(cross_attention_forward, m)
            elif all(hasattr(m, a) for a in _SELF_ATTRS):
                m.forward = types.MethodType(attention_forward, m)
        changed += 1
    return changed
