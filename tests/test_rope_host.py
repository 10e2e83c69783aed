"""RoPE2D without a GPU: the binding's argument checks (each a RuntimeError before any device
work), the ``curope`` drop-in module, ``m3s.rope.cuRoPE2D`` on CPU tensors and ``install`` on
stand-in modules."""
import ctypes

import numpy as np
import pytest
import torch

import rope_model as M


def tok(B=1, N=2, H=2, D=8, dtype=torch.float32):
    return torch.ones(B, N, H, D, dtype=dtype)


def pos(B=1, N=2):
    return torch.zeros(B, N, 2, dtype=torch.int64)


def both(backend, tokens, positions, match):
    """The same rejection from rope_2d and from either side of rope_2d_pair."""
    with pytest.raises(RuntimeError, match=match):
        backend.rope_2d(tokens, positions, 100.0)
    with pytest.raises(RuntimeError, match=match):
        backend.rope_2d_pair(tokens, tok(), positions, pos(), 100.0, 1.0)
    with pytest.raises(RuntimeError, match=match):
        backend.rope_2d_pair(tok(), tokens, pos(), positions, 100.0, 1.0)


def test_cpu_tensors_are_rejected(backend):
    both(backend, tok(), pos(), "no CPU path")
    qkv = torch.ones(1, 2, 3, 2, 8)
    both(backend, qkv[:, :, 1], pos(), "no CPU path")   # the callers' view passes the checks


def test_dtype_checks(backend):
    both(backend, tok(dtype=torch.float64), pos(), "expected scalar type Float or Half but found Double")
    both(backend, tok(dtype=torch.bfloat16), pos(), "expected scalar type Float or Half")
    both(backend, tok(), pos().int(), "expected scalar type Long but found Int")
    with pytest.raises(RuntimeError, match="q is torch.float32 and k is torch.float16"):
        backend.rope_2d_pair(tok(), tok(dtype=torch.float16), pos(), pos(), 100.0)


def test_positions_checks(backend):
    p = torch.zeros(1, 2, 4, dtype=torch.int64)[:, :, ::2]
    assert tuple(p.shape) == (1, 2, 2) and not p.is_contiguous()
    both(backend, tok(), p, "positions are not contiguous")
    both(backend, tok(), pos(1, 3), "bad pos.shape")
    both(backend, tok(), torch.zeros(1, 2, 3, dtype=torch.int64), "bad pos.shape")
    both(backend, tok(), torch.zeros(2, 2, dtype=torch.int64), "bad pos.shape")
    both(backend, tok(B=2), pos(), "bad pos.shape")


def test_token_dim_checks(backend):
    both(backend, tok(D=6), pos(), "token dim must be multiple of 4")
    both(backend, tok(D=260), pos(), "token dim must be in 4..256")
    both(backend, torch.ones(2, 2, 8), pos(), r"must be \[B,N,H,D\]")
    with pytest.raises(RuntimeError, match="must share B, H, D"):
        backend.rope_2d_pair(tok(), tok(H=3), pos(), pos(), 100.0)


def test_token_strides_are_checked(backend):
    # a contiguous [B,H,N,D] tensor seen as [B,N,H,D]: the H stride is N*D
    both(backend, torch.ones(1, 2, 2, 8).transpose(1, 2), pos(), "tokens are not contiguous")
    both(backend, torch.ones(1, 2, 2, 16)[..., ::2], pos(), "tokens are not contiguous")
    both(backend, torch.ones(1, 2, 4, 8)[:, :, ::2], pos(), "tokens are not contiguous")


def test_c_entry_points_validate_without_a_device(backend):
    """Return codes and m3s_last_error of the C entry points; nothing here reaches a launch."""
    A = backend.RopeArgs
    for f in (backend.lib.m3s_rope2d, backend.lib.m3s_rope2d_pair):
        assert f(None) == 1 and b"null args" in backend.lib.m3s_last_error()
        a = A(None, None, 4, 0, 0, None, None, 4, 0, 0, 1, 2, 6, 100.0, 1.0, 0, None)
        assert f(ctypes.byref(a)) == 1 and b"multiple of 4" in backend.lib.m3s_last_error()
        a.D = 260
        assert f(ctypes.byref(a)) == 1 and b"4..256" in backend.lib.m3s_last_error()
        a.D, a.dtype = 8, 2
        assert f(ctypes.byref(a)) == 1 and b"unknown dtype" in backend.lib.m3s_last_error()
        a.dtype, a.base = 0, -1.0
        assert f(ctypes.byref(a)) == 1 and b"base must be positive" in backend.lib.m3s_last_error()
        a.base = 100.0
        assert f(ctypes.byref(a)) == 1 and b"null pointer" in backend.lib.m3s_last_error()
        a.B = 0   # B*N == 0: success, no launch, the null pointers are never looked at
        assert f(ctypes.byref(a)) == 0


def test_curope_is_the_binding(backend):
    import curope

    assert curope.rope_2d is backend.rope_2d
    assert curope.__all__ == ["rope_2d"]


def test_module_on_cpu_equals_rope2d_torch():
    from m3s import rope as R

    assert R.RoPE2D is R.cuRoPE2D
    B, N, H, D = 2, 6, 3, 12
    t = torch.from_numpy(M.make_inputs(B, N, H, D, 5))
    p = torch.from_numpy(M.grid_positions(B, 2, 3, step=(1, 2)))
    want = R.rope2d_torch(t, p, 100.0, 1.0)
    assert want.data_ptr() != t.data_ptr() and not torch.equal(want, t)
    qkv = torch.zeros(B, N, 3, H, D)
    qkv[:, :, 1] = t
    k = qkv.transpose(1, 3)[:, :, 1]                       # [B,H,N,D], as blocks.py:97-98
    out = R.cuRoPE2D(freq=100.0)(k, p)
    assert out is k
    assert torch.equal(qkv[:, :, 1], want)                 # in place, through the view
    assert not qkv[:, :, 0].any() and not qkv[:, :, 2].any()

    # backward = the rotation by -F0, on a copy of the gradient
    x = t.clone().requires_grad_(True)
    w = torch.from_numpy(M.make_inputs(B, N, H, D, 6))
    y = R.cuRoPE2D(freq=100.0, F0=1.0)((x * 1.0).transpose(1, 2), p)   # [B,H,N,D]
    (w.transpose(1, 2) * y).sum().backward()
    assert torch.equal(x.grad, R.rope2d_torch(w, p, 100.0, -1.0))


class OldRope(torch.nn.Module):
    def __init__(self, freq=100.0, F0=1.0):
        super().__init__()
        self.base, self.F0 = freq, F0


class SelfAttn(torch.nn.Module):
    def __init__(self, dim, heads, rope):
        super().__init__()
        self.num_heads, self.scale, self.rope = heads, (dim // heads) ** -0.5, rope
        self.qkv = torch.nn.Linear(dim, 3 * dim)
        self.proj = torch.nn.Linear(dim, dim)


class CrossAttn(torch.nn.Module):
    def __init__(self, dim, heads, rope):
        super().__init__()
        self.num_heads, self.scale, self.rope = heads, (dim // heads) ** -0.5, rope
        self.projq, self.projk, self.projv, self.proj = (torch.nn.Linear(dim, dim) for _ in range(4))


class Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.rope = OldRope(100.0, 1.0)
        other = OldRope(50.0, 2.0)
        self.enc = torch.nn.ModuleList([SelfAttn(8, 2, self.rope), SelfAttn(8, 2, self.rope)])
        self.dec = torch.nn.ModuleList([CrossAttn(8, 2, self.rope), SelfAttn(8, 2, None),
                                        SelfAttn(8, 2, other)])
        self.mlp = torch.nn.Linear(8, 8)


def test_install_swaps_and_counts():
    from m3s import rope as R

    net = Net()
    assert R.install(net, fuse=False) == 5          # net itself, 2 enc, dec[0], dec[2]
    assert isinstance(net.rope, R.cuRoPE2D) and (net.rope.base, net.rope.F0) == (100.0, 1.0)
    assert net.enc[0].rope is net.rope and net.enc[1].rope is net.rope and net.dec[0].rope is net.rope
    assert net.dec[1].rope is None
    assert isinstance(net.dec[2].rope, R.cuRoPE2D) and net.dec[2].rope is not net.rope
    assert (net.dec[2].rope.base, net.dec[2].rope.F0) == (50.0, 2.0)
    assert "forward" not in vars(net.enc[0]) and "forward" not in vars(net.dec[0])

    net = Net()
    assert R.install(net) == 5
    assert net.enc[0].forward.__func__ is R.attention_forward
    assert net.dec[2].forward.__func__ is R.attention_forward
    assert net.dec[0].forward.__func__ is R.cross_attention_forward
    assert "forward" not in vars(net.dec[1]) and "forward" not in vars(net) and "forward" not in vars(net.mlp)

    # the bound forwards run (CPU: rope2d_torch) and equal the reference expressions
    B, N, Nk = 2, 6, 4
    g = torch.Generator().manual_seed(0)
    x, y = torch.randn(B, N, 8, generator=g), torch.randn(B, Nk, 8, generator=g)
    xp = torch.from_numpy(M.grid_positions(B, 2, 3, step=(1, 2)))
    yp = torch.from_numpy(M.grid_positions(B, 2, 2, step=(3, 1)))
    with torch.no_grad():
        a = net.enc[0]
        qkv = a.qkv(x).reshape(B, N, 3, 2, 4)
        q, k = (R.rope2d_torch(qkv[:, :, i], xp, 100.0, 1.0).transpose(1, 2) for i in range(2))
        s = ((q @ k.transpose(-2, -1)) * a.scale).softmax(dim=-1)
        want = a.proj((s @ qkv[:, :, 2].transpose(1, 2)).transpose(1, 2).reshape(B, N, 8))
        torch.testing.assert_close(a(x, xp), want, rtol=1e-5, atol=1e-6)   # matmul layouts differ

        c = net.dec[0]
        q = R.rope2d_torch(c.projq(x).reshape(B, N, 2, 4), xp, 100.0, 1.0).transpose(1, 2)
        k = R.rope2d_torch(c.projk(y).reshape(B, Nk, 2, 4), yp, 100.0, 1.0).transpose(1, 2)
        v = c.projv(y).reshape(B, Nk, 2, 4).transpose(1, 2)
        s = ((q @ k.transpose(-2, -1)) * c.scale).softmax(dim=-1)
        want = c.proj((s @ v).transpose(1, 2).reshape(B, N, 8))
        torch.testing.assert_close(c(x, y, y, xp, yp), want, rtol=1e-5, atol=1e-6)
    assert np.isfinite(want.numpy()).all()
