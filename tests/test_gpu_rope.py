"""RoPE2D on the device (rope.hip via mast3r_slam_backends.rope_2d / rope_2d_pair, the ``curope``
drop-in and m3s.rope) against the f64 host model (tests/rope_model.py) inside the derived bound,
the reference's own outputs (tests/golden/rope_golden.npz), and the identities that hold exactly.

Shapes are the smallest at which the indexing can go wrong: two batch items with different
positions (pos batch stride), N = 6 as a 2 x 3 grid (y differs from x), D = 64 with 3, 8, 9 and 16
heads (a masked step, an exact step, a step plus a tail, two steps of the wave-per-token kernel),
the other D through the pair-per-thread kernel (D = 12 in f16 is a 24-byte head run), the q and k
thirds of a packed qkv buffer and a contiguous tensor.  Every buffer is padded and filled with a
canary pattern: all bytes outside the addressed tokens, the v third included, must come back
unchanged."""
import functools
import os

import numpy as np
import pytest
import torch

import rope_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
PAD = 64          # canary elements in front of and behind every buffer (keeps 16-byte alignment)
B, GH, GW = 2, 2, 3
N = GH * GW
NP = {torch.float32: np.float32, torch.float16: np.float16}
DTYPES = [torch.float32, torch.float16]
LAYOUTS = ("q", "k", "contiguous")


@functools.lru_cache(maxsize=None)
def gold():
    g = np.load(os.path.join(HERE, "golden", "rope_golden.npz"))
    return dict(g=g, Ta=M.tol(g["Ta"]), Tc=M.tol(g["Tc"]))


@functools.lru_cache(maxsize=None)
def grid_pos():
    return M.grid_positions(B, GH, GW, step=(1, 2))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint16)


class Buf:
    """A padded canary buffer on the device holding tokens [B,N,H,D] in the given layout:
    ``q`` / ``k``: qkv[:, :, 0] / qkv[:, :, 1] of a [B,N,3,H,D] buffer; ``contiguous``.  ``shift``
    moves the buffer by that many elements (breaks the 16-byte alignment)."""

    def __init__(self, tokens, layout, seed=99, shift=0):
        Bq, Nq, H, D = tokens.shape
        third = {"q": 0, "k": 1, "contiguous": 0}[layout]
        shape = (Bq, Nq, 3, H, D) if layout != "contiguous" else (Bq, Nq, 1, H, D)
        rng = np.random.default_rng(seed)
        n = int(np.prod(shape))
        host = rng.standard_normal(2 * PAD + shift + n).astype(tokens.dtype)
        body = host[PAD + shift:PAD + shift + n].reshape(shape)
        body[:, :, third] = tokens
        self.before = host.copy()
        self.mask = np.zeros(host.shape, bool)                 # the addressed tokens
        m = self.mask[PAD + shift:PAD + shift + n].reshape(shape)
        m[:, :, third] = True
        self.flat = torch.from_numpy(host).to(DEV)
        self.view = self.flat[PAD + shift:PAD + shift + n].view(shape)[:, :, third]
        assert self.view.shape == tokens.shape and self.view.stride()[2:] == (D, 1)

    def after(self):
        """(tokens after the call, True when every other byte is unchanged)."""
        host = self.flat.cpu().numpy()
        untouched = np.array_equal(bits(host)[~self.mask], bits(self.before)[~self.mask])
        return host[self.mask].reshape(self.view.shape), untouched


def check_model(got, tokens, pos, dtype, F0=1.0):
    G = gold()
    m64 = M.model_f64(tokens, pos, F0=F0)
    bd = M.bound(tokens, pos, G["Ta"], G["Tc"], F0=F0, dtype=NP[dtype], model=m64)
    err = np.abs(got.astype(np.float64) - m64)
    print(f"{tuple(tokens.shape)} {NP[dtype].__name__}: largest err {err.max():.2e}, "
          f"err/bound {np.max(err / bd):.3f}")
    assert got.dtype == NP[dtype]
    assert np.all(err <= bd), float(np.max(err / bd))


def run_layouts(H, D, dtype, pos, seed):
    import mast3r_slam_backends as mb

    tokens = M.make_inputs(pos.shape[0], pos.shape[1], H, D, seed, NP[dtype])
    p = torch.from_numpy(pos).to(DEV)
    outs = []
    for layout in LAYOUTS:
        buf = Buf(tokens, layout)
        assert mb.rope_2d(buf.view, p, M.BASE, 1.0) is None
        got, untouched = buf.after()
        assert untouched, f"{layout}: bytes outside the addressed tokens changed"
        check_model(got, tokens, pos, dtype)
        outs.append(got)
    for o in outs[1:]:
        assert np.array_equal(bits(o), bits(outs[0])), "the layouts disagree"
    return tokens, outs[0]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("H", [3, 8, 9, 16])
def test_d64_against_model(H, dtype):
    run_layouts(H, 64, dtype, grid_pos(), seed=H)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("D", [4, 8, 12, 20, 128, 256])
def test_generic_d_against_model(D, dtype):
    run_layouts(2, D, dtype, grid_pos(), seed=D)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("H,D", [(3, 64), (2, 12)])
def test_arbitrary_positions(H, D, dtype):
    """0, 200, negative and large positions: the model only (no table could hold them)."""
    run_layouts(H, D, dtype, M.wild_positions(B, N, seed=7), seed=11)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_d64_unaligned_buffer_same_bits(dtype):
    """A D = 64 buffer one element off the vector alignment takes the pair-per-thread kernel:
    same bits as the wave-per-token kernel, nothing else touched."""
    import mast3r_slam_backends as mb

    tokens = M.make_inputs(B, N, 9, 64, 21, NP[dtype])
    p = torch.from_numpy(grid_pos()).to(DEV)
    outs = []
    for shift in (0, 1):
        buf = Buf(tokens, "k", shift=shift)
        assert (buf.view.data_ptr() % (4 * tokens.itemsize) != 0) == bool(shift)
        mb.rope_2d(buf.view, p, M.BASE, 1.0)
        got, untouched = buf.after()
        assert untouched
        outs.append(got)
    assert np.array_equal(bits(outs[0]), bits(outs[1]))


@pytest.mark.parametrize("name", ["d64", "d20", "far"])
def test_golden(name):
    """Kernel against the reference's outputs: the kernel's bound plus the reference's."""
    import mast3r_slam_backends as mb

    G = gold()
    tok, pos, ref = (G["g"][f"{name}_{k}"] for k in ("tokens", "pos", "ref"))
    buf = Buf(tok, "contiguous")
    mb.rope_2d(buf.view, torch.from_numpy(pos).to(DEV), float(G["g"]["base"]))
    got, untouched = buf.after()
    assert untouched
    check_model(got, tok, pos, torch.float32)
    bd = M.bound(tok, pos, G["Ta"], G["Tc"])
    assert np.all(np.abs(got.astype(np.float64) - ref) <= 2 * bd)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("H,D", [(9, 64), (2, 20)])
def test_position_zero_keeps_the_values(H, D, dtype):
    import mast3r_slam_backends as mb

    pos = grid_pos().copy()
    pos[0, 0] = 0
    pos[1] = 0
    tokens = M.make_inputs(B, N, H, D, 31, NP[dtype])
    assert np.all(tokens != 0)
    buf = Buf(tokens, "q")
    mb.rope_2d(buf.view, torch.from_numpy(pos).to(DEV), M.BASE, 1.0)
    got, untouched = buf.after()
    assert untouched
    assert np.array_equal(got[0, 0], tokens[0, 0]) and np.array_equal(got[1], tokens[1])
    # position (0, x): the y half keeps its values, the x half turns
    y0 = pos[0, :, 0] == 0
    assert np.array_equal(got[0, y0][..., :D // 2], tokens[0, y0][..., :D // 2])
    assert not np.array_equal(got[0, 1:], tokens[0, 1:])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("H,D", [(9, 64), (3, 20)])
def test_equal_heads_give_equal_bits(H, D, dtype):
    import mast3r_slam_backends as mb

    one = M.make_inputs(B, N, 1, D, 41, NP[dtype])
    tokens = np.ascontiguousarray(np.broadcast_to(one, (B, N, H, D)))
    buf = Buf(tokens, "k")
    mb.rope_2d(buf.view, torch.from_numpy(grid_pos()).to(DEV), M.BASE, 1.0)
    got, untouched = buf.after()
    assert untouched
    for h in range(1, H):
        assert np.array_equal(bits(got[:, :, h]), bits(got[:, :, 0])), h
    check_model(got, tokens, grid_pos(), dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("H,D", [(12, 64), (2, 16)])
def test_pair_equals_two_calls(H, D, dtype):
    """Cross-attention (Nq = 6, Nk = 4, qpos != kpos, two contiguous tensors) and self-attention
    (the q and k thirds of one qkv buffer, one shared pos): bit for bit two rope_2d calls."""
    import mast3r_slam_backends as mb

    qpos, kpos = grid_pos(), M.grid_positions(B, 2, 2, step=(3, 1)) + 2
    q = M.make_inputs(B, 6, H, D, 51, NP[dtype])
    k = M.make_inputs(B, 4, H, D, 52, NP[dtype])
    dq, dk = torch.from_numpy(qpos).to(DEV), torch.from_numpy(kpos).to(DEV)
    one = (Buf(q, "contiguous", seed=1), Buf(k, "contiguous", seed=2))
    two = (Buf(q, "contiguous", seed=1), Buf(k, "contiguous", seed=2))
    assert mb.rope_2d_pair(one[0].view, one[1].view, dq, dk, M.BASE, 1.0) is None
    mb.rope_2d(two[0].view, dq, M.BASE, 1.0)
    mb.rope_2d(two[1].view, dk, M.BASE, 1.0)
    for a, b, t, p in zip(one, two, (q, k), (qpos, kpos)):
        assert torch.equal(a.flat.view(torch.uint8), b.flat.view(torch.uint8))
        got, untouched = a.after()
        assert untouched
        check_model(got, t, p, dtype)

    # self-attention: both thirds of one buffer, v untouched
    a, b = Buf(q, "q", seed=3), Buf(q, "q", seed=3)
    for buf in (a, b):   # k third: other tokens
        buf.flat[PAD:-PAD].view(B, 6, 3, H, D)[:, :, 1] = torch.from_numpy(q[::-1].copy()).to(DEV)
    before = a.flat.cpu().numpy()
    va = a.flat[PAD:-PAD].view(B, 6, 3, H, D)
    vb = b.flat[PAD:-PAD].view(B, 6, 3, H, D)
    mb.rope_2d_pair(va[:, :, 0], va[:, :, 1], dq, dq, M.BASE, 1.0)
    mb.rope_2d(vb[:, :, 0], dq, M.BASE, 1.0)
    mb.rope_2d(vb[:, :, 1], dq, M.BASE, 1.0)
    assert torch.equal(a.flat.view(torch.uint8), b.flat.view(torch.uint8))
    after = a.flat.cpu().numpy()
    body = slice(PAD, -PAD)
    keep = np.ones((B, 6, 3, H, D), bool)
    keep[:, :, :2] = False
    assert np.array_equal(bits(after[body])[keep.ravel()], bits(before[body])[keep.ravel()])
    assert np.array_equal(bits(after[:PAD]), bits(before[:PAD]))
    assert np.array_equal(bits(after[-PAD:]), bits(before[-PAD:]))
    check_model(after[body].reshape(B, 6, 3, H, D)[:, :, 1], q[::-1].copy(), qpos, dtype)


@pytest.mark.parametrize("H,D", [(9, 64), (2, 20)])
def test_f0_then_minus_f0_returns_input(H, D):
    import mast3r_slam_backends as mb

    G = gold()
    tokens = M.make_inputs(B, N, H, D, 61)
    p = torch.from_numpy(grid_pos()).to(DEV)
    buf = Buf(tokens, "k")
    mb.rope_2d(buf.view, p, M.BASE, 1.0)
    mb.rope_2d(buf.view, p, M.BASE, -1.0)
    got, untouched = buf.after()
    assert untouched
    bd = M.bound(tokens, grid_pos(), G["Ta"], G["Tc"])
    assert np.all(np.abs(got.astype(np.float64) - tokens) <= 2 * bd)


def test_drop_in_module_is_the_kernel():
    import curope
    import mast3r_slam_backends as mb

    assert curope.rope_2d is mb.rope_2d


def test_module_rotates_the_view_in_place():
    """cuRoPE2D on the [B,H,N,D] view of a qkv buffer (blocks.py:97-98): the same storage comes
    back rotated; a contiguous [B,H,N,D] tensor is rejected as the reference's binding does."""
    from m3s.rope import cuRoPE2D

    H, D = 3, 64
    tokens = M.make_inputs(B, N, H, D, 71)
    p = torch.from_numpy(grid_pos()).to(DEV)
    buf = Buf(tokens, "q")
    qkv = buf.flat[PAD:-PAD].view(B, N, 3, H, D).transpose(1, 3)      # B,H,3,N,D
    q = qkv[:, :, 0]
    assert q.shape == (B, H, N, D)
    rope = cuRoPE2D(freq=M.BASE)
    with torch.no_grad():
        out = rope(q, p)
    assert out is q and out.data_ptr() == buf.view.data_ptr()
    got, untouched = buf.after()
    assert untouched
    check_model(got, tokens, grid_pos(), torch.float32)
    with pytest.raises(RuntimeError, match="tokens are not contiguous"):
        rope(torch.zeros(B, H, N, D, device=DEV), p)


def test_module_gradient():
    """d/dx sum(w * rope(x)) is w rotated by -theta."""
    from m3s.rope import cuRoPE2D

    H, D = 3, 64
    x = torch.from_numpy(M.make_inputs(B, N, H, D, 81)).to(DEV).requires_grad_(True)
    w = M.make_inputs(B, N, H, D, 82)
    p = torch.from_numpy(grid_pos()).to(DEV)
    y = cuRoPE2D(freq=M.BASE)((x * 1.0).transpose(1, 2), p)            # B,H,N,D
    (torch.from_numpy(w).to(DEV).transpose(1, 2) * y).sum().backward()
    check_model(x.grad.cpu().numpy(), w, grid_pos(), torch.float32, F0=-1.0)


def test_empty_calls_return_cleanly():
    import mast3r_slam_backends as mb

    H, D = 3, 64
    e = torch.zeros(B, 0, 3, H, D, device=DEV)
    pe = torch.zeros(B, 0, 2, dtype=torch.int64, device=DEV)
    assert mb.rope_2d(e[:, :, 0], pe, M.BASE) is None
    assert mb.rope_2d_pair(e[:, :, 0], e[:, :, 1], pe, pe, M.BASE) is None
    z = torch.zeros(0, N, H, D, device=DEV)
    assert mb.rope_2d(z, torch.zeros(0, N, 2, dtype=torch.int64, device=DEV), M.BASE) is None
    # an empty q beside a full k: k alone is rotated
    k = M.make_inputs(B, N, H, D, 91)
    p = torch.from_numpy(grid_pos()).to(DEV)
    a, b = Buf(k, "contiguous"), Buf(k, "contiguous")
    mb.rope_2d_pair(e[:, :, 0], a.view, pe, p, M.BASE)
    mb.rope_2d(b.view, p, M.BASE)
    torch.cuda.synchronize()
    assert torch.equal(a.flat, b.flat) and not torch.equal(a.view, torch.from_numpy(k).to(DEV))


def test_non_default_stream_same_bits():
    import mast3r_slam_backends as mb

    tokens = M.make_inputs(B, N, 16, 64, 95)
    p = torch.from_numpy(grid_pos()).to(DEV)
    a, b = Buf(tokens, "k"), Buf(tokens, "k")
    mb.rope_2d(a.view, p, M.BASE)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        mb.rope_2d(b.view, p, M.BASE)
    s.synchronize()
    assert torch.equal(a.flat, b.flat) and not torch.equal(a.view, torch.from_numpy(tokens).to(DEV))


# ---------------------------------------------------------------------------------
# fused forwards
# ---------------------------------------------------------------------------------

DIM, HEADS = 32, 2
HD = DIM // HEADS


def unit_rows(lin):
    """Scale a Linear's rows to L1 norm 1, so that it passes a perturbation on without growth."""
    with torch.no_grad():
        lin.weight /= lin.weight.abs().sum(dim=1, keepdim=True)
    return lin


class Rope:
    base, F0 = M.BASE, 1.0


class SelfAttn(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.num_heads, self.scale, self.rope = HEADS, HD ** -0.5, Rope()
        self.qkv = torch.nn.Linear(DIM, 3 * DIM, bias=True)
        self.proj = unit_rows(torch.nn.Linear(DIM, DIM))


class CrossAttn(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.num_heads, self.scale, self.rope = HEADS, HD ** -0.5, Rope()
        self.projq, self.projk, self.projv = (torch.nn.Linear(DIM, DIM, bias=True) for _ in range(3))
        self.proj = unit_rows(torch.nn.Linear(DIM, DIM))


def reference_tail(attn, q, k, v):
    """blocks.py:105-112 / :162-169 on rotated q, k [B,N,H,D] and v [B,N,H,D]."""
    q, k, v = (t.transpose(1, 2) for t in (q, k, v))
    a = (q @ k.transpose(-2, -1)) * attn.scale
    a = a.softmax(dim=-1)
    x = (a @ v).transpose(1, 2).reshape(q.shape[0], q.shape[2], DIM)
    return attn.proj(x)


def fused_check(attn, q, k, v, qpos, kpos, fused_out):
    """q, k, v: the unrotated projections [B,N,H,D] on the device.  The allowed distance from the
    reference expressions on rope2d_torch's q, k: the bound of the rotated q (k), summed against
    |k| (|q|) over D and scaled, is a logit perturbation e; the softmax weights then move by at
    most 2e relatively, the output by 2 e max|v| (proj has rows of L1 norm 1), plus the matmul
    rounding measured between the reference expressions on the model's q, k rounded to f32 and on
    rope2d_torch's."""
    from m3s.rope import rope2d_torch

    G = gold()
    qh, kh = q.cpu().numpy(), k.cpu().numpy()
    bq = M.bound(qh, qpos, G["Ta"], G["Tc"]).max()
    bk = M.bound(kh, kpos, G["Ta"], G["Tc"]).max()
    e = attn.scale * (bq * np.abs(kh).sum(-1).max() + bk * np.abs(qh).sum(-1).max())
    dq, dk = torch.from_numpy(qpos).to(DEV), torch.from_numpy(kpos).to(DEV)
    want = reference_tail(attn, rope2d_torch(q, dq, M.BASE), rope2d_torch(k, dk, M.BASE), v)
    model = reference_tail(attn, torch.from_numpy(M.round_to(M.model_f64(qh, qpos), np.float32)).to(DEV),
                           torch.from_numpy(M.round_to(M.model_f64(kh, kpos), np.float32)).to(DEV), v)
    rounding = float((want - model).abs().max())
    allowed = 2 * e * float(v.abs().max()) + rounding
    diff = float((fused_out - want).abs().max())
    print(f"fused - reference {diff:.2e}; allowed {allowed:.2e} (logit perturbation {e:.2e}, "
          f"matmul rounding {rounding:.2e})")
    assert diff <= allowed


def test_fused_attention_forward():
    """Measured on an MI355X: fused - reference 0 (the kernel's q and k had rope2d_torch's bits);
    allowed 6.41e-05 = logit perturbation 1.78e-05 x 2 max|v|, plus matmul rounding 2.98e-08."""
    from m3s.rope import attention_forward

    torch.manual_seed(5)
    attn = SelfAttn().to(DEV)
    x = torch.randn(B, N, DIM, device=DEV)
    with torch.no_grad():
        qkv = attn.qkv(x).reshape(B, N, 3, HEADS, HD)
        out = attention_forward(attn, x, torch.from_numpy(grid_pos()).to(DEV))
        fused_check(attn, qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], grid_pos(), grid_pos(), out)


def test_fused_cross_attention_forward():
    """Measured on an MI355X: fused - reference 0; allowed 4.21e-05 = logit perturbation 1.21e-05
    x 2 max|v|, plus matmul rounding 2.98e-08."""
    from m3s.rope import cross_attention_forward

    torch.manual_seed(6)
    attn = CrossAttn().to(DEV)
    Nk = 4
    kpos = M.grid_positions(B, 2, 2, step=(3, 1)) + 2
    query, key = torch.randn(B, N, DIM, device=DEV), torch.randn(B, Nk, DIM, device=DEV)
    value = torch.randn(B, Nk, DIM, device=DEV)
    with torch.no_grad():
        q = attn.projq(query).reshape(B, N, HEADS, HD)
        k = attn.projk(key).reshape(B, Nk, HEADS, HD)
        v = attn.projv(value).reshape(B, Nk, HEADS, HD)
        out = cross_attention_forward(attn, query, key, value, torch.from_numpy(grid_pos()).to(DEV),
                                      torch.from_numpy(kpos).to(DEV))
        fused_check(attn, q, k, v, grid_pos(), kpos, out)
