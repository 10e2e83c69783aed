"""RoPE2D on the host: the reference's outputs (tests/golden/rope_golden.npz) against the f64
model (tests/rope_model.py) inside the derived bound, ``m3s.rope.rope2d_torch`` against both, and
the rotation by F0 undone by -F0.  No GPU."""
import functools
import os

import numpy as np
import pytest
import torch

import rope_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ("d64", "d20", "far")


@functools.lru_cache(maxsize=None)
def gold():
    g = np.load(os.path.join(HERE, "golden", "rope_golden.npz"))
    return dict(g=g, Ta=M.tol(g["Ta"]), Tc=M.tol(g["Tc"]))


def case(name):
    g = gold()["g"]
    return g[f"{name}_tokens"], g[f"{name}_pos"], g[f"{name}_ref"]


def test_fixture_terms():
    G = gold()
    assert float(G["g"]["base"]) == M.BASE
    assert 0 < float(G["g"]["Ta"]) < 8 and 0 < float(G["g"]["Tc"]) < 4   # a few u, as f32 gives
    assert G["Ta"] >= 2 and G["Tc"] >= 2


@pytest.mark.parametrize("name", CASES)
def test_golden_within_bound_of_model(name):
    G = gold()
    tok, pos, ref = case(name)
    assert tok.dtype == np.float32 and pos.dtype == np.int64 and ref.shape == tok.shape
    err = np.abs(ref.astype(np.float64) - M.model_f64(tok, pos))
    bd = M.bound(tok, pos, G["Ta"], G["Tc"])
    print(f"{name}: reference within {err.max():.2e} of the f64 model, err/bound {np.max(err / bd):.3f}")
    assert np.all(err <= bd)
    # an indexing mistake is O(1): the bound is nowhere near it
    assert bd.max() < 1e-4 and np.abs(ref - tok).max() > 0.1


@pytest.mark.parametrize("name", CASES)
def test_rope2d_torch_against_model_and_golden(name):
    from m3s.rope import rope2d_torch

    G = gold()
    tok, pos, ref = case(name)
    got = rope2d_torch(torch.from_numpy(tok), torch.from_numpy(pos), M.BASE).numpy()
    assert got.dtype == np.float32 and got.shape == tok.shape
    bd = M.bound(tok, pos, G["Ta"], G["Tc"])
    assert np.all(np.abs(got.astype(np.float64) - M.model_f64(tok, pos)) <= bd)
    assert np.all(np.abs(got.astype(np.float64) - ref) <= 2 * bd)


def test_rope2d_torch_f16_and_wild_positions():
    """f16 tokens and positions no table could hold (negative, 200): the model only."""
    from m3s.rope import rope2d_torch

    G = gold()
    tok = M.make_inputs(2, 6, 2, 12, 3, np.float16)
    pos = M.wild_positions(2, 6, 4)
    got = rope2d_torch(torch.from_numpy(tok), torch.from_numpy(pos), M.BASE, 1.0).numpy()
    assert got.dtype == np.float16
    m64 = M.model_f64(tok, pos)
    bd = M.bound(tok, pos, G["Ta"], G["Tc"], dtype=np.float16, model=m64)
    assert np.all(np.abs(got.astype(np.float64) - m64) <= bd)


@pytest.mark.parametrize("name", CASES)
def test_f0_then_minus_f0_returns_input(name):
    from m3s.rope import rope2d_torch

    G = gold()
    tok, pos, _ = case(name)
    p = torch.from_numpy(pos)
    fwd = rope2d_torch(torch.from_numpy(tok), p, M.BASE, 1.0)
    back = rope2d_torch(fwd, p, M.BASE, -1.0).numpy()
    bd = M.bound(tok, pos, G["Ta"], G["Tc"])
    assert np.all(np.abs(back.astype(np.float64) - tok) <= 2 * bd)
    assert np.array_equal(M.model_f64(tok, pos, F0=-1.0), M.model_f64(tok, -pos))
