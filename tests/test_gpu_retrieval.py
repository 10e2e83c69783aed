"""On-device retrieval (csrc/retrieval.hip, m3s/retrieval_database.py) stage by stage against the
fixture of the reference's own RetrievalDatabase, and against the host model
(tests/retrieval_model.py) at the shapes where the tiling can go wrong."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import retrieval_model as M

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda"


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "retrieval_golden.npz"))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def agg_np(words, codes, count):
    k = int(count.item())
    return words[:k].cpu().numpy(), u32(codes[:k])


@functools.lru_cache(maxsize=None)
def conditioned(n, K, D):
    cent, feat = M.conditioned_inputs(1000 * n + K + D, n, K, D)
    ma = min(5, K)
    ids = M.quantize(feat, cent, ma)
    for a in (cent, feat, ids):
        a.setflags(write=False)
    return cent, feat, ids


def gold_calls(gold, tag):
    for c in range(int(gold[f"{tag}_ncalls"])):
        yield c, gold[f"{tag}_c{c}_feat"], bool(gold[f"{tag}_c{c}_add"]), bool(gold[f"{tag}_c{c}_queried"])


# ---- stage by stage against the fixture --------------------------------------------------------


@pytest.mark.parametrize("tag", ["a", "b"])
def test_quantize_and_aggregate_match_the_fixture(backend, gold, tag):
    cent = dev(gold[f"{tag}_centroids"])
    db = backend.retrieval_create(cent, max_feat=64)
    for c, feat, add, queried in gold_calls(gold, tag):
        f = dev(feat)
        ids5 = backend.retrieval_quantize(db, f, 5)
        ids1 = backend.retrieval_quantize(db, f, 1)
        ref = gold[f"{tag}_c{c}_ids"]
        assert np.array_equal(ids1.cpu().numpy(), ref[:, :1]), c
        assert np.array_equal(ids5.cpu().numpy()[:, :1], ref[:, :1]), c
        if queried:
            assert np.array_equal(ids5.cpu().numpy(), ref), c
            words, codes = agg_np(*backend.retrieval_aggregate(db, f, dev(ref.astype(np.int32))))
            assert np.array_equal(words, gold[f"{tag}_c{c}_qwords"]), c
            assert np.array_equal(codes, gold[f"{tag}_c{c}_qcodes"]), c
    db.close()


@pytest.mark.parametrize("tag", ["a", "b"])
def test_update_sequence_matches_the_fixture(gold, tag):
    """With the generating host's term table: scores bitwise (f64), lists equal, the store equal."""
    from m3s.retrieval_database import RetrievalDatabase

    rd = RetrievalDatabase(gold[f"{tag}_centroids"], device=DEV, max_feat=64, table=gold[f"{tag}_table"])
    for c, feat, add, queried in gold_calls(gold, tag):
        f = dev(feat)
        if queried:
            sc = rd.query(f).cpu().numpy()
            print(tag, c, "max |score - ref|", np.abs(sc - gold[f"{tag}_c{c}_scores"]).max())
            assert np.array_equal(sc, gold[f"{tag}_c{c}_scores"]), c
        size = len(rd)
        ret = rd.update(f[None], add, 3, 0.0)  # [1,n,D] like the reference's features
        assert ret == gold[f"{tag}_c{c}_ret"].tolist(), c
        assert len(rd) == size + int(add)
    assert rd.kf_counter == int(gold[f"{tag}_nimages"]) and rd.kf_ids == list(range(rd.kf_counter))
    for m in range(rd.kf_counter):
        words, codes = rd.stored_image(m)
        assert np.array_equal(words.cpu().numpy(), gold[f"{tag}_store{m}_words"]), m
        assert np.array_equal(u32(codes), gold[f"{tag}_store{m}_codes"]), m
    rd.close()


@pytest.mark.parametrize("tag", ["a", "b"])
def test_scores_with_the_library_table(gold, tag):
    """The library's own table: bitwise where the generator found the tables equal (128-bit
    codes), else within 2^-23 of the score (every term within 1 ulp of f32, all non-negative)."""
    from m3s.retrieval_database import RetrievalDatabase

    rd = RetrievalDatabase(gold[f"{tag}_centroids"], device=DEV, max_feat=64)
    for c, feat, add, queried in gold_calls(gold, tag):
        f = dev(feat)
        if queried:
            sc = rd.query(f).cpu().numpy()
            ref = gold[f"{tag}_c{c}_scores"]
            print(tag, c, "max rel", (np.abs(sc - ref) / np.maximum(ref, 1e-300)).max())
            if bool(gold[f"{tag}_table_equals_rule"]):
                assert np.array_equal(sc, ref), c
            else:
                assert (np.abs(sc - ref) <= 2.0 ** -23 * ref).all(), c
        rd.update(f, add, 3, 0.0)
    rd.close()


# ---- against the model at the tiling's edge shapes ---------------------------------------------


@pytest.mark.parametrize("D", [1, 50, 128, 1024])
@pytest.mark.parametrize("K", [5, 1000, 4099])
@pytest.mark.parametrize("n", [1, 33, 300])
def test_quantize_and_aggregate_match_the_model(backend, n, K, D):
    cent, feat, ids = conditioned(n, K, D)
    ma = ids.shape[1]
    db = backend.retrieval_create(dev(cent), max_feat=300)
    f = dev(feat)
    got = backend.retrieval_quantize(db, f, ma).cpu().numpy()
    bad = np.nonzero((got != ids).any(axis=1))[0]
    print(f"n={n} K={K} D={D}: {len(bad)} of {n} features differ from the exact nearest-{ma}")
    assert len(bad) == 0, bad[:8]
    assert np.array_equal(backend.retrieval_quantize(db, f, 1).cpu().numpy(), ids[:, :1])
    for m in (1, ma):
        words, codes = agg_np(*backend.retrieval_aggregate(db, f, dev(ids[:, :m].astype(np.int32))))
        w_ref, c_ref = M.aggregate(feat, cent, ids[:, :m])
        assert np.array_equal(words, w_ref), m
        assert np.array_equal(codes, c_ref), m
    db.close()


def test_update_matches_the_model_across_several_tiles(backend):
    """A whole sequence at K = 4099, D = 50 (scalar loads, ragged tiles, the merge)."""
    from m3s.retrieval_database import RetrievalDatabase

    cent, _, _ = conditioned(33, 4099, 50)
    rd = RetrievalDatabase(cent, device=DEV, max_feat=40)
    model = M.ModelDatabase(cent)
    rng = np.random.default_rng(5)
    for c in range(5):
        feat = M.conditioned_features(rng, cent, 33 + c)
        f = dev(feat)
        if c:
            want = model.query(feat)
            assert np.array_equal(rd.query(f).cpu().numpy(), want), c
        assert rd.update(f, True, 3, 0.0) == model.update(feat, True, 3, 0.0), c
    rd.close()


# ---- tie rule, exact integers ------------------------------------------------------------------


def test_duplicate_centroids_resolve_to_the_lower_index(backend):
    rng = np.random.default_rng(11)
    K, D = 4099, 16
    cent = rng.standard_normal((K, D)).astype(np.float32)
    pairs = [(10, 3000), (200, 4098), (127, 128), (5, 130), (40, 41), (2500, 2501)]
    for lo, hi in pairs:
        cent[hi] = cent[lo]
    feat = np.stack([cent[lo] + np.float32(0.01) * rng.standard_normal(D).astype(np.float32)
                     for lo, _ in pairs for _ in range(7)])
    d = np.sort(M.exact_distances(feat, cent), axis=1)  # the pair ties, the third is far
    assert (d[:, 1] - d[:, 0] < 1e-9).all() and (d[:, 2] - d[:, 1] > M.gap_bound(feat, cent)).all()
    want = np.repeat(np.array(pairs), 7, axis=0)
    db = backend.retrieval_create(dev(cent), max_feat=64)
    f = dev(feat)
    first = backend.retrieval_quantize(db, f, 2).cpu().numpy()
    assert np.array_equal(first, want)
    assert np.array_equal(backend.retrieval_quantize(db, f, 1).cpu().numpy(), want[:, :1])
    for _ in range(3):
        assert np.array_equal(backend.retrieval_quantize(db, f, 2).cpu().numpy(), first)
    db.close()


@pytest.mark.parametrize("n,K,D", [(70, 300, 8), (130, 200, 3)])
def test_exact_integer_distances(backend, n, K, D):
    """Small integers: every product, sum and distance is exact in f32, so the ids are the integer
    argmin with ties by index -- a wrong A/B lane map or a transposed C/D map cannot pass (the
    feature matrix is not symmetric in any sense: n != K, random)."""
    rng = np.random.default_rng(3)
    cent = rng.integers(-3, 4, size=(K, D))
    feat = rng.integers(-3, 4, size=(n, D))
    feat[:, 0] += np.arange(n) % 5  # rows differ from one another systematically
    dist = ((feat[:, None, :] - cent[None, :, :]) ** 2).sum(-1)
    want = np.argsort(dist, axis=1, kind="stable")[:, :5]
    db = backend.retrieval_create(dev(cent.astype(np.float32)), max_feat=n)
    got = backend.retrieval_quantize(db, dev(feat.astype(np.float32)), 5).cpu().numpy()
    assert np.array_equal(got, want)
    db.close()


# ---- repeatability, growth, edge cases, errors -------------------------------------------------


def run_sequence(gold, tag, images, max_feat=64):
    from m3s.retrieval_database import RetrievalDatabase

    rd = RetrievalDatabase(gold[f"{tag}_centroids"], device=DEV, max_feat=max_feat)
    feats = [gold[f"{tag}_c{c}_feat"] for c in range(int(gold[f"{tag}_ncalls"]) - 1)]
    out = []
    for i in range(images):
        f = dev(feats[i % len(feats)][: 20 + (i % 3)])
        if i:
            out.append(rd.query(f).cpu().numpy())
        rd.update(f, True, 3, 0.0)
    return rd, out


def test_replay_is_bitwise_repeatable(gold):
    rd1, s1 = run_sequence(gold, "a", 8)
    rd2, s2 = run_sequence(gold, "a", 8)
    assert len(s1) == 7 and all(np.array_equal(a, b) for a, b in zip(s1, s2))
    rd1.close()
    rd2.close()


def test_growth_past_the_initial_capacity_keeps_earlier_scores(gold):
    rd, _ = run_sequence(gold, "a", 14)
    q = dev(gold["a_c3_feat"])
    before = rd.query(q).cpu().numpy()
    for i in range(14, 40):  # the store starts at 16 images and doubles
        rd.update(dev(gold[f"a_c{i % 9}_feat"]), True, 3, 0.0)
    after = rd.query(q).cpu().numpy()
    assert len(rd) == 40 and after.shape == (40,)
    assert np.array_equal(after[:14], before)
    w0, c0 = rd.stored_image(0)
    assert np.array_equal(w0.cpu().numpy(), M.aggregate(gold["a_c0_feat"][:20], gold["a_centroids"],
                                                        M.quantize(gold["a_c0_feat"][:20], gold["a_centroids"], 1))[0])
    rd.close()


def test_edge_cases(gold):
    from m3s.retrieval_database import RetrievalDatabase

    rng = np.random.default_rng(9)
    K, D = 500, 128
    cent = rng.standard_normal((K, D)).astype(np.float32)
    cent[:250] += 10.0  # two far clusters: the nearest five stay inside one
    cent[250:] -= 10.0
    near = lambda ws: (cent[ws] + np.float32(0.3) * rng.standard_normal((len(ws), D)).astype(np.float32))
    rd = RetrievalDatabase(cent, device=DEV, max_feat=32)
    fa = dev(near(rng.choice(250, 30)))
    assert rd.update(fa, True, 3, 0.0) == [] and len(rd) == 1  # empty database
    assert rd.update(fa, False, 3, 0.0) == [0] and len(rd) == 1  # add_after_query=False
    assert rd.update(fa, True, 10, 0.0) == [0] and len(rd) == 2  # k larger than the database
    sc = rd.query(fa).cpu().numpy()
    assert sc.shape == (2,) and (sc > 0).all()
    assert rd.update(fa, False, 3, float(sc.max()) * 2) == []  # min_thresh above every score
    fb = dev(near(250 + rng.choice(250, 30)))  # the other cluster: no shared word
    sb = rd.query(fb).cpu().numpy()
    assert np.array_equal(sb, np.zeros(2)) and rd.update(fb, False, 3, 0.0) == []
    assert len(rd) == 2
    rd.close()


def test_errors(backend, gold):
    cent = dev(gold["b_centroids"])
    db = backend.retrieval_create(cent, max_feat=20)
    good = dev(gold["b_c0_feat"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        backend.retrieval_query(db, good.cpu())
    with pytest.raises(RuntimeError, match="feat has D = 128"):
        backend.retrieval_query(db, torch.zeros(4, 128, device=DEV))
    with pytest.raises(RuntimeError, match="outside 1..max_feat = 20"):
        backend.retrieval_add(db, torch.zeros(21, 80, device=DEV))
    with pytest.raises(RuntimeError, match="needs a preceding query"):
        backend.retrieval_add(db, good, reuse_last_query=True)
    with pytest.raises(RuntimeError, match="image 0 outside"):
        backend.retrieval_image(db, 0)
    # the C ABI itself: a host pointer and n > max_feat are M3S_ERR_INVALID
    lib = backend.lib
    host = np.zeros((4, 80), dtype=np.float32)
    ids = torch.zeros(4, 1, dtype=torch.int32, device=DEV)
    rc = lib.m3s_retrieval_quantize(db.ptr, host.ctypes.data, 4, 1, ctypes.c_void_p(ids.data_ptr()), None)
    assert rc == 1 and b"not a device pointer" in lib.m3s_last_error()
    rc = lib.m3s_retrieval_add(db.ptr, ctypes.c_void_p(good.data_ptr()), 21, 0, None)
    assert rc == 1 and b"max_feat" in lib.m3s_last_error()
    out = ctypes.c_void_p()
    rc = lib.m3s_retrieval_create(host.ctypes.data, 4, 80, 1, 1, 3.0, 0.0, None, 20, ctypes.byref(out))
    assert rc == 1 and b"not a device pointer" in lib.m3s_last_error()
    assert backend.retrieval_size(db) == 0
    backend.retrieval_add(db, good)  # still usable after the errors
    assert backend.retrieval_size(db) == 1
    db.close()
