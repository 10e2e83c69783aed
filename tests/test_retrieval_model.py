"""The host model of the retrieval update (tests/retrieval_model.py) against the fixture the
reference's own RetrievalDatabase produced (tests/golden/make_retrieval_golden.py): ids, codes,
scores bitwise with the stored term table, returned lists; and the conditions the fixture's and
the GPU tests' inputs must meet.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest

import retrieval_model as M

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "retrieval_golden.npz"))


def calls(gold, tag):
    for c in range(int(gold[f"{tag}_ncalls"])):
        yield c, gold[f"{tag}_c{c}_feat"], bool(gold[f"{tag}_c{c}_add"]), bool(gold[f"{tag}_c{c}_queried"])


@pytest.mark.parametrize("tag", ["a", "b"])
def test_model_reproduces_the_reference_sequence(gold, tag):
    cent = gold[f"{tag}_centroids"]
    db = M.ModelDatabase(cent, table=gold[f"{tag}_table"])
    for c, feat, add, queried in calls(gold, tag):
        ret = db.update(feat, add, 3, 0.0)
        assert ret == gold[f"{tag}_c{c}_ret"].tolist(), c
        assert queried == (c > 0)
        if queried:
            assert np.array_equal(db.last["ids"], gold[f"{tag}_c{c}_ids"]), c
            assert np.array_equal(db.last["words"], gold[f"{tag}_c{c}_qwords"]), c
            assert np.array_equal(db.last["codes"], gold[f"{tag}_c{c}_qcodes"]), c
            assert np.array_equal(db.last["scores"], gold[f"{tag}_c{c}_scores"]), c  # f64 bitwise
        else:
            assert np.array_equal(M.quantize(feat, cent, 1), gold[f"{tag}_c{c}_ids"]), c
    assert len(db.store) == int(gold[f"{tag}_nimages"])
    for m, (words, codes) in enumerate(db.store):
        assert np.array_equal(words, gold[f"{tag}_store{m}_words"]), m
        assert np.array_equal(codes, gold[f"{tag}_store{m}_codes"]), m


@pytest.mark.parametrize("tag", ["a", "b"])
def test_fixture_inputs_are_conditioned(gold, tag):
    cent = gold[f"{tag}_centroids"]
    for c, feat, add, queried in calls(gold, tag):
        assert M.gap_ok(feat, cent, 5).all(), c
        for ma in (1, 5):
            _, sums, tmax, cnt = M.aggregate_sums(feat, cent, M.quantize(feat, cent, ma))
            assert (np.abs(sums) > cnt[:, None] * 2.0 ** -22 * tmax).all(), (c, ma)


def test_fixture_has_a_short_last_code_word(gold):
    assert gold["b_centroids"].shape[1] == 80
    codes = gold["b_c1_qcodes"]
    assert codes.shape[1] == 3 and not (codes[:, 2] & 0xFFFF).any() and (codes[:, 2] >> 16).any()


@pytest.mark.parametrize("tag", ["a", "b"])
def test_term_table_rule_against_the_host_table(gold, tag, backend):
    D = gold[f"{tag}_centroids"].shape[1]
    rule = M.term_table(D, float(gold["alpha"]), float(gold["sim_thresh"]))
    host = gold[f"{tag}_table"]
    # the library builds its table by the same rule
    assert np.array_equal(backend.retrieval_term_table(D, float(gold["alpha"]), float(gold["sim_thresh"])), rule)
    if bool(gold[f"{tag}_table_equals_rule"]):
        assert np.array_equal(rule, host)
    else:  # np.power of the generating host is within 1 ulp of the rule
        ulp = np.spacing(np.maximum(rule, host))
        assert (np.abs(rule.astype(np.float64) - host) <= ulp).all()
    assert bool(gold["a_table_equals_rule"]) and not bool(gold["b_table_equals_rule"])


def test_hamming_restatement_known_answers():
    spec = importlib.util.spec_from_file_location(
        "make_retrieval_golden", os.path.join(HERE, "golden", "make_retrieval_golden.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    # the docstring example of hamming_cdist_packed (cython/hamming.pyx)
    d = g.hamming_cdist_packed(np.array([[3], [1]], dtype=np.uint32), np.array([[1], [2]], dtype=np.uint32), 2)
    assert d.dtype == np.float32 and np.array_equal(d, np.array([[0.5, 0.5], [0.0, 1.0]], dtype=np.float32))
    x = np.zeros((1, 40), dtype=np.float32)
    x[0, [0, 31, 32, 39]] = 1.0
    x[0, 5] = np.nan
    assert g.binarize_and_pack_2D(x).tolist() == [[0x80000001, 0x81000000]]
    assert np.array_equal(M.pack_bits(x > 0), g.binarize_and_pack_2D(x))


def test_model_tie_rule_and_popcount():
    cent = np.array([[0.0, 1.0], [2.0, 0.0], [0.0, 1.0], [5.0, 5.0]], dtype=np.float32)
    ids = M.quantize(np.array([[0.0, 1.0]], dtype=np.float32), cent, 3)
    assert ids.tolist() == [[0, 2, 1]]
    assert M.popcount32(np.array([0, 1, 0xFFFFFFFF, 0x80000001], dtype=np.uint32)).tolist() == [0, 1, 32, 2]


@pytest.mark.parametrize("n,K,D", [(1, 5, 1), (33, 1000, 50), (300, 4099, 128), (33, 4099, 1), (1, 1000, 1024)])
def test_conditioned_inputs_meet_the_gap(n, K, D):
    """The generator of the GPU tests' inputs: every feature meets the gap (cap zero)."""
    cent, feat = M.conditioned_inputs(1000 * n + K + D, n, K, D)
    assert cent.shape == (K, D) and feat.shape == (n, D)
    assert M.gap_ok(feat, cent, min(5, K - 1)).all()
    # and the model's f32 expansion (the reference's formulation) picks the same ids
    q, c = feat.astype(np.float32), cent.astype(np.float32)
    d32 = ((q * q).sum(1)[:, None] + (c * c).sum(1)[None, :]) - np.float32(2) * (q @ c.T)
    ma = min(5, K)
    assert np.array_equal(np.argsort(d32, axis=1, kind="stable")[:, :ma], M.quantize(feat, cent, ma))
