"""Generate the retrieval golden fixture from the REFERENCE Python (dev container only).

Run from the repo root:  python tests/golden/make_retrieval_golden.py
Writes tests/golden/retrieval_golden.npz.

Pinned (reference file:line): RetrievalDatabase.update, query, accumulate_scores,
quantize_custom and add_to_ivf_custom (mast3r_slam/retrieval_database.py:43-166) with the
reference's own ASMKKernel (asmk/kernel.py) and IVF (asmk/inverted_file.py), run as written on
the CPU with the parameters of mast3r/retrieval/processor.py:91-96.  The retrieval network is
replaced by the identity (prep_features), the Retriever base class and how_select_local by stubs;
the package `asmk` is entered through a stub whose __path__ is the reference's directory (its
__init__ needs faiss).  The compiled `asmk.hamming` extension cannot be built in this container:
`binarize_and_pack_2D` and `hamming_cdist_packed` below restate cython/hamming.pyx:24-30, 79-109,
128-152 in numpy, so parity with the compiled extension is not pinned.

Inputs are conditioned: every feature meets the quantise gap (tests/retrieval_model.py gap_ok) and
every aggregated component is clear of zero by more than its summation error, so neither the
top-5 sets nor the code bits depend on the f32 formulation or the BLAS backend.

The reference is read from /root/reference at generation time only; nothing under tests/
imports it at run time, and no reference source is copied.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))


# ---- numpy asmk.hamming ------------------------------------------------------------------------

def binarize_and_pack_2D(arr, threshold=0):
    arr = np.asarray(arr, dtype=np.float32)
    dim0, dim1_orig = arr.shape
    dim1 = int(np.ceil(dim1_orig / 32.0))
    result = np.zeros((dim0, dim1), dtype=np.uint32)
    for i in range(dim0):
        offset = 0
        for j in range(dim1):
            length = min(32, dim1_orig - offset)
            tmp = 0
            for b in arr[i, offset:offset + length] > threshold:
                tmp = ((tmp << 1) + int(b)) & 0xFFFFFFFF
            if j == dim1 - 1:
                tmp = (tmp << (offset + 32 - dim1_orig)) & 0xFFFFFFFF
            result[i, j] = tmp
            offset += 32
    return result


def hamming_cdist_packed(arr1, arr2, normalization=0):
    arr1 = np.asarray(arr1, dtype=np.uint32)
    arr2 = np.asarray(arr2, dtype=np.uint32)
    assert arr1.shape[1] == arr2.shape[1]
    norm = np.float32(normalization)
    if norm == 0:
        norm = np.float32(arr1.shape[1] * 32)
    result = np.zeros((arr1.shape[0], arr2.shape[0]), dtype=np.float32)
    for i in range(arr1.shape[0]):
        for j in range(arr2.shape[0]):
            s = sum(bin(int(x)).count("1") for x in arr1[i] ^ arr2[j])
            result[i, j] = np.float32(s) / norm
    return result


# ---- the fixture -------------------------------------------------------------------------------

CASES = [dict(name="a", K=500, D=128, n=37, images=10, seed=101),
         dict(name="b", K=300, D=80, n=20, images=8, seed=202)]
ALPHA, THRESH = 3.0, 0.0


def host_power_table(D):
    """The term per Hamming distance as THIS host's numpy computes it in kernel.py:62-63 and
    functional.py:13-14 (np.power on f32)."""
    nbits = 32 * ((D + 31) // 32)
    nh = np.arange(nbits + 1).astype(np.float32) / np.float32(nbits)
    sim = -2 * nh + 1
    mask = sim >= THRESH
    t = np.zeros(nbits + 1, dtype=np.float32)
    t[mask] = np.power(sim[mask], ALPHA)
    one = np.array([np.power(sim[h:h + 1], ALPHA)[0] if mask[h] else 0.0 for h in range(nbits + 1)],
                   dtype=np.float32)
    assert np.array_equal(t, one), "np.power differs between array positions on this host"
    return t


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.dirname(HERE))
    import torch

    import retrieval_model as M

    pkg = types.ModuleType("asmk")
    pkg.__path__ = [os.path.join(REF, "thirdparty", "mast3r", "asmk", "asmk")]
    sys.modules["asmk"] = pkg
    ham = types.ModuleType("asmk.hamming")
    ham.binarize_and_pack_2D = binarize_and_pack_2D
    ham.hamming_cdist_packed = hamming_cdist_packed
    sys.modules["asmk.hamming"] = ham
    pkg.hamming = ham
    for name in ("mast3r", "mast3r.retrieval"):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
    proc = types.ModuleType("mast3r.retrieval.processor")
    proc.Retriever = type("Retriever", (), {})
    sys.modules["mast3r.retrieval.processor"] = proc
    model = types.ModuleType("mast3r.retrieval.model")
    model.how_select_local = None
    sys.modules["mast3r.retrieval.model"] = model
    ms = types.ModuleType("mast3r_slam")
    ms.__path__ = [os.path.join(REF, "mast3r_slam")]
    sys.modules["mast3r_slam"] = ms
    from asmk import inverted_file, kernel
    from mast3r_slam import retrieval_database as rdb

    params = {"build_ivf": {"kernel": {"binary": True}, "ivf": {"use_idf": False},
                            "quantize": {"multiple_assignment": 1}, "aggregate": {}},
              "query_ivf": {"quantize": {"multiple_assignment": 5}, "aggregate": {},
                            "search": {"topk": None},
                            "similarity": {"similarity_threshold": THRESH, "alpha": ALPHA}}}
    out = {"cases": np.array([c["name"] for c in CASES]), "alpha": np.array(ALPHA),
           "sim_thresh": np.array(THRESH)}
    for case in CASES:
        K, D, n, N, tag = case["K"], case["D"], case["n"], case["images"], case["name"]
        rng = np.random.default_rng(case["seed"])
        cent = rng.standard_normal((K, D)).astype(np.float32)
        pool = rng.choice(K, size=60, replace=False)

        def draw():
            feat = np.zeros((n, D), dtype=np.float32)
            todo = np.arange(n)
            while len(todo):
                w = rng.choice(pool, size=len(todo))
                feat[todo] = cent[w] + np.float32(0.6) * rng.standard_normal((len(todo), D)).astype(np.float32)
                todo = todo[~M.gap_ok(feat[todo], cent, 5)]
            return feat

        db = rdb.RetrievalDatabase.__new__(rdb.RetrievalDatabase)
        codebook = types.SimpleNamespace(centroids=cent)
        db.asmk = types.SimpleNamespace(codebook=codebook, params=params)
        db.ivf_builder = types.SimpleNamespace(
            kernel=kernel.ASMKKernel(codebook, **params["build_ivf"]["kernel"]),
            ivf=inverted_file.IVF.initialize_empty(codebook_size=K, **params["build_ivf"]["ivf"]),
            step_params=params["build_ivf"])
        db.kf_counter, db.kf_ids = 0, []
        db.query_dtype, db.query_device = torch.float32, "cpu"
        db.centroids = torch.from_numpy(cent)
        db.prep_features = lambda f: f

        rec = {}
        kern = db.ivf_builder.kernel
        agg0 = kern.aggregate_image

        def aggregate_image(des, word_ids, **kw):
            ades, ids = agg0(des, word_ids, **kw)
            rec.setdefault("agg", []).append((np.array(ades), np.array(ids), np.array(word_ids)))
            return ades, ids

        kern.aggregate_image = aggregate_image
        query0 = db.query

        def query(feat, id):
            ranks, ranked, topk = query0(feat, id)
            sc = np.empty_like(ranked)
            sc[np.arange(ranked.shape[0])[:, None], ranks] = ranked
            rec["scores"], rec["ids"] = sc[0].copy(), np.array(topk)
            return ranks, ranked, topk

        db.query = query

        table = host_power_table(D)
        lib_rule = M.term_table(D, ALPHA, THRESH)
        out[f"{tag}_centroids"] = cent
        out[f"{tag}_table"] = table
        out[f"{tag}_table_equals_rule"] = np.array(bool(np.array_equal(table, lib_rule)))
        print(f"case {tag}: {32 * ((D + 31) // 32)}-bit codes, host np.power table == library rule: "
              f"{np.array_equal(table, lib_rule)} ({int((table != lib_rule).sum())} of "
              f"{int((table > 0).sum())} positive entries differ)")

        feats = [draw() for _ in range(N)]
        calls = [(feats[i], True) for i in range(N - 1)] + [(feats[N - 1], False), (feats[N - 1], True)]
        model_db = M.ModelDatabase(cent, table=table)
        for c, (feat, add) in enumerate(calls):
            rec.clear()
            frame = types.SimpleNamespace(feat=torch.from_numpy(feat)[None])
            ret = db.update(frame, add, 3, 0.0)
            assert ret == model_db.update(feat, add, 3, 0.0), (tag, c)
            queried = "scores" in rec
            out[f"{tag}_c{c}_feat"] = feat
            out[f"{tag}_c{c}_add"] = np.array(add)
            out[f"{tag}_c{c}_ret"] = np.array(ret, dtype=np.int64)
            out[f"{tag}_c{c}_queried"] = np.array(queried)
            if queried:
                ades, words, ids = rec["agg"][0]
                assert np.array_equal(ids, rec["ids"])
                out[f"{tag}_c{c}_ids"] = rec["ids"].astype(np.int64)
                out[f"{tag}_c{c}_qwords"] = words.astype(np.int64)
                out[f"{tag}_c{c}_qcodes"] = ades.astype(np.uint32)
                out[f"{tag}_c{c}_scores"] = rec["scores"].astype(np.float64)
                assert np.array_equal(rec["scores"], model_db.last["scores"]), (tag, c)
            else:
                out[f"{tag}_c{c}_ids"] = rec["agg"][0][2].astype(np.int64)  # the add's ma = 1 ids
            # sign condition of every aggregation this call made
            for ades, words, ids in rec["agg"]:
                _, sums, tmax, cnt = M.aggregate_sums(feat, cent, ids)
                assert np.array_equal(M.pack_bits(sums > 0), ades)
                assert (np.abs(sums) > cnt[:, None] * 2.0 ** -22 * tmax).all(), (tag, c)
        ivf = db.ivf_builder.ivf
        assert ivf.n_images == N and db.kf_counter == N
        for m in range(N):
            ws = [w for w in range(K) if ivf.ivf_image_ids[w] is not None
                  and m in ivf.ivf_image_ids[w][:ivf.counts[w]]]
            cs = [ivf.ivf_vecs[w][list(ivf.ivf_image_ids[w][:ivf.counts[w]]).index(m)] for w in ws]
            assert len(ws) == int(ivf.norm_factor[m])
            out[f"{tag}_store{m}_words"] = np.array(ws, dtype=np.int64)
            out[f"{tag}_store{m}_codes"] = np.array(cs, dtype=np.uint32).reshape(len(ws), -1)
        out[f"{tag}_ncalls"] = np.array(len(calls))
        out[f"{tag}_nimages"] = np.array(N)
    # the table comparison for the flagship code width as well (no fixture case uses it)
    t1024 = host_power_table(1024)
    print("1024-bit codes: host np.power table == library rule:",
          np.array_equal(t1024, M.term_table(1024, ALPHA, THRESH)))
    path = os.path.join(HERE, "retrieval_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
