"""Host model of the retrieval update (numpy), restated from its specification.

One ``update(feat, add_after_query, k, min_thresh)`` of the reference's RetrievalDatabase
(mast3r_slam/retrieval_database.py:43-166 with the ASMK binary kernel, no idf):

 1. quantise   the ``ma`` centroids of least squared L2 distance per feature, ascending, ties by
               the lower index.  Distances here are exact (f64 of the f32 inputs); the device and
               the reference form |q|^2 + |c|^2 - 2 q.c in f32, whose error ``gap_bound`` covers.
 2. aggregate  per unique word the f32 sum of (des[f] - centroid[w]) over ascending f, binarised
               with > 0 and packed MSB first into ceil(D/32) uint32.
 3. score      per stored image and shared word: h = popcount(xor), term = f32(f64(T[h]) /
               sqrt(f64(n_words))) summed in f64 in ascending word order, divided by
               f64(sqrtf(f32(|U|))).
 4. pick       torch.topk on the scores, keep those > min_thresh.
 5. add        the nearest word of each feature, aggregated as in 2.

Test infrastructure only (after tests/pcg_model.py).
"""
from __future__ import annotations

import numpy as np


def exact_distances(feat, cent):
    """[n,K] f64 squared distances of the f32 inputs: the expansion in f64, whose rounding
    (about D 2^-52 (|q| + |c|)^2) is nine orders below gap_bound."""
    q = np.asarray(feat, dtype=np.float64)
    c = np.asarray(cent, dtype=np.float64)
    return (q * q).sum(1)[:, None] + (c * c).sum(1)[None, :] - 2.0 * (q @ c.T)


def quantize(feat, cent, ma):
    """ids [n,ma] int64 of the exact nearest centroids, ascending distance, ties by lower index."""
    d = exact_distances(feat, cent)
    return np.argsort(d, axis=1, kind="stable")[:, :ma]


def gap_bound(feat, cent):
    """[n] the distance gap above which the f32 expansion cannot reorder two centroids:
    4 (D+4) 2^-24 (|q| + max|c|)^2."""
    q = np.asarray(feat, dtype=np.float64)
    c = np.asarray(cent, dtype=np.float64)
    D = q.shape[1]
    qn = np.sqrt((q * q).sum(1))
    cmax = np.sqrt((c * c).sum(1)).max()
    return 4.0 * (D + 4) * 2.0 ** -24 * (qn + cmax) ** 2


def gap_ok(feat, cent, ma):
    """[n] bool: consecutive exact distances among the first ma+1 differ by more than gap_bound."""
    d = np.sort(exact_distances(feat, cent), axis=1)[:, : ma + 1]
    if d.shape[1] < 2:
        return np.ones(d.shape[0], dtype=bool)
    return (np.diff(d, axis=1) > gap_bound(feat, cent)[:, None]).all(axis=1)


def pack_bits(bits):
    """[m,D] bool -> [m,ceil(D/32)] uint32, component 32j+i at bit 31-i of word j."""
    bits = np.asarray(bits, dtype=bool)
    m, D = bits.shape
    W = (D + 31) // 32
    pad = np.zeros((m, 32 * W), dtype=np.uint64)
    pad[:, :D] = bits
    w = (pad.reshape(m, W, 32) << np.arange(31, -1, -1, dtype=np.uint64)).sum(-1)
    return w.astype(np.uint32)


def aggregate_sums(feat, cent, ids):
    """words [U] int64 ascending, sums [U,D] f32 (sequential over ascending feature), and the
    largest |term| and term count per component ([U,D] f32, [U] int)."""
    feat = np.asarray(feat, dtype=np.float32)
    cent = np.asarray(cent, dtype=np.float32)
    ids = np.asarray(ids)
    words = np.unique(ids)
    sums = np.zeros((len(words), feat.shape[1]), dtype=np.float32)
    tmax = np.zeros_like(sums)
    cnt = np.zeros(len(words), dtype=np.int64)
    for u, w in enumerate(words):
        fs = np.nonzero((ids == w).any(axis=1))[0]
        acc = None
        for f in fs:
            r = (feat[f] - cent[w]).astype(np.float32)
            acc = r if acc is None else (acc + r).astype(np.float32)
            tmax[u] = np.maximum(tmax[u], np.abs(r))
        sums[u] = acc
        cnt[u] = len(fs)
    return words.astype(np.int64), sums, tmax, cnt


def aggregate(feat, cent, ids):
    """-> words [U] int64 ascending, codes [U,W] uint32."""
    words, sums, _, _ = aggregate_sums(feat, cent, ids)
    return words, pack_bits(sums > 0)


def term_table(D, alpha, sim_thresh):
    """T[h], h = 0..32W: the f32 steps to sim, then the f32 rounding of the f64 power."""
    nbits = 32 * ((D + 31) // 32)
    h = np.arange(nbits + 1)
    nh = h.astype(np.float32) / np.float32(nbits)
    sim = (np.float32(-2.0) * nh).astype(np.float32) + np.float32(1.0)
    keep = sim >= np.float32(sim_thresh)
    t = np.power(sim.astype(np.float64), float(alpha)).astype(np.float32)
    return np.where(keep, t, np.float32(0.0)).astype(np.float32)


_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)


def popcount32(x):
    x = np.asarray(x, dtype=np.uint32)
    return (_POP8[x & 0xFF] + _POP8[(x >> 8) & 0xFF] + _POP8[(x >> 16) & 0xFF] + _POP8[x >> 24])


def scores(q_words, q_codes, store, table):
    """store: list of (words, codes) per image -> [n_images] f64."""
    out = np.zeros(len(store), dtype=np.float64)
    q_words = np.asarray(q_words)
    for m, (words, codes) in enumerate(store):
        norm = np.sqrt(np.float64(len(words)))
        s = np.float64(0.0)
        for u, w in enumerate(q_words):  # ascending
            i = np.searchsorted(words, w)
            if i < len(words) and words[i] == w:
                h = int(popcount32(q_codes[u] ^ codes[i]).sum())
                s = s + np.float64(np.float32(np.float64(table[h]) / norm))
        out[m] = s / np.float64(np.sqrt(np.float32(len(q_words))))
    return out


def pick(sc, k, min_thresh):
    import torch

    if len(sc) == 0:
        return []
    top = torch.topk(torch.from_numpy(np.asarray(sc, dtype=np.float64)), min(int(k), len(sc)))
    return top.indices[top.values > min_thresh].tolist()


class ModelDatabase:
    def __init__(self, cent, ma_build=1, ma_query=5, alpha=3.0, sim_thresh=0.0, table=None):
        self.cent = np.asarray(cent, dtype=np.float32)
        self.ma_build, self.ma_query = ma_build, ma_query
        D = self.cent.shape[1]
        self.table = term_table(D, alpha, sim_thresh) if table is None else np.asarray(table, np.float32)
        self.store = []
        self.last = None

    def query(self, feat):
        ids = quantize(feat, self.cent, self.ma_query)
        words, codes = aggregate(feat, self.cent, ids)
        sc = scores(words, codes, self.store, self.table)
        self.last = dict(ids=ids, words=words, codes=codes, scores=sc)
        return sc

    def update(self, feat, add_after_query, k, min_thresh=0.0):
        out, ids = [], None
        if self.store:
            out = pick(self.query(feat), k, min_thresh)
            ids = self.last["ids"][:, : self.ma_build]
        if add_after_query:
            if ids is None:
                ids = quantize(feat, self.cent, self.ma_build)
            self.store.append(aggregate(feat, self.cent, ids))
        return out


def conditioned_features(rng, cent, n, ma=5, pool=60, noise=0.6):
    """feat [n,D] f32 with EVERY feature meeting gap_ok against ``cent`` for ``ma`` (and so for
    every smaller ma): centroid + noise with the words drawn from a pool (so that images share
    words), resampled until they pass."""
    K, D = cent.shape
    pool_ids = rng.choice(K, size=min(pool, K), replace=False)
    feat = np.zeros((n, D), dtype=np.float32)
    todo = np.arange(n)
    mm = min(ma, K - 1)
    for r in range(400):
        if r < 20:
            w = rng.choice(pool_ids, size=len(todo))
            feat[todo] = cent[w] + np.float32(noise) * rng.standard_normal((len(todo), D)).astype(np.float32)
        else:  # low D with many centroids: only the sparse tails separate the nearest few
            feat[todo] = (3.0 * rng.standard_normal((len(todo), D))).astype(np.float32)
        todo = todo[~gap_ok(feat[todo], cent, mm)]
        if len(todo) == 0:
            return feat
    raise RuntimeError("conditioned_features: could not meet the quantise gap")


def conditioned_inputs(seed, n, K, D, ma=5):
    """Seeded (cent [K,D], feat [n,D]) f32, the features conditioned as above."""
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((K, D)).astype(np.float32)
    return cent, conditioned_features(rng, cent, n, ma)
