"""Loop-closure retrieval database on the device.

Mirrors the reference's ``RetrievalDatabase`` (mast3r_slam/retrieval_database.py:9-166) from the
prepared local features on: ``update`` quantises them against the ASMK codebook, aggregates binary
codes per visual word, scores every stored image and optionally adds the image -- all in HIP
kernels (csrc/retrieval.hip); the only host round trip is the copy of the scores for the host
``topk`` the reference performs as well.  ASMK parameters are the reference's
(thirdparty/mast3r/mast3r/retrieval/processor.py:91-96): binary kernel, no idf, multiple
assignment 1 (build) / 5 (query), alpha 3, similarity threshold 0.

The retrieval network is not part of this package: pass ``model`` (an object with the
reference model's ``prewhiten``, ``projector``, ``residual``, ``attention``, ``postwhiten``,
``nfeat`` and a ``select_local`` callable) to have ``prep_features`` applied to ``frame.feat``;
without one, ``update`` takes the prepared features ``[n, D]`` (or ``[1, n, D]``) themselves.
"""
from __future__ import annotations

import torch

import mast3r_slam_backends as mb

ASMK_PARAMS = {  # processor.py:91-96
    "build_ivf": {"kernel": {"binary": True}, "ivf": {"use_idf": False},
                  "quantize": {"multiple_assignment": 1}, "aggregate": {}},
    "query_ivf": {"quantize": {"multiple_assignment": 5}, "aggregate": {},
                  "search": {"topk": None},
                  "similarity": {"similarity_threshold": 0.0, "alpha": 3.0}},
}


class RetrievalDatabase:
    def __init__(self, centroids, model=None, device="cuda", params=None, max_feat=300, table=None):
        """centroids [K, D] (tensor or array): the ASMK codebook.  ``params``: an ASMK parameter
        dict shaped like ``ASMK_PARAMS``.  ``max_feat``: the most local features one image brings.
        ``table``: optional score term table (mast3r_slam_backends.retrieval_create)."""
        self.params = ASMK_PARAMS if params is None else params
        build, query = self.params["build_ivf"], self.params["query_ivf"]
        if build.get("ivf", {}).get("use_idf", False):
            raise ValueError("RetrievalDatabase: use_idf=True is not supported (the reference runs "
                             "use_idf=False)")
        if build.get("kernel", {}).get("binary", True) not in (True, "bin"):
            raise ValueError("RetrievalDatabase: only the binary ASMK kernel is supported")
        self.model = model
        self.kf_counter = 0
        self.kf_ids = []
        self.query_dtype = torch.float32
        self.query_device = torch.device(device)
        self.centroids = torch.as_tensor(centroids).to(
            device=self.query_device, dtype=self.query_dtype).contiguous()
        if self.centroids.dim() != 2:
            raise ValueError("RetrievalDatabase: centroids must be [K, D]")
        sim = query["similarity"]
        self._db = mb.retrieval_create(
            self.centroids, build["quantize"]["multiple_assignment"],
            query["quantize"]["multiple_assignment"], sim["alpha"], sim["similarity_threshold"],
            table=table, max_feat=max_feat)

    # retrieval_database.py:25-41
    def prep_features(self, backbone_feat):
        m = self.model
        if m is None:
            return backbone_feat
        pre = m.prewhiten(backbone_feat)
        proj = m.projector(pre) + (0.0 if not m.residual else pre)
        attention = m.attention(proj)
        topk_features, _, _ = m.select_local(m.postwhiten(proj), attention, m.nfeat)
        return topk_features

    def _features(self, frame_or_feat):
        feat = frame_or_feat.feat if hasattr(frame_or_feat, "feat") else frame_or_feat
        if not isinstance(feat, torch.Tensor):
            raise TypeError("RetrievalDatabase: expected a frame with .feat or a feature tensor")
        feat = self.prep_features(feat)
        if feat.dim() == 3:
            if feat.shape[0] != 1:
                raise ValueError("RetrievalDatabase: one frame at a time")
            feat = feat[0]
        if feat.dim() != 2 or feat.shape[1] != self.centroids.shape[1]:
            raise ValueError(f"RetrievalDatabase: features must be [n, {self.centroids.shape[1]}], "
                             f"got {tuple(feat.shape)}")
        return feat.to(device=self.query_device, dtype=self.query_dtype).contiguous()

    def update(self, frame, add_after_query, k, min_thresh=0.0):
        """retrieval_database.py:43-72 -> the list of stored-image indices to close loops with."""
        feat = self._features(frame)
        topk_image_inds = []
        queried = False
        if self.kf_counter > 0:
            scores = mb.retrieval_query(self._db, feat).cpu()  # the update's one host round trip
            topk_images = torch.topk(scores, min(int(k), self.kf_counter))
            valid = topk_images.values > min_thresh
            topk_image_inds = topk_images.indices[valid].tolist()
            queried = True
        if add_after_query:
            self._add(feat, queried)
        return topk_image_inds

    def query(self, feat):
        """-> scores [n_images] f64 on the device."""
        return mb.retrieval_query(self._db, self._features(feat))

    def add_to_database(self, feat):
        """Quantise (build parameters), aggregate and append the image."""
        self._add(self._features(feat), False)

    def _add(self, feat, reuse_last_query):
        mb.retrieval_add(self._db, feat, reuse_last_query)
        self.kf_ids.append(self.kf_counter)
        self.kf_counter += 1

    def quantize_custom(self, qvecs, params):
        """retrieval_database.py:96-105 -> [n, ma] indices of the nearest centroids."""
        return mb.retrieval_quantize(self._db, self._features(qvecs),
                                     params["quantize"]["multiple_assignment"]).long()

    def stored_image(self, m):
        """Stored image m -> (words, codes) on the device (inspection)."""
        return mb.retrieval_image(self._db, m)

    def __len__(self):
        return self.kf_counter

    def close(self):
        self._db.close()
