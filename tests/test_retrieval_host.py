"""Retrieval on the host side: the library exports the retrieval entry points, the bindings and
RetrievalDatabase check their arguments before any device work, and the configuration carries the
reference's retrieval / reloc blocks.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

ENTRY_POINTS = ["m3s_retrieval_create", "m3s_retrieval_destroy", "m3s_retrieval_size",
                "m3s_retrieval_term_table", "m3s_retrieval_quantize", "m3s_retrieval_aggregate",
                "m3s_retrieval_query", "m3s_retrieval_add", "m3s_retrieval_image"]


def test_library_exports_the_retrieval_entry_points(backend):
    lib = ctypes.CDLL(backend.library_path)
    missing = [s for s in ENTRY_POINTS if not hasattr(lib, s)]
    assert not missing, missing
    for name in ("retrieval_create", "retrieval_query", "retrieval_add", "retrieval_quantize",
                 "retrieval_aggregate", "retrieval_image", "retrieval_size", "retrieval_destroy"):
        assert callable(getattr(backend, name)), name


def test_config_has_the_retrieval_and_reloc_blocks():
    from m3s.config import DEFAULT_CONFIG, config

    assert DEFAULT_CONFIG["retrieval"] == {"k": 3, "min_thresh": 5e-3}
    assert DEFAULT_CONFIG["reloc"] == {"min_match_frac": 0.3, "strict": True}
    assert config["retrieval"]["k"] == 3
    assert DEFAULT_CONFIG["matching"]["max_iter"] == 10  # the existing blocks are untouched


def test_create_rejects_bad_arguments_before_the_device(backend):
    c = torch.zeros(16, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        backend.retrieval_create(c)
    with pytest.raises(RuntimeError, match="expected scalar type Float"):
        backend.retrieval_create(c.double())
    with pytest.raises(RuntimeError, match="outside 1..4096"):
        backend.retrieval_create(torch.zeros(16, 4097))
    with pytest.raises(RuntimeError, match="ma_build <= ma_query"):
        backend.retrieval_create(c, ma_build=2, ma_query=1)
    with pytest.raises(RuntimeError, match="ma_build <= ma_query"):
        backend.retrieval_create(c, ma_query=9)
    with pytest.raises(RuntimeError, match="smaller than the multiple assignment"):
        backend.retrieval_create(torch.zeros(3, 8))
    with pytest.raises(RuntimeError, match="max_feat"):
        backend.retrieval_create(c, max_feat=2000)
    with pytest.raises(RuntimeError, match="table must hold 33 floats"):
        backend.retrieval_create(c, table=np.zeros(5, dtype=np.float32))


def test_c_abi_rejects_bad_arguments(backend):
    lib = backend.lib
    out = ctypes.c_void_p()
    host = np.zeros((16, 8), dtype=np.float32)
    rc = lib.m3s_retrieval_create(host.ctypes.data, 16, 0, 1, 5, 3.0, 0.0, None, 300, ctypes.byref(out))
    assert rc == 1 and b"D = 0" in lib.m3s_last_error()
    rc = lib.m3s_retrieval_create(host.ctypes.data, 4, 8, 1, 5, 3.0, 0.0, None, 300, ctypes.byref(out))
    assert rc == 1 and b"K = 4" in lib.m3s_last_error()
    rc = lib.m3s_retrieval_create(host.ctypes.data, 16, 8, 1, 5, 3.0, 0.0, None, 5000, ctypes.byref(out))
    assert rc == 1 and b"max_feat" in lib.m3s_last_error()
    assert out.value is None
    rc = lib.m3s_retrieval_quantize(None, host.ctypes.data, 4, 1, None, None)
    assert rc == 1 and b"null database" in lib.m3s_last_error()
    assert lib.m3s_retrieval_destroy(None) == 0


def test_term_table_binding(backend):
    t = backend.retrieval_term_table(128, 3.0, 0.0)
    assert t.dtype == np.float32 and t.shape == (129,)
    assert t[0] == 1.0 and t[64] == 0.0 and (t[65:] == 0.0).all() and (np.diff(t[:65]) < 0).all()
    assert backend.retrieval_term_table(128, 3.0, -1.0)[128] == -1.0
    with pytest.raises(RuntimeError, match="outside 1..4096"):
        backend.retrieval_term_table(0, 3.0, 0.0)


def test_database_class_checks_its_parameters():
    import copy

    from m3s.retrieval_database import ASMK_PARAMS, RetrievalDatabase

    cent = torch.zeros(16, 8)
    p = copy.deepcopy(ASMK_PARAMS)
    p["build_ivf"]["ivf"]["use_idf"] = True
    with pytest.raises(ValueError, match="use_idf"):
        RetrievalDatabase(cent, device="cpu", params=p)
    p = copy.deepcopy(ASMK_PARAMS)
    p["build_ivf"]["kernel"]["binary"] = False
    with pytest.raises(ValueError, match="binary"):
        RetrievalDatabase(cent, device="cpu", params=p)
    with pytest.raises(ValueError, match=r"\[K, D\]"):
        RetrievalDatabase(torch.zeros(16), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):  # no CPU fallback
        RetrievalDatabase(cent, device="cpu")
    assert ASMK_PARAMS["query_ivf"]["quantize"]["multiple_assignment"] == 5
    assert ASMK_PARAMS["query_ivf"]["similarity"] == {"similarity_threshold": 0.0, "alpha": 3.0}
