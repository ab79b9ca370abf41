"""IVF-Flat search, the parts that need no GPU: the index string parser, the constructor's argument checks (made
before the library or a GPU is touched), the host check of a stored partition, and the C entries' argument
validation."""
import numpy as np
import pytest
import torch

from recommendflow_amd.backend.third_party_components import faiss_searcher as FS
from recommendflow_amd.runtime import lib as L


@pytest.mark.parametrize("text,want", [("Flat", ("flat", None)), ("flat", ("flat", None)), ("IVF64,Flat", ("ivf", 64)),
                                       ("ivf8, flat", ("ivf", 8)), ("IVF1024,Flat", ("ivf", 1024))])
def test_parse_index_param_accepts(text, want):
    assert FS.parse_index_param(text) == want


@pytest.mark.parametrize("text", ["HNSW32", "IVF64,PQ8", "IVF,Flat", "PQ16", "IVF64", "IVF-3,Flat", "IVF64,Flat,x"])
def test_parse_index_param_rejects(text):
    with pytest.raises(NotImplementedError):
        FS.parse_index_param(text)


ITEMS = np.zeros((10, 8), np.float32)


@pytest.mark.parametrize("kwargs", [dict(index_param="IVF0,Flat"), dict(index_param="IVF32769,Flat"),
                                    dict(index_param="IVF4,Flat", nprobe=0), dict(index_param="IVF4,Flat", niter=-1)])
def test_constructor_value_errors(kwargs):
    with pytest.raises(ValueError):
        FS.FaissSearcher(items=ITEMS, measurement="ip", **kwargs)


@pytest.mark.parametrize("kwargs", [dict(index_param="IVF4,Flat", dtype=torch.bfloat16),
                                    dict(index_param="IVF4,Flat", dtype=torch.float16), dict(index_param="HNSW64"),
                                    dict(index_param="IVF256,PQ32"), dict(index_param="PQ16")])
def test_constructor_not_implemented(kwargs):
    with pytest.raises(NotImplementedError):
        FS.FaissSearcher(items=ITEMS, measurement="ip", **kwargs)


def good_arrays():
    off = np.array([0, 3, 3, 7, 10], np.int64)
    ids = np.array([0, 4, 9, 1, 2, 5, 8, 3, 6, 7], np.int64)
    return off, ids


def test_validate_ivf_arrays_accepts():
    off, ids = good_arrays()
    FS.validate_ivf_arrays(off, ids, 10, 4)
    FS.validate_ivf_arrays(off.astype(np.int32), ids.astype(np.uint32), 10, 4)
    FS.validate_ivf_arrays(np.array([0, 0]), np.zeros(0, np.int64), 0, 1)


@pytest.mark.parametrize("case", ["end", "decreasing", "duplicate", "too_large", "start", "short_off"])
def test_validate_ivf_arrays_rejects(case):
    off, ids = good_arrays()
    if case == "end":
        off[-1] = 9
    elif case == "decreasing":
        off[1], off[2] = 5, 3
    elif case == "duplicate":
        ids[3] = ids[0]
    elif case == "too_large":
        ids[2] = 10
    elif case == "start":
        off[0] = 1
    elif case == "short_off":
        off = off[:-1]
    with pytest.raises(ValueError):
        FS.validate_ivf_arrays(off, ids, 10, 4)


def test_entries_validate_before_any_hip_call():
    lib = L.load()
    # K = 6 is no multiple of 4
    rc = lib.rf_ivf_scan_f32(None, 8, 1, None, 0, 6, None, None, None, None, 0, None, None, None, None, 0, None)
    assert rc == L.RF_EINVAL and b"rf_ivf_scan_f32" in lib.rf_last_error()
    rc = lib.rf_ivf_scan_f32(None, 2048, 1, None, 0, 1028, None, None, None, None, 0, None, None, None, None, 0, None)
    assert rc == L.RF_EINVAL
    rc = lib.rf_ivf_scan_f32(None, 8, 0, None, 0, 8, None, None, None, None, 0, None, None, None, None, 0, None)
    assert rc == L.RF_EINVAL  # M = 0
    rc = lib.rf_ivf_build_lists(None, 0, 0, None, None, None, 0, None)
    assert rc == L.RF_EINVAL and b"rf_ivf_build_lists" in lib.rf_last_error()
    assert lib.rf_ivf_build_lists(None, 5, 32769, None, None, None, 0, None) == L.RF_EINVAL
    assert lib.rf_ivf_build_lists(None, 1 << 31, 4, None, None, None, 1 << 30, None) == L.RF_EINVAL
    assert lib.rf_ivf_list_mean(None, 0, None, 4, 0, None, None) == L.RF_EINVAL
    assert lib.rf_ivf_list_mean(None, 8, None, 4, 2, None, None) == L.RF_EINVAL
    assert lib.rf_ivf_build_ws_bytes(1000, 7) > 0
