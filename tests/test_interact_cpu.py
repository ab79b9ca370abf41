"""Feature-interaction layers without a GPU: the float64 restatements agree with each other, the new entry points are
exported, and every limit is refused with its argument named (validation precedes any HIP call)."""
import ctypes

import pytest
import torch

import interact_ref as R
from recommendflow_amd.runtime import lib as L


def test_cin_literal_matches_einsum():
    """fields != H_k: a swapped (i, j) order in the flattened index i H_k + j would not survive."""
    x, Ws = R.cin_inputs(3, 5, 6, [7, 4, 3], seed=1)
    x, Ws = x.double(), [W.double() for W in Ws]
    a, b = R.cin_literal(x, Ws), R.cin_einsum(x, Ws)
    assert a.shape == (3, 14)
    err = R.rel_err(a, b)
    print("cin literal vs einsum", err)
    assert err <= 1e-12
    # the transposed flattening is a different function
    Wt = [W[0].reshape(5, h, -1).transpose(0, 1).reshape(1, 5 * h, -1) for W, h in zip(Ws, [5, 7, 4])]
    assert R.rel_err(R.cin_literal(x, Wt), b) > 1e-3


def test_fm_second_order_is_the_pair_sum():
    g = torch.Generator().manual_seed(2)
    e = torch.randn(4, 7, 5, generator=g, dtype=torch.float64)
    err = R.rel_err(R.fm(e), R.fm_pairs(e))
    print("fm vs pairs", err)
    assert err <= 1e-12


def test_symbols_exported():
    lib = L.load()
    for s in ("rf_fm_fwd", "rf_cross_fwd", "rf_cin_fwd", "rf_cin_ws_bytes", "rf_cin_pack_w", "rf_cin_packed_w_bytes"):
        assert s in L.EXPORTED and hasattr(lib, s), s


def _sizes(*v):
    return (ctypes.c_int32 * len(v))(*v)


def _fm(lib, fields=4, dim=8, n=0, x=1, V=None):
    return lib.rf_fm_fwd(x, L.DT_F32, fields * dim, dim, V, None, 0, 0, 1, fields, dim, None, None, None, n, 0, 0, None, None)


@pytest.mark.parametrize("kw,name", [({"dim": 1025}, b"dim"), ({"dim": 0}, b"dim"), ({"fields": 4097}, b"fields"),
                                     ({"fields": 0}, b"fields"), ({"n": 4097}, b"n ("), ({"x": None}, b"exactly one")])
def test_fm_limits(kw, name):
    lib = L.load()
    assert _fm(lib, **kw) == L.RF_EINVAL
    assert name in lib.rf_last_error(), lib.rf_last_error()


@pytest.mark.parametrize("dim,layers,name", [(32769, 1, b"dim"), (0, 1, b"dim"), (8, 0, b"n_layers"), (8, 17, b"n_layers")])
def test_cross_limits(dim, layers, name):
    lib = L.load()
    assert lib.rf_cross_fwd(1, L.DT_F32, max(dim, 1), 1, dim, layers, 1, 1, 1, max(dim, 1), None) == L.RF_EINVAL
    assert name in lib.rf_last_error(), lib.rf_last_error()


@pytest.mark.parametrize("fields,dim,sizes,name", [(513, 8, [4], b"fields"), (0, 8, [4], b"fields"), (4, 257, [4], b"dim"),
                                                   (4, 0, [4], b"dim"), (4, 8, [4, 513], b"sizes[1]"),
                                                   (4, 8, [0], b"sizes[0]"), (4, 8, [], b"n_layers"),
                                                   (4, 8, [4] * 9, b"n_layers")])
def test_cin_limits(fields, dim, sizes, name):
    lib = L.load()
    s = _sizes(*sizes) if sizes else _sizes(1)
    rc = lib.rf_cin_fwd(1, L.DT_F32, fields * dim, dim, 1, fields, dim, s, len(sizes), 1, 1, 1024, 1, 1 << 30, None)
    assert rc == L.RF_EINVAL
    assert name in lib.rf_last_error(), lib.rf_last_error()


def test_cin_dtype_and_workspace_are_checked():
    lib = L.load()
    s = _sizes(6, 4)
    assert lib.rf_cin_fwd(16, L.DT_F16, 40, 8, 1, 5, 8, s, 2, 16, 16, 10, 16, 1 << 20, None) == L.RF_EINVAL
    assert b"x_dtype" in lib.rf_last_error()
    need = lib.rf_cin_ws_bytes(3, 5, 8, s, 2)
    assert need >= 3 * 10 * 4
    assert lib.rf_cin_fwd(16, L.DT_F32, 40, 8, 3, 5, 8, s, 2, 16, 16, 10, 16, need - 1, None) == L.RF_EINVAL
    assert b"ws_bytes" in lib.rf_last_error()
    assert lib.rf_cin_packed_w_bytes(5, s, 2) % 1024 == 0 and lib.rf_cin_packed_w_bytes(5, s, 2) > 0


def test_index_mapping():
    from recommendflow_amd.backend.layers.layer_utils import index_mapping

    out = index_mapping({"a": torch.tensor([1, 2]), "b": torch.tensor([0, 3])}, {"a": 0, "b": 100})
    assert out["a"].shape == (2, 1) and out["b"].flatten().tolist() == [100, 103]
    with pytest.raises(ValueError, match="map dict error!"):
        index_mapping({"c": torch.tensor([1])}, {"a": 0})
