"""FM / CrossNetwork backward without a GPU: the new entry points are exported, every limit is refused with its argument
named (validation precedes any HIP call), the workspace size is sane, and the float64 restatement's gradients are
pinned by central finite differences."""
import pytest
import torch

import interact_ref as R
import interact_train_ref as T
from recommendflow_amd.runtime import lib as L

NEW = ("rf_fm_bwd", "rf_cross_bwd", "rf_cross_bwd_ws_bytes")


def test_symbols_exported():
    lib = L.load()
    for s in NEW:
        assert s in L.EXPORTED and hasattr(lib, s), s


def _fm_bwd(lib, fields=4, dim=8, x=16, V=None, dsf=None, dsb=None):
    dsf = max(dim, 1) if dsf is None else dsf
    dsb = max(fields, 1) * dsf if dsb is None else dsb
    return lib.rf_fm_bwd(x, L.DT_F32, max(fields * dim, 0), dim, V, None, 0, 0, 1, fields, dim, 16, 16, dsb, dsf, None)


@pytest.mark.parametrize("kw,name", [({"dim": 0}, b"dim"), ({"dim": 1025}, b"dim"), ({"fields": 0}, b"fields"),
                                     ({"fields": 4097}, b"fields"), ({"x": None}, b"exactly one"),
                                     ({"V": 16}, b"exactly one"), ({"dsf": 7}, b"dx_stride_f"),
                                     ({"dsb": 31}, b"dx_stride_b")])
def test_fm_bwd_limits(kw, name):
    lib = L.load()
    assert _fm_bwd(lib, **kw) == L.RF_EINVAL
    msg = lib.rf_last_error()
    assert b"rf_fm_bwd" in msg and name in msg, msg


def test_fm_bwd_dtype_and_gather_arguments():
    lib = L.load()
    assert lib.rf_fm_bwd(16, L.DT_F16, 32, 8, None, None, 0, 0, 1, 4, 8, 16, 16, 32, 8, None) == L.RF_EINVAL
    assert b"x_dtype" in lib.rf_last_error()
    # gathered form without ids
    assert lib.rf_fm_bwd(None, L.DT_F32, 0, 0, 16, None, 0, 10, 1, 4, 8, 16, 16, 32, 8, None) == L.RF_EINVAL
    assert b"ids" in lib.rf_last_error()


def _cross_bwd(lib, dim=8, layers=2, batch=1, ws_bytes=1 << 30, dtype=L.DT_F32):
    ld = max(dim, 1)
    return lib.rf_cross_bwd(16, dtype, ld, batch, dim, layers, 16, 16, 16, ld, 16, ld, 16, 16, 16, ws_bytes, None)


@pytest.mark.parametrize("kw,name", [({"dim": 0}, b"dim"), ({"dim": 32769}, b"dim"), ({"layers": 0}, b"n_layers"),
                                     ({"layers": 17}, b"n_layers"), ({"dtype": L.DT_F16}, b"x_dtype"),
                                     ({"batch": -1}, b"batch")])
def test_cross_bwd_limits(kw, name):
    lib = L.load()
    assert _cross_bwd(lib, **kw) == L.RF_EINVAL
    msg = lib.rf_last_error()
    assert b"rf_cross_bwd" in msg and name in msg, msg


def test_cross_bwd_workspace():
    lib = L.load()
    need = lib.rf_cross_bwd_ws_bytes(3, 8, 2)
    assert need >= 3 * 2 * 2 * 4 + 3 * 8 * 4  # the scalars of every example and one chunk of [L + 1][dim] partials
    sizes = [lib.rf_cross_bwd_ws_bytes(B, 8, 2) for B in (0, 1, 127, 128, 129, 1000, 4096)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[1]
    assert lib.rf_cross_bwd_ws_bytes(4, 0, 2) == 0 and lib.rf_cross_bwd_ws_bytes(4, 8, 17) == 0
    # no [B][L][dim] intermediate: the workload's shape stays far below batch * layers * dim * 4 bytes
    assert lib.rf_cross_bwd_ws_bytes(4096, 29184, 3) < 4096 * 3 * 29184 * 4 // 16
    assert _cross_bwd(lib, batch=3, ws_bytes=need - 1) == L.RF_EINVAL
    assert b"ws_bytes" in lib.rf_last_error()
    assert lib.rf_cross_bwd(16, L.DT_F32, 7, 1, 8, 2, 16, 16, 16, 8, 16, 8, 16, 16, 16, 1 << 30, None) == L.RF_EINVAL
    assert b"ldx" in lib.rf_last_error()


def test_batch_zero_is_a_no_op_without_a_gpu():
    lib = L.load()
    assert lib.rf_fm_bwd(16, L.DT_F32, 32, 8, None, None, 0, 0, 0, 4, 8, None, None, 32, 8, None) == L.RF_OK
    assert _cross_bwd(lib, batch=0, ws_bytes=0) == L.RF_OK


def test_fm_restatement_gradient_by_finite_differences():
    g = torch.Generator().manual_seed(5)
    e = torch.randn(3, 5, 10, generator=g, dtype=torch.float64)
    gout = torch.randn(3, generator=g, dtype=torch.float64)
    _, de = T.fm_grads(e, gout)
    fd = T.central_differences(lambda t: (R.fm(t)[:, 0] * gout).sum(), e)
    err = R.rel_err(de, fd)
    print("fm autograd vs central differences", err)
    assert err <= 1e-8
    # and the closed form the kernel implements: g (S - e)
    closed = gout[:, None, None] * (e.sum(dim=1, keepdim=True) - e)
    assert R.rel_err(closed, de) <= 1e-12


def test_cross_restatement_gradient_by_finite_differences():
    g = torch.Generator().manual_seed(6)
    B, dim, layers = 3, 10, 2
    x = torch.randn(B, dim, generator=g, dtype=torch.float64)
    w = torch.randn(layers, dim, generator=g, dtype=torch.float64) * 0.3
    b = torch.randn(layers, dim, generator=g, dtype=torch.float64) * 0.3
    gout = torch.randn(B, dim, generator=g, dtype=torch.float64)
    _, dx, dw, db = T.cross_grads(x, w, b, gout)

    def f(xx, ww, bb):
        return (R.cross(xx, [ww[i].unsqueeze(1) for i in range(layers)], [bb[i].unsqueeze(1) for i in range(layers)]) * gout).sum()

    for name, got, fd in (("dx", dx, T.central_differences(lambda t: f(t, w, b), x)),
                          ("dw", dw, T.central_differences(lambda t: f(x, t, b), w)),
                          ("db", db, T.central_differences(lambda t: f(x, w, t), b))):
        err = R.rel_err(got, fd)
        print("cross", name, "autograd vs central differences", err)
        assert err <= 1e-8, name
