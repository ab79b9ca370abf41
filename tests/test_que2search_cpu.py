"""CPU: the float64 AttentionFusion restatement is pinned by finite differences, rf_attention_fusion_bwd validates its
arguments before any HIP call, and TrainableQue2Search refuses more than 16 channels before touching the library."""
import ctypes
import types

import pytest
import torch

import fusion_ref as R
from recommendflow_amd.models.matching.que2search import MAX_CHANNELS, TrainableQue2Search
from recommendflow_amd.runtime import lib as L


@pytest.mark.parametrize("is_norm", [0, 1])
def test_reference_backward_against_finite_differences(is_norm):
    """Central differences of L = sum(out * g) in float64 at (B 3, C 3, d 5): step 1e-6, truncation error
    O(h^2) ~ 1e-12 and rounding ~ 1e-16 / 1e-6 = 1e-10 on values of order 1, so 1e-7 relative is a safe bar."""
    B, C, d = 3, 3, 5
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(B, C * d, generator=gen, dtype=torch.float64)
    W = torch.randn(C * d, C, generator=gen, dtype=torch.float64) * 0.5
    g = torch.randn(B, d, generator=gen, dtype=torch.float64)
    _, _, dx, dW = R.fusion_grads(x, W, g, C, d, is_norm)

    def loss(xx, ww):
        return float((R.fusion(xx, ww, C, d, is_norm)[0] * g).sum())

    h = 1e-6
    for t, grad, is_x in ((x, dx, True), (W, dW, False)):
        fd = torch.zeros_like(t)
        for i in range(t.numel()):
            tp, tm = t.clone(), t.clone()
            tp.view(-1)[i] += h
            tm.view(-1)[i] -= h
            fd.view(-1)[i] = (loss(tp, W) - loss(tm, W)) / (2 * h) if is_x else (loss(x, tp) - loss(x, tm)) / (2 * h)
        assert R.rel_err(grad, fd) < 1e-7, (is_norm, is_x, R.rel_err(grad, fd))


def test_reference_clamped_branch_passes_no_norm_gradient():
    """An all-zero row with is_norm: ss = 0 < 1e-12, the gradient is rsqrt(1e-12) * g through u alone (finite)."""
    C, d = 2, 3
    x = torch.zeros(1, C * d, dtype=torch.float64)
    W = torch.ones(C * d, C, dtype=torch.float64)
    g = torch.tensor([[1.0, -2.0, 0.5]], dtype=torch.float64)
    _, att, dx, dW = R.fusion_grads(x, W, g, C, d, 1)
    want = torch.cat([att[0, c] * 1e6 * g for c in range(C)], dim=1)
    assert torch.isfinite(dx).all() and R.rel_err(dx, want) < 1e-12
    assert float(dW.abs().max()) == 0.0


def _bwd(lib, **kw):
    a = dict(x=8, batch=2, channels=2, dim=4, ldx=8, W=8, is_norm=1, att=8, dout=8, ldg=4, dx=8, lddx=8, dW=8, ws=16,
             ws_bytes=1 << 20, stream=None)
    a.update(kw)
    return lib.rf_attention_fusion_bwd(a["x"], a["batch"], a["channels"], a["dim"], a["ldx"], a["W"], a["is_norm"],
                                       a["att"], a["dout"], a["ldg"], a["dx"], a["lddx"], a["dW"], a["ws"],
                                       a["ws_bytes"], a["stream"])


def test_bwd_argument_errors_without_gpu():
    """Every rejected call returns RF_EINVAL with the entry's name in rf_last_error, before any HIP call (the
    pointers are never dereferenced: the values are small non-null integers)."""
    lib = L.load()
    need = lib.rf_attention_fusion_bwd_ws_bytes(2, 2, 4)
    assert need > 0 and lib.rf_attention_fusion_bwd_ws_bytes(4096, 16, 256) > need
    bad = [dict(channels=0), dict(channels=17), dict(ldx=7), dict(lddx=7), dict(ldg=3), dict(ws_bytes=need - 1),
           dict(x=None), dict(W=None), dict(att=None), dict(dout=None), dict(dx=None), dict(ws=None)]
    for kw in bad:
        assert _bwd(lib, **kw) == L.RF_EINVAL, kw
        assert b"rf_attention_fusion_bwd" in lib.rf_last_error(), kw
    # batch 0 is a no-op whatever the pointers are
    assert _bwd(lib, batch=0, x=None, W=None, att=None, dout=None, dx=None, dW=None, ws=None, ws_bytes=0) == L.RF_OK


def test_bwd_binding_matches_header():
    assert "rf_attention_fusion_bwd" in L.EXPORTED and "rf_attention_fusion_bwd_ws_bytes" in L.EXPORTED
    res, args = L._SIGS["rf_attention_fusion_bwd"]
    assert res is ctypes.c_int and len(args) == 16


def test_constructor_refuses_17_channels():
    """The check runs on the encoder's widths alone: a stub without a table or a device is enough to reach it."""
    assert MAX_CHANNELS == 16
    enc = types.SimpleNamespace(out_width=2 * 8 * 18, dim=8)
    with pytest.raises(ValueError, match="17 channels"):
        TrainableQue2Search(enc, 1, 16)
    with pytest.raises(ValueError, match="17 channels"):
        TrainableQue2Search(enc, 17, 16)
    with pytest.raises(ValueError, match="0 channels"):
        TrainableQue2Search(types.SimpleNamespace(out_width=2 * 8 * 4, dim=8), 4, 16)
