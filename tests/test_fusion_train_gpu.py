"""GPU: rf_attention_fusion_bwd (dx, deterministic dW) and TrainAttentionFusion against the float64 restatement
(tests/fusion_ref.py). Tolerance per output tensor: err = max|got - want| / max|want| <= 8 x the err of the float32
torch-CPU evaluation of the same formula, floor 2^-20 (fusion_ref.bar)."""
import functools

import pytest
import torch

import fusion_ref as R
from recommendflow_amd.runtime import lib as L

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 4), (5, 2, 1), (7, 3, 33), (130, 4, 64), (64, 16, 128), (3, 6, 200), (1000, 5, 64)]
PAD_X, PAD_G, PAD_DX, SENTINEL = 5, 3, 7, 777.0


@functools.lru_cache(maxsize=None)
def _case(B, C, d, zero_row=-1):
    gen = torch.Generator().manual_seed(1000 * B + 10 * C + d)
    K = C * d
    x = torch.randn(B, K, generator=gen)
    if zero_row >= 0:
        x[zero_row] = 0.0
    W = (torch.rand(K, C, generator=gen) * 2 - 1) * (6.0 / (K + C)) ** 0.5 * 4
    g = torch.randn(B, d, generator=gen)
    return x, W, g


@functools.lru_cache(maxsize=None)
def _ref(B, C, d, is_norm, zero_row=-1):
    """(float64 dx, dW; float32-CPU dx, dW) of the case, computed once and shared."""
    x, W, g = _case(B, C, d, zero_row)
    _, _, dx64, dW64 = R.fusion_grads(x, W, g, C, d, is_norm, torch.float64)
    _, _, dx32, dW32 = R.fusion_grads(x, W, g, C, d, is_norm, torch.float32)
    return dx64, dW64, dx32, dW32


def _run(B, C, d, is_norm, zero_row=-1, with_dW=True):
    """The forward (for att) and the backward through the C ABI, every row stride wider than its row; pad columns
    of the inputs hold NaN (never read), pad columns of dx a sentinel (never written)."""
    x, W, g = _case(B, C, d, zero_row)
    K = C * d
    xb = torch.full((B, K + PAD_X), float("nan"))
    xb[:, :K] = x
    gb = torch.full((B, d + PAD_G), float("nan"))
    gb[:, :d] = g
    xb, gb, Wd = xb.cuda(), gb.cuda(), W.cuda()
    out = torch.empty((B, d), device="cuda")
    att = torch.empty((B, C), device="cuda")
    L.call("rf_attention_fusion_fwd", L.ptr(xb), B, C, d, xb.stride(0), L.ptr(Wd), is_norm, L.ptr(out), d, L.ptr(att),
           L.stream_ptr())
    dxb = torch.full((B, K + PAD_DX), SENTINEL, device="cuda")
    dW = torch.full((K, C), SENTINEL, device="cuda") if with_dW else None
    wsb = int(L.load().rf_attention_fusion_bwd_ws_bytes(B, C, d))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    L.call("rf_attention_fusion_bwd", L.ptr(xb), B, C, d, xb.stride(0), L.ptr(Wd), is_norm, L.ptr(att), L.ptr(gb),
           gb.stride(0), L.ptr(dxb), dxb.stride(0), L.ptr(dW), L.ptr(ws), wsb, L.stream_ptr())
    torch.cuda.synchronize()
    assert bool((dxb[:, K:] == SENTINEL).all()), "dx pad columns were written"
    return dxb[:, :K].contiguous(), dW


def _check(name, got, want64, want32, scale=None):
    err, bar = R.rel_err(got, want64, scale), R.bar(want32, want64, scale)
    print(f"{name}: err {err:.3e} bar {bar:.3e} (float32 CPU err {R.rel_err(want32, want64, scale):.3e})")
    assert bool(torch.isfinite(got).all()) and err <= bar, (name, err, bar)


@pytest.mark.parametrize("is_norm", [0, 1])
@pytest.mark.parametrize("B,C,d", SHAPES)
def test_kernel_against_float64(cuda, B, C, d, is_norm):
    dx64, dW64, dx32, dW32 = _ref(B, C, d, is_norm)
    dx, dW = _run(B, C, d, is_norm)
    # d = 1 under is_norm: the exact gradients are identically zero, err is taken against the size of the terms that
    # cancel instead of max|want| = float64 rounding noise (fusion_ref.cancel_scale); same 8x rule and floor
    sx, sw = R.cancel_scale(*_case(B, C, d), C, d) if (d == 1 and is_norm) else (None, None)
    _check(f"dx B{B} C{C} d{d} norm{is_norm}", dx, dx64, dx32, sx)
    _check(f"dW B{B} C{C} d{d} norm{is_norm}", dW, dW64, dW32, sw)
    if C == 1:  # one channel: att = 1, the softmax backward and dW are exactly zero
        assert float(dW.abs().max()) == 0.0


def test_clamped_branch(cuda):
    """One all-zero row under is_norm: ss = 0 takes the clamped branch (r = 1e6, no gradient through ss)."""
    B, C, d, z = 4, 3, 8, 2
    dx64, dW64, dx32, dW32 = _ref(B, C, d, 1, z)
    dx, dW = _run(B, C, d, 1, z)
    assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dW).all())
    _check("clamped dx", dx, dx64, dx32)
    _check("clamped dW", dW, dW64, dW32)
    _check("clamped dx, the zero row", dx[z], dx64[z], dx32[z])


@pytest.mark.parametrize("is_norm", [0, 1])
def test_null_dW_leaves_dx_identical(cuda, is_norm):
    dx_a, _ = _run(130, 4, 64, is_norm)
    dx_b, none = _run(130, 4, 64, is_norm, with_dW=False)
    assert none is None and torch.equal(dx_a, dx_b)


@pytest.mark.parametrize("B,C,d", [(1000, 5, 64), (64, 16, 128)])
def test_two_launches_are_bit_identical(cuda, B, C, d):
    dx_a, dW_a = _run(B, C, d, 1)
    dx_b, dW_b = _run(B, C, d, 1)
    assert torch.equal(dx_a, dx_b) and torch.equal(dW_a, dW_b)


@pytest.mark.parametrize("is_norm", [False, True])
def test_layer_gradients_and_infer_weights(cuda, is_norm):
    from recommendflow_amd.backend.layers.fusion_layers import AttentionFusion, TrainAttentionFusion

    B, C, d = 37, 3, 33
    x, _, g = _case(B, C, d)
    layer = TrainAttentionFusion(d, C, is_norm=is_norm, seed=5)
    parent = AttentionFusion(d, C, is_norm=is_norm, seed=5)
    assert isinstance(layer.W, torch.nn.Parameter) and not isinstance(parent.W, torch.nn.Parameter)
    assert torch.equal(layer.W.detach(), parent.W)
    ins = [x[:, c * d: (c + 1) * d].cuda().requires_grad_(True) for c in range(C)]
    out = layer(ins, True)
    assert torch.equal(out.detach(), parent([t.detach() for t in ins], True))
    (out * g.cuda()).sum().backward()
    W = layer.W.detach().cpu()
    _, _, dx64, dW64 = R.fusion_grads(x, W, g, C, d, is_norm, torch.float64)
    _, _, dx32, dW32 = R.fusion_grads(x, W, g, C, d, is_norm, torch.float32)
    for c in range(C):
        sl = slice(c * d, (c + 1) * d)
        _check(f"layer input {c} norm{int(is_norm)}", ins[c].grad, dx64[:, sl], dx32[:, sl])
    _check(f"layer W norm{int(is_norm)}", layer.W.grad, dW64, dW32)
    # the inference statistics accumulate in both modes, as the parent's do
    with torch.no_grad():
        layer([t.detach() for t in ins], False)
    parent([t.detach() for t in ins], False)
    assert torch.equal(layer.infer_weights, parent.infer_weights)
    assert abs(float(layer.get_fusion_weights().sum()) - 1.0) < 1e-6
