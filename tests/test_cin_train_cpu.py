"""No GPU: the ABI limits of rf_cin_bwd (validated before any HIP call) and the restatements of tests/cin_train_ref.py
(float64 autograd against central differences; the bf16 emulation's own error on every shape of the GPU list, which is
the condition that keeps the GPU tests' tolerance honest)."""
import ctypes

import pytest
import torch

import cin_train_ref as C
import interact_ref as R
from interact_train_ref import central_differences
from recommendflow_amd.runtime import lib as L


def _sizes(*v):
    return (ctypes.c_int32 * len(v))(*v)


def test_symbols_exported():
    lib = L.load()
    for s in ("rf_cin_bwd", "rf_cin_bwd_ws_bytes", "rf_cin_bwd_pack_w", "rf_cin_bwd_packed_w_bytes"):
        assert s in L.EXPORTED and hasattr(lib, s), s


def _bwd(lib, fields=5, dim=8, sizes=(6, 4), n_layers=None, batch=3, x_dtype=L.DT_F32, x_stride_f=None, lddo=10,
         dx_stride_b=None, dx_stride_f=None, packed_w=16, packed_w_t=16, ws=16, ws_bytes=1 << 40):
    """rf_cin_bwd on fake (never dereferenced) device pointers: every check comes before the first HIP call."""
    s = _sizes(*sizes) if sizes else _sizes(1)
    K = len(sizes) if n_layers is None else n_layers
    x_stride_f = dim if x_stride_f is None else x_stride_f
    dx_stride_f = dim if dx_stride_f is None else dx_stride_f
    dx_stride_b = fields * dx_stride_f if dx_stride_b is None else dx_stride_b
    dW = (ctypes.c_void_p * max(K, 1))(*([16] * max(K, 1)))
    return lib.rf_cin_bwd(16, x_dtype, fields * x_stride_f, x_stride_f, batch, fields, dim, s, K, packed_w, packed_w_t, 16,
                          lddo, 16, dx_stride_b, dx_stride_f, dW, ws, ws_bytes, None)


@pytest.mark.parametrize("kw,name", [
    (dict(fields=513), b"fields"), (dict(fields=0), b"fields"), (dict(dim=257), b"dim"), (dict(dim=0), b"dim"),
    (dict(sizes=(4, 513), lddo=1000), b"sizes[1]"), (dict(sizes=(0,)), b"sizes[0]"), (dict(sizes=(), n_layers=0), b"n_layers"),
    (dict(sizes=(4,) * 9, lddo=100), b"n_layers"), (dict(x_dtype=L.DT_F16), b"x_dtype"), (dict(x_stride_f=7), b"x_stride_f"),
    (dict(lddo=9), b"lddo"), (dict(dx_stride_f=7), b"dx_stride_f"), (dict(dx_stride_b=39), b"dx_stride_b"),
    (dict(packed_w=8), b"packed_w "), (dict(packed_w_t=8), b"packed_w_t"), (dict(ws=8), b"workspace"),
    (dict(ws_bytes=1000), b"ws_bytes"), (dict(packed_w=None), b"null"), (dict(batch=-1), b"batch"),
])
def test_cin_bwd_limits(kw, name):
    lib = L.load()
    assert _bwd(lib, **kw) == L.RF_EINVAL
    assert name in lib.rf_last_error(), lib.rf_last_error()


def test_batch_zero_is_a_no_op():
    lib = L.load()
    assert _bwd(lib, batch=0, packed_w=None, ws=None, ws_bytes=0) == L.RF_OK


def test_workspace_size():
    lib = L.load()
    s = _sizes(6, 4)
    last = 0
    for B in (0, 1, 2, 3, 4, 7, 64, 300, 1000, 1024, 1025, 4096, 20000):
        need = lib.rf_cin_bwd_ws_bytes(B, 5, 10, s, 2)
        assert need >= last and need > 0, (B, need, last)
        last = need
    assert lib.rf_cin_bwd_ws_bytes(4, 513, 10, s, 2) == 0
    assert lib.rf_cin_bwd_ws_bytes(4, 5, 257, s, 2) == 0
    assert lib.rf_cin_bwd_ws_bytes(-1, 5, 10, s, 2) == 0
    assert lib.rf_cin_bwd_ws_bytes(4, 5, 10, _sizes(6, 513), 2) == 0
    assert lib.rf_cin_bwd_packed_w_bytes(5, s, 2) > 0 and lib.rf_cin_bwd_packed_w_bytes(5, s, 2) % 1024 == 0
    # the probe shape: no [B][dim][F0 H] intermediate (one of them in fp32 is B D F0 128 4 bytes)
    B, F0, D = 4096, 200, 128
    need = lib.rf_cin_bwd_ws_bytes(B, F0, D, _sizes(128, 128), 2)
    print("rf_cin_bwd_ws_bytes at the probe shape:", need)
    assert 0 < need < B * D * F0 * 128 * 4 // 16


def test_float64_autograd_against_central_differences():
    B, F0, D, sizes = 2, 3, 4, [3, 2]
    x, Ws, g = C.inputs(B, F0, D, sizes)
    x, Ws, g = x.double(), [W.double() for W in Ws], g.double()
    _, dx, dWs = C.cin_grads(x, Ws, g)
    num = central_differences(lambda t: (R.cin_einsum(t, Ws) * g).sum(), x)
    assert R.rel_err(dx, num) <= 1e-8
    for k in range(2):
        def f(t, k=k):
            return (R.cin_einsum(x, [t if i == k else W for i, W in enumerate(Ws)]) * g).sum()
        assert R.rel_err(dWs[k], central_differences(f, Ws[k])) <= 1e-8


@pytest.mark.parametrize("bf16_x", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,F0,D,sizes", C.SHAPES)
def test_emulation_stays_under_the_cap(B, F0, D, sizes, bf16_x):
    x, Ws, g = C.inputs(B, F0, D, sizes, bf16_x)
    want = C.cin_grads(x, Ws, g)
    emu = C.cin_bwd_emulated(x, Ws, g)
    errs = [R.rel_err(emu[0], want[0]), R.rel_err(emu[1], want[1])] + \
        [R.rel_err(e, w) for e, w in zip(emu[2], want[2])]
    print(f"emulation {B}x{F0}x{D} {sizes}: out {errs[0]:.3e} dx {errs[1]:.3e} dW", [f"{e:.3e}" for e in errs[2:]])
    assert max(errs) <= C.CAP
    assert R.rel_err(emu[0], R.cin_literal(x.double(), [W.double() for W in Ws], bf16=True)) <= 1e-12


def test_cin_emu_passes_its_gradients_through_autograd():
    B, F0, D, sizes = 3, 5, 10, [6, 4]
    x, Ws, g = C.inputs(B, F0, D, sizes)
    xl = x.double().requires_grad_(True)
    Wl = [W.double().requires_grad_(True) for W in Ws]
    out = C.cin_emu(xl, Wl)
    (out * g.double()).sum().backward()
    eo, edx, edW = C.cin_bwd_emulated(x, Ws, g)
    assert torch.equal(out.detach(), eo) or R.rel_err(out.detach(), eo) <= 1e-12
    assert torch.equal(xl.grad, edx)
    for k in range(2):
        assert torch.equal(Wl[k].grad, edW[k])
