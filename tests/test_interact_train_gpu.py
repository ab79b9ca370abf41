"""GPU: rf_fm_bwd, rf_cross_bwd and the trainable interaction layers against the float64 restatement
(tests/interact_train_ref.py: tests/interact_ref.py differentiated by torch CPU autograd).

Tolerance per tensor: rel_err = max|got - want| / max|want| <= 8 x the error of the float32 CPU evaluation of the same
restatement against float64 on the same inputs, floor 2^-20 (fusion_ref.bar). Each check prints the bar it used.
"""
import pytest
import torch

import interact_train_ref as T
from recommendflow_amd.backend.layers import network_layers as N
from recommendflow_amd.runtime import lib as L

pytestmark = pytest.mark.gpu

# (2, 9, 130): a lane's third column is a tail. (4, 228, 128): the workload's field count, where S is a long sum.
# Examples of 8192 padded elements and more, up to 32 fields per thread, take the register kernel: (3, 64, 128) is its
# first size (8 fields per thread; (3, 63, 128) is the wave kernel's last), (2, 100, 128) 16 per thread, (2, 70, 130)
# dim padded to 256, (1, 256, 128) its last size (32 per thread) and (1, 257, 128) back on the wave kernel
FM_SHAPES = [(1, 1, 1), (3, 5, 10), (7, 39, 16), (2, 9, 130), (4, 228, 128), (3, 63, 128), (3, 64, 128), (2, 100, 128),
             (2, 70, 130), (1, 256, 128), (1, 257, 128)]
# (2, 29184, 3): 1024 threads x 32 elements. (300, 20, 2): three batch chunks of 128, the last one partial
CROSS_SHAPES = [(1, 1, 1), (3, 10, 2), (5, 257, 3), (4, 4100, 4), (2, 29184, 3), (300, 20, 2)]


def _check(name, got, want64, want32):
    tol = T.bar(want32, want64)
    err = T.rel_err(got, want64)
    print(f"{name}: rel_err {err:.3e} bar {tol:.3e} (float32 CPU err {T.rel_err(want32, want64):.3e})")
    assert bool(torch.isfinite(got).all()) and err <= tol, (name, err, tol)


def _fm_case(B, fields, dim, seed=0):
    g = torch.Generator().manual_seed(seed)
    rows = 3 * fields + 5
    e = torch.randn(B, fields, dim, generator=g)
    ids = torch.randint(0, rows, (B, fields), generator=g)
    if fields > 1:
        ids[0, 1] = ids[0, 0]  # an id twice in one example
    V = torch.randn(rows, dim, generator=g) * 0.5
    w = torch.randn(rows, 1, generator=g)
    w0 = torch.randn(1, generator=g)
    gout = torch.randn(B, generator=g)
    return e, ids, V, w, w0, gout


def _fm_bwd_dense(xv, gout, dxv):
    B, fields, dim = xv.shape
    L.call("rf_fm_bwd", L.ptr(xv), L.torch_dtype_code(xv.dtype), xv.stride(0), xv.stride(1), None, None, 0, 0, B, fields, dim,
           L.ptr(gout), L.ptr(dxv), dxv.stride(0), dxv.stride(1), L.stream_ptr())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,fields,dim", FM_SHAPES)
def test_fm_bwd_dense(cuda, B, fields, dim, dtype):
    e, _, _, _, _, gout = _fm_case(B, fields, dim)
    e = e.to(dtype)
    # x and dx are views of wider buffers: batch and field strides both larger than the packed ones
    buf = torch.zeros(B, fields + 1, dim + 3, dtype=dtype, device=cuda)
    buf[:, :fields, :dim] = e.to(cuda)
    xv = buf[:, :fields, :dim]
    PAD = 777.0
    dbuf = torch.full((B, fields + 2, dim + 5), PAD, dtype=torch.float32, device=cuda)
    dxv = dbuf[:, :fields, :dim]
    gd = gout.to(cuda)
    _fm_bwd_dense(xv, gd, dxv)
    first = dbuf.clone()
    dbuf.fill_(PAD)
    _fm_bwd_dense(xv, gd, dxv)
    assert torch.equal(first, dbuf), "two launches differ"
    pad = dbuf.clone()
    pad[:, :fields, :dim] = PAD
    assert bool((pad == PAD).all()), "rf_fm_bwd wrote outside its [B, fields, dim] view"
    _, want64 = T.fm_grads(e, gout, torch.float64)
    _, want32 = T.fm_grads(e, gout, torch.float32)
    _check(f"fm_bwd dense {B}x{fields}x{dim} {dtype}", dxv, want64, want32)


@pytest.mark.parametrize("B,fields,dim", FM_SHAPES)
def test_fm_layer_gradients(cuda, B, fields, dim):
    """The gathered form plus rf_segment_sum_rows through TrainFMLayer: dV, dw, dw0. Tables of 3 * fields + 5 rows: ids
    repeat within and across examples."""
    _, ids, V, w, w0, gout = _fm_case(B, fields, dim, seed=1)
    rows = V.shape[0]
    # one feature per field; every field indexes the whole table (offset 0), so that an id can repeat inside an example
    cols = [{"feat_name": f"f{i}", "feat_num": rows if i == 0 else 0} for i in range(fields)]
    net = N.TrainFMLayer(cols, dim, w_reg=0.01, v_reg=0.02, device=cuda)
    net.map_dict = dict.fromkeys(net.map_dict, 0)
    net.build()
    with torch.no_grad():
        net.V.copy_(V.to(cuda))
        net.w.copy_(w.to(cuda))
        net.w0.copy_(w0.to(cuda))
    out = net({f"f{i}": ids[:, i].to(cuda) for i in range(fields)})
    (out[:, 0] * gout.to(cuda)).sum().backward()
    o64, dV64, dw64, dw064 = T.fm_layer_grads(V, w, w0, ids, gout, torch.float64)
    o32, dV32, dw32, dw032 = T.fm_layer_grads(V, w, w0, ids, gout, torch.float32)
    tag = f"fm layer {B}x{fields}x{dim}"
    _check(tag + " out", out, o64, o32)
    _check(tag + " dV", net.V.grad, dV64, dV32)
    _check(tag + " dw", net.w.grad, dw64, dw32)
    _check(tag + " dw0", net.w0.grad, dw064, dw032)
    untouched = torch.ones(rows, dtype=torch.bool)
    untouched[ids.reshape(-1)] = False
    assert bool((net.V.grad.cpu()[untouched] == 0).all()) and bool((net.w.grad.cpu()[untouched] == 0).all())


def test_fm_bwd_gathered_out_of_range_id(cuda):
    B, fields, dim = 3, 5, 12
    _, ids, V, _, _, gout = _fm_case(B, fields, dim, seed=2)
    ids[1, 2] = V.shape[0]  # one past the table
    idc, Vc, gd = ids.to(cuda), V.to(cuda), gout.to(cuda)
    pos = torch.zeros(B * fields, dim, device=cuda)
    L.call("rf_fm_bwd", None, L.DT_F32, 0, 0, L.ptr(Vc), L.ptr(idc), idc.stride(0), V.shape[0], B, fields, dim, L.ptr(gd),
           L.ptr(pos), fields * dim, dim, L.stream_ptr())
    pos = pos.view(B, fields, dim).cpu()
    assert bool(torch.isnan(pos[1]).all()), "the example with the bad id must be NaN"
    ok = [0, 2]
    _, want64 = T.fm_grads(V[ids[ok]], gout[ok], torch.float64)
    _, want32 = T.fm_grads(V[ids[ok]], gout[ok], torch.float32)
    _check("fm_bwd gathered, the other examples", pos[ok], want64, want32)


def _cross_case(B, dim, layers, dtype):
    g = torch.Generator().manual_seed(dim + layers)
    x = torch.randn(B, dim, generator=g).to(dtype)
    w = torch.randn(layers, dim, generator=g) * 0.05
    b = torch.randn(layers, dim, generator=g) * 0.05
    gout = torch.randn(B, dim, generator=g)
    return x, w, b, gout


_CROSS_REF = {}


def _cross_ref(B, dim, layers, dtype):
    key = (B, dim, layers, dtype)
    if key not in _CROSS_REF:
        x, w, b, gout = _cross_case(B, dim, layers, dtype)
        _CROSS_REF[key] = (T.cross_grads(x, w, b, gout, torch.float64), T.cross_grads(x, w, b, gout, torch.float32))
    return _CROSS_REF[key]


def _cross_bwd(xv, w, b, gv, dxv):
    B, dim = xv.shape
    layers = w.shape[0]
    dw, db = torch.full_like(w, 555.0), torch.full_like(b, 555.0)
    wsb = int(L.load().rf_cross_bwd_ws_bytes(B, dim, layers))
    ws = torch.empty(wsb, dtype=torch.uint8, device=xv.device)
    L.call("rf_cross_bwd", L.ptr(xv), L.torch_dtype_code(xv.dtype), xv.stride(0), B, dim, layers, L.ptr(w), L.ptr(b),
           L.ptr(gv), gv.stride(0), L.ptr(dxv), dxv.stride(0), L.ptr(dw), L.ptr(db), L.ptr(ws), wsb, L.stream_ptr())
    return dw, db


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,dim,layers", CROSS_SHAPES)
def test_cross_bwd(cuda, B, dim, layers, dtype):
    x, w, b, gout = _cross_case(B, dim, layers, dtype)
    # row strides wider than dim, each its own
    xb = torch.zeros(B, dim + 5, dtype=dtype, device=cuda)
    xb[:, :dim] = x.to(cuda)
    gb = torch.zeros(B, dim + 3, device=cuda)
    gb[:, :dim] = gout.to(cuda)
    PAD = 777.0
    dxb = torch.full((B, dim + 7), PAD, device=cuda)
    wd, bd = w.to(cuda), b.to(cuda)
    dw, db = _cross_bwd(xb[:, :dim], wd, bd, gb[:, :dim], dxb[:, :dim])
    first = dxb.clone()
    dxb.fill_(PAD)
    dw2, db2 = _cross_bwd(xb[:, :dim], wd, bd, gb[:, :dim], dxb[:, :dim])
    assert torch.equal(first, dxb) and torch.equal(dw, dw2) and torch.equal(db, db2), "two launches differ"
    assert bool((dxb[:, dim:] == PAD).all()), "rf_cross_bwd wrote outside its rows"
    (_, dx64, dw64, db64), (_, dx32, dw32, db32) = _cross_ref(B, dim, layers, dtype)
    tag = f"cross_bwd {B}x{dim} L={layers} {dtype}"
    _check(tag + " dx", dxb[:, :dim], dx64, dx32)
    _check(tag + " dw", dw, dw64, dw32)
    _check(tag + " db", db, db64, db32)


def test_train_cross_network_autograd(cuda):
    B, dim, layers = 5, 257, 3
    x, w, b, gout = _cross_case(B, dim, layers, torch.float32)
    net = N.TrainCrossNetwork(layers, reg_w=0.03, reg_b=0.07, device=cuda)
    net.build((None, dim))
    with torch.no_grad():
        net.w.copy_(w.to(cuda))
        net.b.copy_(b.to(cuda))
    xd = x.to(cuda).requires_grad_(True)
    right = torch.randn(B, 6, device=cuda, requires_grad=True)
    out = net(xd, concat=right)
    assert out.shape == (B, dim + 6) and torch.equal(out[:, dim:], right)
    gfull = torch.cat([gout.to(cuda), torch.ones(B, 6, device=cuda)], dim=1)
    (out * gfull).sum().backward()
    (o64, dx64, dw64, db64), (o32, dx32, dw32, db32) = _cross_ref(B, dim, layers, torch.float32)
    _check("TrainCrossNetwork out", out[:, :dim], o64, o32)
    _check("TrainCrossNetwork dx", xd.grad, dx64, dx32)
    _check("TrainCrossNetwork dw", net.w.grad, dw64, dw32)
    _check("TrainCrossNetwork db", net.b.grad, db64, db32)
    assert torch.equal(right.grad, torch.ones_like(right))
    # the inference layer computes the same forward
    ref = N.CrossNetwork(layers, device=cuda)
    ref.build((None, dim))
    ref.w.data.copy_(net.w.data)
    ref.b.data.copy_(net.b.data)
    assert torch.equal(ref(x.to(cuda)), out[:, :dim].detach())


def test_train_cross_network_zero_layers_passes_the_gradient_through(cuda):
    x = torch.randn(3, 10, device=cuda, requires_grad=True)
    g = torch.randn(3, 10, device=cuda)
    out = N.TrainCrossNetwork(0, device=cuda)(x)
    (out * g).sum().backward()
    assert torch.equal(x.grad, g)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_train_new_fm_autograd(cuda, dtype):
    B, fields, dim = 7, 39, 16
    e, ids, _, w, _, gout = _fm_case(B, fields, dim, seed=3)
    e = e.to(dtype)
    rows = w.shape[0]
    net = N.TrainNewFM(rows, w_reg=0.05, device=cuda)
    net.build()
    with torch.no_grad():
        net.w.copy_(w.to(cuda))
    # the encoder's [B, S * 2D] output viewed as [B, S, 2D]
    flat = e.reshape(B, fields * dim).to(cuda).requires_grad_(True)
    out = net({"sparse_inputs": {"a": ids[:, :20].to(cuda), "b": ids[:, 20:].to(cuda)}, "embed_inputs": flat.view(B, fields, dim)})
    (out[:, 0] * gout.to(cuda)).sum().backward()
    o64, de64, dw64 = T.new_fm_grads(e, w, ids, gout, torch.float64)
    o32, de32, dw32 = T.new_fm_grads(e, w, ids, gout, torch.float32)
    _check(f"TrainNewFM out {dtype}", out, o64, o32)
    assert flat.grad.dtype == dtype and flat.grad.shape == (B, fields * dim)
    if dtype == torch.bfloat16:
        # the kernel's f32 gradient is rounded once to the input's dtype (autograd's contract). Against the float64
        # gradient rounded the same way the two can differ by one bf16 ulp where the f32 error crosses a rounding
        # boundary: 2^-7 of the element (8 significand bits), so at most 2^-7 of max|want|
        want = de64.float().to(dtype).double()
        err = T.rel_err(flat.grad.view(B, fields, dim), want)
        print(f"TrainNewFM d embed bf16: rel_err {err:.3e} bar {2.0 ** -7:.3e}")
        assert err <= 2.0 ** -7
    else:
        _check("TrainNewFM d embed", flat.grad.view(B, fields, dim), de64, de32)
    _check(f"TrainNewFM dw {dtype}", net.w.grad, dw64, dw32)
    # no first order: no w, and the same second-order gradient
    flat2 = e.reshape(B, fields * dim).to(cuda).requires_grad_(True)
    out2 = N.TrainNewFM(0, device=cuda)({"embed_inputs": flat2.view(B, fields, dim)})
    (out2[:, 0] * gout.to(cuda)).sum().backward()
    assert torch.equal(flat2.grad, flat.grad)


def test_regularization(cuda):
    """Keras l2(c): c * sum(w^2), gradient 2 c w."""
    cross = N.TrainCrossNetwork(2, reg_w=0.03, reg_b=0.07, device=cuda)
    cross.build((None, 9))
    fm = N.TrainFMLayer([{"feat_name": "a", "feat_num": 11}], 4, w_reg=0.01, v_reg=0.02, device=cuda)
    fm.build()
    nfm = N.TrainNewFM(13, w_reg=0.05, device=cuda)
    nfm.build()
    for net, terms in ((cross, [(0.03, "w"), (0.07, "b")]), (fm, [(0.01, "w"), (0.02, "V")]), (nfm, [(0.05, "w")])):
        r = net.regularization()
        want = sum(c * float((getattr(net, n).detach().double() ** 2).sum()) for c, n in terms)
        assert abs(float(r.detach()) - want) <= 1e-6 * want, (type(net).__name__, float(r.detach()), want)
        r.backward()
        for c, n in terms:
            p = getattr(net, n)
            assert torch.allclose(p.grad, 2 * c * p.detach(), rtol=1e-6, atol=0), (type(net).__name__, n)
    assert fm.w0.grad is None  # w0 has no regularizer in the reference


def test_inference_layers_stay_frozen(cuda):
    net = N.CrossNetwork(2, device=cuda)
    net.build((None, 8))
    assert not net.w.requires_grad and not hasattr(net, "regularization")
