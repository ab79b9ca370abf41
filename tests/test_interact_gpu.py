"""FM, CrossNetwork and CIN on the GPU against the float64 restatements (tests/interact_ref.py), through the Python
layers and directly through the ABI with strided views.

Tolerances are measured, rel_err = max|got - want| / max|want|:
  FM, Cross: 8 x the error of the float32 CPU evaluation of the same restatement, floor 2^-20 (fusion_ref.bar; the GPU
             sums in another order);
  CIN:       4 x the error of the bf16-emulating restatement against float64 on the same inputs, floor 2^-20 (the
             kernel rounds where the emulation rounds; only the accumulation order differs).
Each test prints the bar it used.
"""
import ctypes

import pytest
import torch

import interact_ref as R
from recommendflow_amd.backend.layers import network_layers as N
from recommendflow_amd.runtime import lib as L

pytestmark = pytest.mark.gpu

FM_SHAPES = [(1, 1, 1), (3, 5, 10), (7, 39, 16), (4, 228, 128)]
CROSS_SHAPES = [(1, 1, 1), (3, 10, 2), (5, 257, 3), (4, 4100, 4), (2, 29184, 3)]
# [130, 3]: nine output tiles, two passes of the 64-row workgroup. The last three leave it (no room in LDS): 32 rows
# (two 260-wide layers in LDS; the field limit), 16 rows (two 512-wide layers, the width limit, two passes too)
CIN_SHAPES = [(1, 1, 1, [1]), (3, 5, 10, [6, 4]), (2, 7, 16, [8]), (4, 33, 24, [16, 16, 8]), (5, 40, 130, [20]),
              (70, 3, 8, [4]), (64, 64, 32, [64, 64]), (2, 5, 10, [130, 3]), (2, 8, 4, [260, 260, 4]), (1, 512, 3, [8]),
              (1, 8, 3, [512, 512, 4])]


def _check(name, got, want64, want32):
    tol = R.bar(want32, want64)
    err = R.rel_err(got, want64)
    print(f"{name}: rel_err {err:.3e} bar {tol:.3e}")
    assert err <= tol, (name, err, tol)


def _fm_case(B, fields, dim, seed=0):
    g = torch.Generator().manual_seed(seed)
    rows = 3 * fields + 5
    e = torch.randn(B, fields, dim, generator=g)
    ids = torch.randint(0, rows, (B, fields), generator=g)
    V = torch.randn(rows, dim, generator=g) * 0.5
    w = torch.randn(rows, 1, generator=g)
    w0 = torch.randn(1, generator=g)
    return e, ids, V, w, w0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("B,fields,dim", FM_SHAPES)
def test_fm_dense(cuda, B, fields, dim, first, dtype):
    e, ids, _, w, _ = _fm_case(B, fields, dim)
    e = e.to(dtype)
    # a view of a wider buffer: batch stride and field stride both larger than the packed ones
    buf = torch.zeros(B, fields + 1, dim + 3, dtype=dtype, device=cuda)
    buf[:, :fields, :dim] = e.to(cuda)
    xv = buf[:, :fields, :dim]
    got = N.fm_forward(embed=xv, w=w.to(cuda) if first else None, w_ids=ids.to(cuda) if first else None)
    again = N.fm_forward(embed=xv, w=w.to(cuda) if first else None, w_ids=ids.to(cuda) if first else None)
    assert got.shape == (B, 1) and torch.equal(got, again)
    wa = (w, ids) if first else (None, None)
    want64 = R.fm(e.double(), None, wa[0].double() if first else None, wa[1])
    want32 = R.fm(e.float(), None, wa[0], wa[1])
    _check(f"fm dense {B}x{fields}x{dim} {dtype} first={first}", got, want64, want32)


@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("B,fields,dim", FM_SHAPES)
def test_fm_gathered(cuda, B, fields, dim, first):
    _, ids, V, w, w0 = _fm_case(B, fields, dim, seed=1)
    idc = ids.to(cuda)
    kw = dict(w0=w0.to(cuda), w=w.to(cuda), w_ids=idc) if first else {}
    got = N.fm_forward(V=V.to(cuda), ids=idc, **kw)
    assert torch.equal(got, N.fm_forward(V=V.to(cuda), ids=idc, **kw))
    want64 = R.fm(V.double()[ids], w0.double() if first else None, w.double() if first else None, ids)
    want32 = R.fm(V[ids], w0 if first else None, w if first else None, ids)
    _check(f"fm gathered {B}x{fields}x{dim} first={first}", got, want64, want32)


def test_fm_out_of_range_id_is_nan(cuda):
    _, ids, V, _, _ = _fm_case(3, 5, 10)
    ids[1, 2] = V.shape[0]
    got = N.fm_forward(V=V.to(cuda), ids=ids.to(cuda)).cpu()
    assert torch.isnan(got[1, 0]) and not torch.isnan(got[0, 0]) and not torch.isnan(got[2, 0])


def test_fm_layers(cuda):
    cols = [{"feat_name": "a", "feat_num": 7, "embed_dim": 4}, {"feat_name": "b", "feat_num": 5, "embed_dim": 4},
            {"feat_name": "c", "feat_num": 11, "embed_dim": 4}]
    g = torch.Generator().manual_seed(3)
    inputs = {c["feat_name"]: torch.randint(0, c["feat_num"], (6,), generator=g) for c in cols}
    layer = N.FM_Layer(cols, k=10, seed=5)
    got = layer({k: v.to(cuda) for k, v in inputs.items()})
    assert got.shape == (6, 1) and layer.w0.shape == (1,) and layer.w.shape == (23, 1) and layer.V.shape == (23, 10)
    assert float(layer.w0) == 0.0 and 0.03 < float(layer.V.std()) < 0.07
    layer.w0.data.fill_(0.25)
    got = layer({k: v.to(cuda) for k, v in inputs.items()})
    ids = torch.stack([inputs["a"], inputs["b"] + 7, inputs["c"] + 12], dim=1)
    V, w, w0 = layer.V.data.cpu(), layer.w.data.cpu(), layer.w0.data.cpu()
    _check("FM_Layer", got, R.fm(V.double()[ids], w0.double(), w.double(), ids), R.fm(V[ids], w0, w, ids))
    with pytest.raises(ValueError, match="map dict error!"):
        layer({"zz": inputs["a"]})

    fm2 = N.New_FM(23, seed=6)
    e = torch.randn(6, 3, 10, generator=g)
    sparse = {"a": inputs["a"].reshape(-1, 1), "b": (inputs["b"] + 7).reshape(-1, 1), "c": (inputs["c"] + 12).reshape(-1, 1)}
    got = fm2({"sparse_inputs": {k: v.to(cuda) for k, v in sparse.items()}, "embed_inputs": e.to(cuda)})
    w = fm2.w.data.cpu()
    assert got.shape == (6, 1) and w.shape == (23, 1)
    _check("New_FM", got, R.fm(e.double(), None, w.double(), ids), R.fm(e, None, w, ids))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,dim,layers", CROSS_SHAPES)
def test_cross(cuda, B, dim, layers, dtype):
    g = torch.Generator().manual_seed(dim)
    x = torch.randn(B, dim, generator=g).to(dtype)
    net = N.CrossNetwork(layers, seed=2)
    # a view with a row stride wider than dim
    buf = torch.zeros(B, dim + 5, dtype=dtype, device=cuda)
    buf[:, :dim] = x.to(cuda)
    got = net(buf[:, :dim])
    assert got.shape == (B, dim) and got.dtype == torch.float32
    assert torch.equal(got, net(buf[:, :dim]))
    assert len(net.cross_weights) == layers and net.cross_weights[0].shape == (dim, 1)
    ws, bs = [w.cpu() for w in net.cross_weights], [b.cpu() for b in net.cross_bias]
    want64 = R.cross(x.double(), [w.double() for w in ws], [b.double() for b in bs])
    want32 = R.cross(x.float(), ws, bs)
    _check(f"cross {B}x{dim} L={layers} {dtype}", got, want64, want32)


def test_cross_zero_layers_returns_input(cuda):
    x = torch.randn(3, 10, device=cuda)
    assert N.CrossNetwork(0)(x) is x


_CIN_REF = {}


def _cin_ref(B, F0, D, sizes, dtype):
    """(x, Ws, float64 result, bf16-emulated result), computed once per case."""
    key = (B, F0, D, tuple(sizes), dtype)
    if key not in _CIN_REF:
        x, Ws = R.cin_inputs(B, F0, D, sizes, seed=F0 + D)
        x = x.to(dtype)
        xd, Wd = x.double(), [W.double() for W in Ws]
        _CIN_REF[key] = (x, Ws, R.cin_einsum(xd, Wd), R.cin_literal(xd, Wd, bf16=True))
    return _CIN_REF[key]


def _cin_layer(F0, sizes, Ws, cuda):
    layer = N.CIN(sizes)
    layer.build((None, F0, None))
    for i, W in enumerate(Ws):
        assert layer.cin_W[f"CIN_W_{i}"].shape == W.shape
        layer.cin_W[f"CIN_W_{i}"].data.copy_(W.to(cuda))
    layer.refresh()
    return layer


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,F0,D,sizes", CIN_SHAPES)
def test_cin(cuda, B, F0, D, sizes, dtype):
    x, Ws, want64, emu = _cin_ref(B, F0, D, sizes, dtype)
    layer = _cin_layer(F0, sizes, Ws, cuda)
    xc = x.to(cuda)
    got = layer(xc)
    assert got.shape == (B, sum(sizes)) and got.dtype == torch.float32
    assert torch.equal(got, layer(xc))
    tol = max(4.0 * R.rel_err(emu, want64), R.FLOOR)
    err = R.rel_err(got, want64)
    print(f"cin {B}x{F0}x{D} {sizes} {dtype}: rel_err {err:.3e} bar {tol:.3e} max|want| {float(want64.abs().max()):.3f}")
    assert err <= tol


def test_cin_strided_view_through_the_abi(cuda):
    """x as a [B, F0, D] view of a wider buffer (batch stride > F0 * D, field stride > D), out with ldo > sum H."""
    B, F0, D, sizes = 4, 33, 24, [16, 16, 8]
    x, Ws, want64, emu = _cin_ref(B, F0, D, sizes, torch.float32)
    layer = _cin_layer(F0, sizes, Ws, cuda)
    buf = torch.full((B, F0 * (D + 8) + 40), 7.0, device=cuda)
    xv = buf[:, : F0 * (D + 8)].view(B, F0, D + 8)[:, :, :D]
    xv.copy_(x.to(cuda))
    assert xv.stride() == (F0 * (D + 8) + 40, D + 8, 1)
    s = (ctypes.c_int32 * 3)(*sizes)
    lib = L.load()
    ws = torch.empty(int(lib.rf_cin_ws_bytes(B, F0, D, s, 3)), dtype=torch.uint8, device=cuda)
    out = torch.full((B, 48), -1.0, device=cuda)
    L.call("rf_cin_fwd", L.ptr(xv), L.DT_F32, xv.stride(0), xv.stride(1), B, F0, D, s, 3, L.ptr(layer._packed), L.ptr(out),
           out.stride(0), L.ptr(ws), ws.numel(), L.stream_ptr())
    tol = max(4.0 * R.rel_err(emu, want64), R.FLOOR)
    err = R.rel_err(out[:, :40], want64)
    print(f"cin strided: rel_err {err:.3e} bar {tol:.3e}")
    assert err <= tol
    assert torch.equal(out[:, :40], layer(x.to(cuda))) and bool((out[:, 40:] == -1.0).all())


def test_cin_lazy_build_and_state_dict(cuda):
    g = torch.Generator().manual_seed(9)
    x = (torch.rand(3, 5, 10, generator=g) * 2 - 1).to(cuda)
    a = N.CIN([6, 4], seed=1)
    ya = a(x)
    assert a.cin_W["CIN_W_0"].shape == (1, 25, 6) and a.cin_W["CIN_W_1"].shape == (1, 30, 4)
    assert 0.03 < float(a.cin_W["CIN_W_0"].std()) < 0.07
    b = N.CIN([6, 4], seed=2)
    assert not torch.equal(b(x), ya)
    b.load_state_dict(a.state_dict())
    assert torch.equal(b(x), ya)
    c = N.CIN([6, 4], seed=3)
    c.load_state_dict(a.state_dict())  # before the first call
    assert torch.equal(c(x), ya)
