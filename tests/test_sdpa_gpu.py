"""rf_sdpa_fwd (sdpa_kernel) on the GPU against the float64 restatement (tests/sdpa_ref.py), through
scaled_dot_product_attention, MultiHeadAttention and directly through the ABI, at the kernel's tile, LDS and mask edges.

Tolerance (the CIN / TransformerEncoder convention): rel_err = max|got - want64| / max|want64|; bar = 4 x the error of
the restatement that rounds the probabilities to fp16 / bf16 against float64 on the same inputs, floor 2^-20, and never
above 2^-8 (fp16) / 2^-5 (bf16). Every case prints its error and its bar. What must be the same arithmetic (a second
launch, a masked row and a zero query row, one head's slice on its own, a view and its copy) is compared bit for bit.
"""
import pytest
import torch

import sdpa_ref as R
from oracle import oracle as O
from recommendflow_amd.backend.layers.attention_layers import MultiHeadAttention
from recommendflow_amd.backend.layers.layer_utils import scaled_dot_product_attention
from recommendflow_amd.runtime import lib as L

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]


def _gpu(case, dtype, masked, cuda, scale=1.0):
    """The case's inputs on the GPU, its reference and the result of the plain call."""
    q, k, v, mask, want, _, bar = R.reference(case, dtype, masked, scale)
    assert bar <= R.CAP[dtype]
    qc, kc, vc = q.to(cuda), k.to(cuda), v.to(cuda)
    mc = None if mask is None else mask.to(cuda)
    got = scaled_dot_product_attention(qc, kc, vc, mc, heads=case[1], dtype=dtype)
    return qc, kc, vc, mc, got, want, bar


def _run_case(cuda, case, dtype, masked, scale=1.0):
    B, heads, Lq, Lk, depth = case
    qc, kc, vc, mc, got, want, bar = _gpu(case, dtype, masked, cuda, scale)
    assert got.shape == (B, Lq, heads * depth) and got.dtype == torch.float32
    assert bool(torch.isfinite(got).all())
    err = R.rel_err(got, want)
    print(f"sdpa {case} {dtype} masked={masked} scale={scale}: rel_err {err:.3e} bar {bar:.3e} ratio {err / bar:.3f}")
    assert err <= bar
    assert torch.equal(got, scaled_dot_product_attention(qc, kc, vc, mc, heads=heads, dtype=dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("case", R.CASES)
def test_sdpa(cuda, case, masked, dtype):
    _run_case(cuda, case, dtype, masked)


@pytest.mark.parametrize("dtype", DTYPES)
def test_large_logits(cuda, dtype):
    """q and k scaled by 6: logits in the hundreds, nearly one-hot softmaxes; the kernel subtracts the row maximum."""
    _run_case(cuda, R.SCALED_CASE, dtype, True, scale=R.SCALE)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [(2, 3, 5, 5, 32), (2, 1, 65, 31, 128)])
def test_masked_rows_equal_zero_query_rows(cuda, case, dtype):
    """A masked row and a zero query row are both a uniform softmax, exp(0) over the same Lk keys through the same
    instructions: equal bits, and the mean of v over exactly Lk keys (a mean over the padded tile is off by O(1))."""
    B, heads, Lq, Lk, depth = case
    qc, kc, vc, mc, got, _, bar = _gpu(case, dtype, True, cuda)
    rows = mc == 0
    assert int(rows[0].sum()) == Lq and int(rows.sum()) >= Lq
    qz = qc.clone()
    qz[rows] = 0
    zero = scaled_dot_product_attention(qz, kc, vc, None, heads=heads, dtype=dtype)
    assert torch.equal(got[rows], zero[rows])
    assert torch.equal(got, zero)  # the other rows do not see the mask at all
    mean = vc.double().mean(dim=1, keepdim=True).expand(B, Lq, heads * depth)
    err = R.rel_err(got[rows], mean[rows])
    print(f"masked rows {case} {dtype}: rel_err to mean(v) {err:.3e} bar {bar:.3e}")
    assert err <= bar


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [(70, 2, 8, 8, 32), (2, 3, 5, 5, 32)])
def test_head_and_example_slices_are_independent(cuda, case, dtype):
    """One (example, head) on its own, as a heads = 1, B = 1 call on contiguous copies: the same depth, Lq and Lk, so
    the same arithmetic. Any difference is an addressing error."""
    B, heads, Lq, Lk, depth = case
    qc, kc, vc, mc, got, _, _ = _gpu(case, dtype, True, cuda)
    for b, h in {(0, 0), (0, heads - 1), (B // 2, 0), (B - 1, 0), (B - 1, heads - 1)}:
        cols = slice(h * depth, (h + 1) * depth)
        one = scaled_dot_product_attention(qc[b: b + 1, :, cols].contiguous(), kc[b: b + 1, :, cols].contiguous(),
                                           vc[b: b + 1, :, cols].contiguous(), mc[b: b + 1], heads=1, dtype=dtype)
        assert one.shape == (1, Lq, depth)
        assert torch.equal(got[b, :, cols], one[0]), (b, h)


@pytest.mark.parametrize("dtype", DTYPES)
def test_mask_shapes_and_views(cuda, dtype):
    case = (2, 2, 17, 16, 64)
    qc, kc, vc, mc, got, _, _ = _gpu(case, dtype, True, cuda)
    assert torch.equal(got, scaled_dot_product_attention(qc, kc, vc, mc.unsqueeze(2), heads=2, dtype=dtype))
    qv = qc.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    assert not qv.is_contiguous() and torch.equal(qv, qc)
    assert torch.equal(got, scaled_dot_product_attention(qv, kc, vc, mc, heads=2, dtype=dtype))


def _middle(t, fill):
    """t's rows as the middle of a buffer one row longer at either end, filled with `fill`: a contiguous view that is one
    row (a multiple of 16 bytes) off the allocation's start. -> (the view, the whole buffer)."""
    rows = t.reshape(-1, t.shape[-1])
    buf = torch.full((rows.shape[0] + 2, rows.shape[1]), fill, dtype=t.dtype, device=t.device)
    view = buf[1: 1 + rows.shape[0]]
    view.copy_(rows)
    assert view.is_contiguous() and view.data_ptr() % 16 == 0 and view.data_ptr() != buf.data_ptr()
    return view, buf


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [(2, 2, 17, 16, 64), (1, 2, 7, 255, 32), (2, 3, 5, 5, 32)])
def test_nothing_outside_the_tensors_is_read_or_written(cuda, case, dtype):
    """The ABI with q, k and v each the middle of a buffer of NaN and out the middle of a buffer of a sentinel. A v row
    read past Lk would put NaN into every output; a write past a tensor's end would change a sentinel."""
    B, heads, Lq, Lk, depth = case
    qc, kc, vc, mc, got, _, _ = _gpu(case, dtype, True, cuda)
    w = heads * depth
    (qv, _), (kv, _), (vv, _) = (_middle(t, float("nan")) for t in (qc, kc, vc))
    ob = torch.full((B * Lq + 2, w), -7.0, device=cuda)
    ov = ob[1: 1 + B * Lq]
    assert ov.data_ptr() % 16 == 0
    L.call("rf_sdpa_fwd", L.ptr(qv), L.ptr(kv), L.ptr(vv), L.torch_dtype_code(dtype), B, heads, Lq, Lk, depth,
           L.ptr(mc.contiguous()), L.ptr(ov), L.stream_ptr())
    assert bool(torch.isfinite(ov).all())
    assert torch.equal(ov.reshape(B, Lq, w), got)
    ov.fill_(-7.0)
    assert bool((ob == -7.0).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_multi_head_attention_cross_lengths(cuda, dtype):
    """MultiHeadAttention with Lq != Lk and in_features != d_model against the float64 oracle. The projections are exact
    fp32, so the bar is the emulation's: the float64 projections rounded to `dtype`, then the restatement."""
    B, Lq, Lk, d_in, d_model, heads = 3, 9, 21, 40, 64, 2
    g = torch.Generator().manual_seed(Lq + Lk + d_in)
    q = torch.randn(B, Lq, d_in, generator=g)
    k, v = torch.randn(B, Lk, d_in, generator=g), torch.randn(B, Lk, d_in, generator=g)
    mask = torch.tensor(R.MASK_VALUES)[torch.randint(0, len(R.MASK_VALUES), (B, Lq, 1), generator=g)]
    mask[0] = 0.0
    mask[-1] = 1.0
    mha = MultiHeadAttention(d_model, heads, dtype=dtype, seed=2, in_features=d_in)
    layers = (mha.wq, mha.wk, mha.wv)
    for dl in layers:
        dl.bias.copy_(torch.randn(d_model, generator=g).to(cuda) * 0.1)
    P = [(dl.weight.cpu().double().t(), dl.bias.cpu().double()) for dl in layers]  # kernels as [in, d_model]
    qp, kp, vp = ((x.double() @ W + b).to(dtype) for x, (W, b) in zip((q, k, v), P))
    args = [a for W, b in P for a in (W.numpy(), b.numpy())]
    for m in (mask, None):
        want = torch.from_numpy(O.multi_head_attention(q.numpy(), k.numpy(), v.numpy(), None if m is None else m.numpy(),
                                                       *args, heads))
        emu = R.sdpa(qp.float(), kp.float(), vp.float(), m, heads, round_p=dtype)
        bar = R.bar_of(emu, want)
        got = mha.call(q.to(cuda), k.to(cuda), v.to(cuda), None if m is None else m.to(cuda))
        assert got.shape == (B, Lq, d_model) and got.dtype == torch.float32
        err = R.rel_err(got, want)
        print(f"mha Lq {Lq} Lk {Lk} {dtype} masked={m is not None}: rel_err {err:.3e} bar {bar:.3e} ratio {err / bar:.3f}")
        assert err <= bar <= R.CAP[dtype]
        if m is not None:  # example 0: every row is the mean of the projected v over exactly Lk keys
            mean = (v[0].double() @ P[2][0] + P[2][1]).mean(dim=0)
            assert R.rel_err(got[0], mean.expand(Lq, d_model)) <= bar


def test_refused_shapes_raise(cuda):
    """Argument checks, so nothing is launched; a valid call after each still returns the right result."""
    case, dtype = (2, 3, 5, 5, 32), torch.float16
    qc, kc, vc, mc, got, want, bar = _gpu(case, dtype, True, cuda)
    z = lambda *shape: torch.zeros(shape, device=cuda)  # noqa: E731
    for (Lq, Lk, w, heads), name in (((4, 257, 32, 1), "Lk"), ((4, 8, 48, 1), "depth"), ((4, 256, 128, 1), "LDS"),
                                     ((4, 8, 64, 3), "divisible")):
        with pytest.raises(ValueError, match=name):
            scaled_dot_product_attention(z(1, Lq, w), z(1, Lk, w), z(1, Lk, w), None, heads=heads, dtype=dtype)
        again = scaled_dot_product_attention(qc, kc, vc, mc, heads=case[1], dtype=dtype)
        assert torch.equal(again, got) and R.rel_err(again, want) <= bar
    # the largest accepted shape at depth 128 beside the refused one
    out = scaled_dot_product_attention(z(1, 4, 128), z(1, 224, 128), z(1, 224, 128), None, heads=1, dtype=dtype)
    assert float(out.abs().max()) == 0.0
