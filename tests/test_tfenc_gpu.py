"""rf_tfenc_fwd / TransformerEncoder on the GPU against the float64 restatement (tests/tfenc_ref.py), through
transformer_encoder_stack and directly through the ABI with strided views.

Tolerance (the CIN convention): rel_err = max|got - want64| / max|want64|; bar = 4 x the error of the bf16-emulating
restatement against float64 on the same inputs, floor 2^-20, and never above 2^-5 (the kernel rounds where the emulation
rounds; the accumulation order, exp and the reciprocal differ). Every case prints its error and its bar.
"""
import pytest
import torch

import tfenc_ref as R
from recommendflow_amd.backend.layers import network_layers as N
from recommendflow_amd.runtime import lib as L

pytestmark = pytest.mark.gpu

_KERNELS = (("wq", "Wq", "bq"), ("wk", "Wk", "bk"), ("wv", "Wv", "bv"), ("conv1", "W1", "b1"), ("conv2", "W2", "b2"))


def _blocks(params, d, heads, ffn, cuda):
    """TransformerEncoder modules holding the given parameters (Dense keeps its kernel as [out][in])."""
    out = []
    for P in params:
        blk = N.TransformerEncoder(d, num_heads=heads, ffn_hidden_unit=ffn, layer_norm_eps=R.EPS)
        for name, W, b in _KERNELS:
            getattr(blk, name + "_kernel").copy_(P[W].t().to(cuda))
            getattr(blk, name + "_bias").copy_(P[b].to(cuda))
        for n, g, be in ((1, "g1", "be1"), (2, "g2", "be2")):
            getattr(blk, f"ln{n}_gamma").copy_(P[g].to(cuda))
            getattr(blk, f"ln{n}_beta").copy_(P[be].to(cuda))
        blk.refresh()
        out.append(blk)
    return out


def _abi_strided(blocks, x, mask, case, cuda):
    """The ABI with x a view of a wider buffer (both strides larger than packed, nothing 16-byte aligned) and out a row
    and column slice of a wider buffer. Returns (the out view, the whole buffer)."""
    B, Ln, d, heads, ffn, nb = case
    xb = torch.full((B, Ln + 1, d + 3), 9.0, dtype=x.dtype, device=cuda)
    xv = xb[:, :Ln, :d]
    xv.copy_(x.to(cuda))
    assert xv.stride() == ((Ln + 1) * (d + 3), d + 3, 1)
    ob = torch.full((B, Ln + 2, d + 5), -7.0, device=cuda)
    ov = ob[:, 1: Ln + 1, 3: 3 + d]
    m = None if mask is None else mask.to(cuda).contiguous()
    packed = blocks[0]._stack[1]
    L.call("rf_tfenc_fwd", L.ptr(xv), L.torch_dtype_code(x.dtype), xv.stride(0), xv.stride(1), L.ptr(m), B, Ln, d, heads, ffn,
           nb, L.ptr(packed), R.EPS, L.ptr(ov), ov.stride(0), ov.stride(1), L.stream_ptr())
    return ov, ob


def _run_case(cuda, case, dtype, masked, scale=1.0):
    B, Ln, d, heads, ffn, nb = case
    x, params, mask, want, _, bar = R.reference(case, dtype, masked, scale)
    assert bar <= R.CAP
    blocks = _blocks(params, d, heads, ffn, cuda)
    xc = x.to(cuda)
    mc = None if mask is None else mask.to(cuda)
    got = N.transformer_encoder_stack(blocks, xc, mc)
    assert got.shape == (B, Ln, d) and got.dtype == torch.float32
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, N.transformer_encoder_stack(blocks, xc, None if mc is None else mc.unsqueeze(2)))
    err = R.rel_err(got.cpu().double(), want)
    ov, ob = _abi_strided(blocks, x, mask, case, cuda)
    err_abi = R.rel_err(ov.cpu().double(), want)
    print(f"tfenc {case} {dtype} masked={masked} scale={scale}: rel_err {err:.3e} (abi, strided {err_abi:.3e}) bar {bar:.3e}")
    assert err <= bar and err_abi <= bar
    # vector or scalar loads and stores: the same arithmetic
    assert torch.equal(ov, got)
    # nothing outside the view is written
    ob[:, 1: Ln + 1, 3: 3 + d] = -7.0
    assert bool((ob == -7.0).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("case", R.CASES)
def test_tfenc(cuda, case, masked, dtype):
    _run_case(cuda, case, dtype, masked)


def test_large_logits_stay_finite(cuda):
    """x scaled by 30: logits of several hundred; the softmax subtracts the row maximum."""
    _run_case(cuda, R.SCALED_CASE, torch.float32, True, scale=30.0)


def test_masked_rows_attention_term(cuda):
    """One block with W1 = W2 = 0, zero FFN biases and identity LayerNorm parameters: out = LN(LN(x + att)), so the
    masked query rows check the attention term (the mean of v over exactly L keys) on its own."""
    B, Ln, d, heads, ffn = 3, 5, 32, 2, 48
    x, params, mask = R.inputs(B, Ln, d, heads, ffn, 1, seed=4)
    P = params[0]
    for n in ("W1", "W2", "b1", "b2", "be1", "be2"):
        P[n].zero_()
    P["g1"].fill_(1.0)
    P["g2"].fill_(1.0)
    want = R.encoder(x.double(), R.cast(params, torch.float64), mask, heads, R.EPS)
    emu = R.encoder(x, params, mask, heads, R.EPS, bf16=True)
    got = N.transformer_encoder_stack(_blocks(params, d, heads, ffn, cuda), x.to(cuda), mask.to(cuda)).cpu().double()
    rows = mask == 0
    assert int(rows.sum()) >= Ln
    bar = max(4.0 * R.rel_err(emu[rows], want[rows]), R.FLOOR)
    err = R.rel_err(got[rows], want[rows])
    print(f"masked rows: rel_err {err:.3e} bar {bar:.3e}")
    assert err <= bar <= R.CAP
    # a mean over the 16 rows of the padded tile instead of the 5 keys would be off by O(1)
    att, v, _ = R.block(x.double(), R.cast(params, torch.float64)[0], mask, heads, R.EPS, parts=True)
    assert R.rel_err(att[rows], v.mean(dim=1, keepdim=True).expand_as(att)[rows]) <= 1e-12


def test_layer_equals_stack_of_one_and_out_view(cuda):
    case = (3, 5, 32, 2, 48, 1)
    x, params, mask, want, _, bar = R.reference(case, torch.float32, True)
    (blk,) = _blocks(params, 32, 2, 48, cuda)
    xc, mc = x.to(cuda), mask.to(cuda)
    y = blk([xc, mc])
    assert torch.equal(y, N.transformer_encoder_stack([blk], xc, mc))
    assert R.rel_err(y.cpu().double(), want) <= bar
    # the fused encoder's [B, S * 2D] output read in place, the result landed in a concat buffer
    flat = xc.reshape(3, 5 * 32)
    cat = torch.full((3, 5, 32 + 8), -1.0, device=cuda)
    r = blk([flat.view(3, 5, 32), mc.unsqueeze(2)], out=cat[:, :, :32])
    assert r.data_ptr() == cat.data_ptr() and torch.equal(cat[:, :, :32], y) and bool((cat[:, :, 32:] == -1.0).all())
    with pytest.raises(ValueError):
        blk([xc, mc], out=torch.empty(3, 5, 16, device=cuda))


def test_state_dict_and_refresh(cuda):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 9, 32, generator=g).to(cuda)
    a = N.TransformerEncoder(32, num_heads=2, ffn_hidden_unit=64, seed=1)
    b = N.TransformerEncoder(32, num_heads=2, ffn_hidden_unit=64, seed=2)
    # Glorot kernels, zero biases, gamma one, beta zero
    lim = (6.0 / (32 + 64)) ** 0.5
    assert a.conv1_kernel.shape == (64, 32) and 0.9 * lim < float(a.conv1_kernel.abs().max()) <= lim
    assert float(a.wq_bias.abs().max()) == 0 and float(a.conv2_bias.abs().max()) == 0
    assert bool((a.ln1_gamma == 1).all()) and bool((a.ln2_beta == 0).all())
    assert a.mha.wq.weight.dtype == torch.float32 and a.ffn.conv1.weight is a.conv1_kernel
    ya, yb = a([x, None]), b([x, None])
    assert not torch.equal(ya, yb)
    b.load_state_dict(a.state_dict())
    assert torch.equal(b([x, None]), ya)
    # an in-place change of a master weight reaches the kernel after refresh()
    b.ln2_beta.add_(0.5)
    assert torch.equal(b([x, None]), ya)
    b.refresh()
    y2 = b([x, None])
    assert not torch.equal(y2, ya)
    assert float((y2 - ya - 0.5).abs().max()) < 1e-5
    # FFN on its own is the two Dense layers
    h = torch.relu(x.reshape(-1, 32) @ a.conv1_kernel.t() + a.conv1_bias)
    want = (h @ a.conv2_kernel.t() + a.conv2_bias).reshape(2, 9, 32)
    assert float((a.ffn(x) - want).abs().max()) < 1e-4


def test_batch_zero_and_unequal_blocks(cuda):
    a = N.TransformerEncoder(32, num_heads=2, ffn_hidden_unit=64)
    y = a([torch.empty(0, 7, 32, device=cuda), None])
    assert y.shape == (0, 7, 32)
    packed = a._stack[1]
    assert L.load().rf_tfenc_fwd(None, L.DT_F32, 7 * 32, 32, None, 0, 7, 32, 2, 64, 1, L.ptr(packed), 1e-6, None, 7 * 32, 32,
                                 None) == L.RF_OK
    x = torch.zeros(1, 7, 32, device=cuda)
    for other in (N.TransformerEncoder(32, num_heads=1, ffn_hidden_unit=64), N.TransformerEncoder(32, num_heads=2, ffn_hidden_unit=32),
                  N.TransformerEncoder(32, num_heads=2, ffn_hidden_unit=64, layer_norm_eps=1e-3)):
        with pytest.raises(ValueError):
            N.transformer_encoder_stack([a, other], x)
    with pytest.raises(ValueError):
        N.transformer_encoder_stack([N.TransformerEncoder(64, num_heads=2, ffn_hidden_unit=64)], x)
