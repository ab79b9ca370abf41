"""TransformerEncoder training without a GPU: the float64 restatement (tests/tfenc_train_ref.py) on its own relu pattern
equals torch autograd through torch's own layer_norm / softmax / matmul; every GPU case meets the seed conditions (every
bar under the cap, min|pre| of the emulation at least 2^-16); dbk of the reference is zero; the new entry points are
exported; every limit is refused with its argument named before any HIP call."""
import ctypes
import math

import pytest
import torch

import tfenc_ref as R
import tfenc_train_ref as T
from recommendflow_amd.runtime import lib as L


def _torch_block(x, P, mask, heads, eps):
    F = torch.nn.functional
    B, Ln, d = x.shape
    depth = d // heads
    q, k, v = (x @ P["W" + n] + P["b" + n] for n in "qkv")
    sp = lambda t: t.view(B, Ln, heads, depth).transpose(1, 2)  # noqa: E731
    logits = sp(q) @ sp(k).transpose(-1, -2) / math.sqrt(depth)
    if mask is not None:
        logits = logits.masked_fill(mask.view(B, 1, Ln, 1) == 0, -4294967295.0)
    att = (F.softmax(logits, dim=-1) @ sp(v)).transpose(1, 2).reshape(B, Ln, d)
    out1 = F.layer_norm(x + att, (d,), P["g1"], P["be1"], eps)
    ffn = F.relu(out1 @ P["W1"] + P["b1"]) @ P["W2"] + P["b2"]
    return F.layer_norm(out1 + ffn, (d,), P["g2"], P["be2"], eps)


@pytest.mark.parametrize("masked", [False, True])
def test_restatement_gradients_match_torch_composition(masked):
    B, Ln, d, heads, ffn, blocks = 3, 7, 32, 2, 48, 2
    x, params, mask = R.inputs(B, Ln, d, heads, ffn, blocks, seed=1)
    mask = mask if masked else None
    g = torch.randn(B, Ln, d, generator=torch.Generator().manual_seed(2))
    got, pats, lo, _ = T.grads(x, params, mask, g, heads, torch.float64)
    xl = x.double().requires_grad_(True)
    Ps = [{n: t.double().requires_grad_(True) for n, t in P.items()} for P in params]
    y = xl
    for P in Ps:
        y = _torch_block(y, P, None if mask is None else mask.double(), heads, R.EPS)
    (y * g.double()).sum().backward()
    want = {"dx": xl.grad}
    for i, P in enumerate(Ps):
        for n in T.PARAMS:
            want[f"{i}.{n}"] = P[n].grad
    for n in want:
        if n.endswith(".bk"):
            assert float(got[n].abs().max()) <= 1e-12 * float(want[n[:-2] + "bq"].abs().max())
            continue
        err = R.rel_err(got[n], want[n])
        assert err <= 1e-10, (n, err)
    # the shared pattern of the same run reproduces it
    again, _, _, _ = T.grads(x, params, mask, g, heads, torch.float64, gates=pats)
    assert all(torch.equal(again[n], got[n]) for n in got)


@pytest.mark.parametrize("dtype,masked", T.VARIANTS)
@pytest.mark.parametrize("case", T.CASES)
def test_seed_conditions(case, dtype, masked):
    ref = T.reference(case, dtype, masked)
    worst = max(ref["bars"], key=ref["bars"].get)
    print(f"{case} {dtype} masked={masked}: seed {T.SEEDS[case]} worst bar {worst} {ref['bars'][worst]:.3e} "
          f"min|pre| {ref['min_pre']:.3e}")
    assert ref["bars"][worst] <= T.CAP
    assert ref["min_pre"] >= T.MIN_PRE
    L_ = case[1]
    for n, w in ref["want"].items():
        if n.endswith(".bk"):
            assert float(w.abs().max()) <= 1e-12 * max(float(ref["want"][n[:-2] + "bq"].abs().max()), 1e-300) or L_ == 1
            # the emulation's own noise is far below the bound the kernel gets
            assert float(ref["emu"][n].abs().max()) <= T.zero_bound(ref, n, L_)
    if L_ == 1:
        for n in ("0.Wq", "0.Wk", "0.bq", "0.bk"):
            assert float(ref["want"][n].abs().max()) == 0.0


def test_symbols_and_layers_exported():
    lib = L.load()
    for s in ("rf_tfenc_bwd", "rf_tfenc_bwd_pack", "rf_tfenc_bwd_packed_bytes", "rf_tfenc_bwd_ws_bytes"):
        assert s in L.EXPORTED and hasattr(lib, s), s
    from recommendflow_amd.backend.layers import network_layers as N
    from recommendflow_amd.models import ranking

    for s in ("TrainTransformerEncoder", "train_transformer_encoder_stack"):
        assert hasattr(N, s), s
    assert "TrainableTabTransformer" in ranking.__all__


def _bwd(lib, L_=8, d=32, heads=2, ffn=32, blocks=1, dtype=L.DT_F32, batch=1, packed_t=16, ws=16, ws_bytes=None, grads=True,
         dx=1 << 20, dout=1 << 30, xsl=None, dosl=None, dxsl=None, eps=1e-6):
    """Fake device pointers: every refusal precedes any HIP call."""
    n = 14 * max(blocks, 1)
    g = (ctypes.c_void_p * n)(*([16] * n)) if grads is True else grads
    if ws_bytes is None:
        ws_bytes = 1 << 40
    return lib.rf_tfenc_bwd(16, dtype, L_ * d, d if xsl is None else xsl, None, batch, L_, d, heads, ffn, blocks, 16, packed_t, eps,
                            dout, L_ * d, d if dosl is None else dosl, dx, L_ * d, d if dxsl is None else dxsl, g, ws, ws_bytes, None)


@pytest.mark.parametrize("kw,name", [
    ({"L_": 0}, b"L ("), ({"L_": 257}, b"L ("),
    ({"d": 8, "heads": 1}, b"d_model"), ({"d": 24, "heads": 1}, b"d_model"), ({"d": 272, "heads": 1}, b"d_model"),
    ({"heads": 0}, b"heads"), ({"d": 64, "heads": 3}, b"heads"), ({"d": 64, "heads": 8}, b"heads"),
    ({"ffn": 8}, b"ffn_hidden"), ({"ffn": 24}, b"ffn_hidden"), ({"ffn": 1040}, b"ffn_hidden"),
    ({"blocks": 0}, b"n_blocks"), ({"blocks": 9}, b"n_blocks"),
    ({"L_": 256, "d": 256}, b"LDS"), ({"L_": 192, "d": 224}, b"LDS"),
    ({"dtype": L.DT_F16}, b"x_dtype"), ({"batch": -1}, b"batch"),
    ({"grads": None}, b"grads"), ({"packed_t": 8}, b"packed_t"), ({"packed_t": None}, b"packed_t"),
    ({"ws": 8}, b"ws"), ({"ws": None}, b"ws"), ({"ws_bytes": 64}, b"ws_bytes"),
    ({"dx": 1 << 30}, b"alias"), ({"dx": (1 << 30) + 4 * 100}, b"alias"),
    ({"xsl": 16}, b"x_stride_l"), ({"dosl": 16}, b"dout_stride_l"), ({"dxsl": 16}, b"dx_stride_l"),
    ({"eps": -1.0}, b"eps"),
])
def test_tfenc_bwd_limits(kw, name):
    lib = L.load()
    assert _bwd(lib, **kw) == L.RF_EINVAL
    assert name in lib.rf_last_error(), lib.rf_last_error()


def test_null_gradient_pointer_is_named():
    lib = L.load()
    g = (ctypes.c_void_p * 14)(*([16] * 5 + [None] + [16] * 8))
    assert _bwd(lib, grads=g) == L.RF_EINVAL and b"grads[5]" in lib.rf_last_error()


def test_sizes_and_batch_zero():
    lib = L.load()
    for Ln, d in ((256, 128), (128, 256)):
        assert _bwd(lib, L_=Ln, d=d, heads=1, ffn=128, batch=0) == L.RF_OK
        for batch in (0, 1, 3, 4096):
            n = lib.rf_tfenc_bwd_ws_bytes(batch, Ln, d, 1, 128, 2)
            assert n > 0 and n % 16 == 0, (batch, Ln, d, n)
    # the workload's shape, and every case of the GPU list
    for heads in (1, 2, 8):
        assert lib.rf_tfenc_bwd_ws_bytes(4096, 228, 128, heads, 512, 2) > 0
    for B, Ln, d, heads, ffn, nb in T.CASES:
        assert lib.rf_tfenc_bwd_ws_bytes(B, Ln, d, heads, ffn, nb) > 0
    # nothing of size [B][heads][L][L]: the workspace grows with L, not with L^2
    a, b = lib.rf_tfenc_bwd_ws_bytes(64, 128, 128, 8, 128, 1), lib.rf_tfenc_bwd_ws_bytes(64, 256, 128, 8, 128, 1)
    assert b <= 2 * a + 4096
    assert lib.rf_tfenc_bwd_ws_bytes(1, 256, 256, 1, 128, 1) == 0 and b"LDS" in lib.rf_last_error()
    assert lib.rf_tfenc_bwd_ws_bytes(1, 8, 32, 2, 32, 9) == 0 and b"n_blocks" in lib.rf_last_error()
    assert lib.rf_tfenc_bwd_ws_bytes(-1, 8, 32, 2, 32, 1) == 0 and b"batch" in lib.rf_last_error()
    assert lib.rf_tfenc_bwd_ws_bytes(1, 8, 32, 3, 32, 1) == 0 and b"heads" in lib.rf_last_error()
    d, ffn = 128, 256
    n = lib.rf_tfenc_bwd_packed_bytes(d, ffn, 2)
    assert n >= 2 * (3 * d * d + 2 * d * ffn) * 2 and n % 16 == 0
    assert lib.rf_tfenc_bwd_packed_bytes(24, ffn, 2) == 0 and b"d_model" in lib.rf_last_error()
    assert lib.rf_tfenc_bwd_packed_bytes(d, ffn, 9) == 0 and b"n_blocks" in lib.rf_last_error()
    ptrs = [16] * 5
    assert lib.rf_tfenc_bwd_pack(1, 32, 32, 1, *ptrs, 16, None) == L.RF_EINVAL and b"block" in lib.rf_last_error()
    assert lib.rf_tfenc_bwd_pack(0, 32, 32, 1, *ptrs, 8, None) == L.RF_EINVAL and b"aligned" in lib.rf_last_error()
    assert lib.rf_tfenc_bwd_pack(0, 32, 32, 1, *([16] * 4 + [None]), 16, None) == L.RF_EINVAL and b"null" in lib.rf_last_error()
