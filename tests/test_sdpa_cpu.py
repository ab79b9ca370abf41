"""rf_sdpa_fwd without a GPU: the restatement (tests/sdpa_ref.py) agrees with a composition of torch's own softmax /
masked_fill / matmul and with the float64 oracle, a masked query row is the mean of v over exactly Lk keys, every limit is
refused with its argument named (validation precedes any HIP call, and does not depend on the batch), the limit shapes
are accepted, and the bar of every GPU case stays under its cap."""
import math

import numpy as np
import pytest
import torch

import sdpa_ref as R
from oracle import oracle as O
from recommendflow_amd.runtime import lib as L


def _torch_sdpa(q, k, v, mask, heads):
    B, Lq, w = q.shape
    Lk, depth = k.shape[1], w // heads
    sp = lambda t, n: t.view(B, n, heads, depth).transpose(1, 2)  # noqa: E731
    logits = sp(q, Lq) @ sp(k, Lk).transpose(-1, -2) / math.sqrt(depth)
    if mask is not None:
        logits = logits.masked_fill(mask.view(B, 1, Lq, 1) == 0, -4294967295.0)
    return (torch.softmax(logits, dim=-1) @ sp(v, Lk)).transpose(1, 2).reshape(B, Lq, w)


@pytest.mark.parametrize("masked", [False, True])
def test_restatement_matches_torch_composition_and_oracle(masked):
    case = (3, 3, 7, 11, 32)  # Lq != Lk
    B, heads, Lq, Lk, depth = case
    q, k, v, mask = (t.double() for t in R.inputs(case, torch.float32, seed=1))
    mask = mask if masked else None
    got = R.sdpa(q, k, v, mask, heads)
    assert got.shape == (B, Lq, heads * depth) and got.dtype == torch.float64
    err = R.rel_err(got, _torch_sdpa(q, k, v, mask, heads))
    sp = lambda t, n: t.view(B, n, heads, depth).permute(0, 2, 1, 3).numpy()  # noqa: E731
    m = None if mask is None else np.broadcast_to(mask.numpy().reshape(B, 1, Lq), (B, heads, Lq))
    want = O.sdpa(sp(q, Lq), sp(k, Lk), sp(v, Lk), m).transpose(0, 2, 1, 3).reshape(B, Lq, heads * depth)
    err_o = R.rel_err(got, torch.from_numpy(want))
    print(f"restatement vs torch composition {err:.3e}, vs oracle.sdpa {err_o:.3e}")
    assert err <= 1e-12 and err_o <= 1e-12


def test_masked_query_row_is_the_mean_of_v():
    """The mask marks query rows and broadcasts over the keys: a masked row's output is the plain mean of v over all Lk
    keys. -0.0 masks as 0.0 does; 0.5 and -3.0 are not zero and do not."""
    case = (3, 2, 6, 9, 32)
    B, heads, Lq, Lk, depth = case
    q, k, v, _ = (t.double() for t in R.inputs(case, torch.float32, seed=2))
    mask = torch.tensor([[0.0, -0.0, 1.0, 0.5, -3.0, 1.0]]).repeat(B, 1)
    assert math.copysign(1.0, float(mask[0, 1])) == -1.0
    out = R.sdpa(q, k, v, mask, heads)
    plain = R.sdpa(q, k, v, None, heads)
    for b in range(B):
        mean = v[b].mean(dim=0)
        for i in (0, 1):
            assert R.rel_err(out[b, i], mean) <= 1e-12
        for i in (2, 3, 4, 5):
            assert R.rel_err(out[b, i], mean) > 1e-3
            assert torch.equal(out[b, i], plain[b, i])
    # the generated masks hold every value, example 0 is fully masked and the last example is not masked at all
    m = R.inputs((3, 1, 130, 4, 32), torch.float16, seed=3)[3]
    assert float(m[0].abs().sum()) == 0 and bool((m[-1] == 1).all())
    assert set(m[1].tolist()) == {0.0, 1.0, 0.5, -3.0} and bool((torch.signbit(m[1]) & (m[1] == 0)).any())


def test_inputs_are_values_of_the_dtype():
    for dtype in (torch.float16, torch.bfloat16):
        q, k, v, mask, want, emu, _ = R.reference((2, 3, 5, 5, 32), dtype, True)
        assert q.dtype == k.dtype == v.dtype == dtype and mask.dtype == torch.float32
        assert want.dtype == torch.float64 and emu.dtype == torch.float32
        assert R.reference((2, 3, 5, 5, 32), dtype, True)[4] is want  # cached


def test_lds_of_the_cases():
    """The byte counts the case list relies on."""
    assert R.lds_bytes(129, 64) == 67584 and R.lds_bytes(256, 64) == 107520
    assert R.lds_bytes(224, 128) == 151552 <= 160 * 1024 < R.lds_bytes(225, 128) == R.lds_bytes(256, 128) == 173056
    assert R.lds_bytes(256, 32) < R.lds_bytes(256, 64)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("case", R.CASES + [R.SCALED_CASE + (R.SCALE,)])
def test_bar_of_every_gpu_case_is_under_the_cap(case, dtype):
    """The cap condition: bar = 4 x the emulation's error must stay <= 2^-8 (fp16) / 2^-5 (bf16), or it would hide a
    failure."""
    scale = case[5] if len(case) == 6 else 1.0
    for masked in (True, False):
        bar = R.reference(tuple(case[:5]), dtype, masked, scale)[6]
        print(f"{case} {dtype} masked={masked}: bar {bar:.3e} cap {R.CAP[dtype]:.3e}")
        assert R.FLOOR <= bar <= R.CAP[dtype]


def _fwd(lib, Lq=8, Lk=8, depth=32, heads=2, dtype=L.DT_F16, batch=1, q=16):
    return lib.rf_sdpa_fwd(q, 16, 16, dtype, batch, heads, Lq, Lk, depth, None, 16, None)


@pytest.mark.parametrize("kw,name", [
    ({"Lk": 0}, b"Lk"), ({"Lk": 257}, b"Lk"), ({"Lq": 0}, b"Lq"), ({"Lq": 4097}, b"Lq"),
    ({"depth": 48}, b"depth"), ({"depth": 256}, b"depth"), ({"dtype": L.DT_F32}, b"dtype"), ({"heads": 0}, b"heads"),
    ({"batch": -1}, b"batch"), ({"q": 8}, b"aligned"),
    ({"depth": 128, "Lk": 225}, b"LDS"), ({"depth": 128, "Lk": 256}, b"LDS"),
    ({"depth": 128, "Lk": 225, "batch": 0}, b"LDS"), ({"depth": 128, "Lk": 256, "batch": 0}, b"LDS"),
])
def test_sdpa_limits(kw, name):
    lib = L.load()
    assert _fwd(lib, **kw) == L.RF_EINVAL
    err = lib.rf_last_error()
    print(kw, err.decode())
    assert name in err and b"rf_sdpa_fwd" in err, err
    if name == b"LDS":
        assert b"Lk" in err and b"depth" in err, err


def test_limit_shapes_are_accepted():
    """batch 0 is a no-op that still validates: accepted without a GPU."""
    lib = L.load()
    for kw in ({"Lk": 256, "depth": 64}, {"Lk": 256, "depth": 32}, {"Lk": 224, "depth": 128}, {"Lq": 4096},
               {"Lq": 4096, "Lk": 224, "depth": 128}, {"Lq": 1, "Lk": 1}):
        assert _fwd(lib, batch=0, **kw) == L.RF_OK, (kw, lib.rf_last_error())
