"""GPU: every entry point of csrc/rf_tower.hip through the C ABI at its dispatch edges, against float64 numpy on the
same fp32 inputs: the scalar (V == 1) and float4 instantiations of the column kernels (a width that is no multiple
of 4, a row stride that is none, a base pointer one float in), the row tail and the lane loop of the LayerNorm
row kernel, the second column block (widths above 1024), the four activations of act_vd at 0 and below it, distinct
row strides per operand, and row counts just above 4096 where the last row chunks are empty.

Bars are those of tests/test_esim_train_gpu.py, |got - want| <= rel max|want| + 1e-7 with rel = 1e-5 for forward
values and 1e-4 for gradients. Every operand lives in a NaN-filled buffer wider than the logical block: a pad column
read shows up as a NaN in the result, and after the launch everything outside the output block must still be NaN."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from recommendflow_amd.runtime import lib as L

pytestmark = pytest.mark.gpu

FWD, GRAD = 1e-5, 1e-4
GUARD = 8  # NaN floats kept behind every buffer


def close(got, want, rel=GRAD, what=""):
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), what
    err = np.abs(got - want).max() if got.size else 0.0
    print(f"{what}: err {err:.3e} max|want| {np.abs(want).max():.3e}")
    assert err <= rel * np.abs(want).max() + 1e-7, (what, err, np.abs(want).max())


class Blk:
    """An [M, K] block with row stride ld, `off` floats into a NaN-filled device buffer with GUARD NaNs behind it."""

    def __init__(self, M, K, ld, off=0, values=None):
        assert ld >= K
        self.M, self.K, self.ld, self.off = M, K, ld, off
        self.flat = torch.full((off + M * ld + GUARD,), float("nan"), device="cuda")
        self.view = self.flat[off: off + M * ld].view(M, ld)[:, :K]
        if values is not None:
            self.view.copy_(torch.as_tensor(np.ascontiguousarray(values, dtype=np.float32)))

    @property
    def ptr(self):
        return L.ptr(self.view)

    def get(self):
        return self.view.cpu().numpy()

    def assert_outside_untouched(self, what=""):
        chk = self.flat.clone()
        chk[self.off: self.off + self.M * self.ld].view(self.M, self.ld)[:, :self.K] = float("nan")
        assert torch.isnan(chk).all(), f"{what}: written outside the block"

    def assert_all_untouched(self, what=""):
        assert torch.isnan(self.flat).all(), f"{what}: written by a refused call"


def vec(K, values=None):
    return Blk(1, K, K, 0, None if values is None else np.asarray(values).reshape(1, K))


def ws_bytes(name, *a):
    return int(getattr(L.load(), name)(*a))


def ws_buf(n):
    return torch.empty(max(n, 4), dtype=torch.uint8, device="cuda")


def last_error():
    return L.load().rf_last_error().decode(errors="replace")


def bits(*arrs):
    return [np.ascontiguousarray(a).view(np.uint32) for a in arrs]


def same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(bits(*a), bits(*b)))


# ---- rf_layernorm_bwd ------------------------------------------------------------------------------------------
LN_EPS = 1e-6


def ln_bwd_ref(dy, x, gamma, eps=LN_EPS):
    dy, x, gamma = (np.asarray(t, np.float64) for t in (dy, x, gamma))
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    xh = (x - mu) * rstd
    u = dy * gamma
    dx = rstd * (u - u.mean(-1, keepdims=True) - xh * (u * xh).mean(-1, keepdims=True))
    return dx, (dy * xh).sum(0), dy.sum(0)


def ln_layouts(K):
    """(lddy, offdy), (ldx, offx), (lddx, offdx) of the three ways a case runs. padded: three distinct strides, each
    a multiple of 4 beyond K (K % 4 == 0: every row 16-byte aligned, the float4 kernel); misaligned: dy rows K + 1
    apart and x one float into its buffer, so the scalar kernel runs whatever K is."""
    return {"contiguous": ((K, 0), (K, 0), (K, 0)),
            "padded": ((K + 4, 0), (K + 8, 4), (K + 12, 0)),
            "misaligned": ((K + 1, 0), (K + 8, 1), (K + 3, 2))}


def run_ln_bwd(dy, x, gamma, layout):
    M, K = x.shape
    (lddy, ody), (ldx, ox), (lddx, odx) = layout
    bdy, bx = Blk(M, K, lddy, ody, dy), Blk(M, K, ldx, ox, x)
    bg = vec(K, gamma)
    n = ws_bytes("rf_layernorm_bwd_ws_bytes", M, K)
    outs = []
    for _ in range(2):  # the second launch: fresh outputs and workspace, the same bits
        bdx, bdg, bdb = Blk(M, K, lddx, odx), vec(K), vec(K)
        ws = ws_buf(n)
        L.call("rf_layernorm_bwd", bdy.ptr, lddy, bx.ptr, ldx, M, K, bg.ptr, LN_EPS, bdx.ptr, lddx, bdg.ptr, bdb.ptr,
               L.ptr(ws), n, L.stream_ptr())
        for b, what in ((bdx, "dx"), (bdg, "dgamma"), (bdb, "dbeta")):
            b.assert_outside_untouched(what)
        outs.append((bdx.get(), bdg.get()[0], bdb.get()[0]))
    assert same_bits(outs[0], outs[1]), "replay differs"
    return outs[0]


def ln_inputs(M, K, seed):
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=(M, K)) * 2 + 0.5).astype(np.float32)
    dy = rng.normal(size=(M, K)).astype(np.float32)
    gamma = (1 + 0.3 * rng.normal(size=K)).astype(np.float32)
    return dy, x, gamma


def check_ln_bwd(dy, x, gamma, rel=GRAD, tag=""):
    K = x.shape[1]
    want = ln_bwd_ref(dy, x, gamma)
    got = {}
    for name, layout in ln_layouts(K).items():
        got[name] = run_ln_bwd(dy, x, gamma, layout)
        for g, w, what in zip(got[name], want, ("dx", "dgamma", "dbeta")):
            close(g, w, rel, f"{tag}{name} {what}")
    if K % 4 == 0:  # float4 and scalar column kernels walk the same rows in the same order
        assert same_bits(got["padded"], got["misaligned"]), "float4 and scalar results differ"
        assert same_bits(got["contiguous"], got["misaligned"]), "float4 and scalar results differ"
    return got


@pytest.mark.parametrize("K", [1, 3, 48, 63, 64, 65, 130, 1028])
@pytest.mark.parametrize("M", [1, 3, 5, 301])
def test_layernorm_bwd_vs_float64(cuda, M, K):
    """M: the 4-rows-a-workgroup tail (1, 3, 5, 301 are no multiples of 4); K: idle lanes (1, 3, 48, 63), exactly a
    wave (64), a second and a third lane trip (65, 130), a second column block (1028); K = 1 has zero variance."""
    check_ln_bwd(*ln_inputs(M, K, 1000 * M + K))


def test_layernorm_bwd_empty_row_chunks(cuda):
    """M = 4100, K = 12: 512 chunks of 9 rows, the last 56 of them empty (zero partials)."""
    check_ln_bwd(*ln_inputs(4100, 12, 7))


def test_layernorm_bwd_zero_variance_row(cuda):
    """A row whose columns are all equal: xhat = 0, rstd = 1 / sqrt(eps), dx = rstd (u - mean(u)), finite. The value
    0.75 keeps the fp32 row sum and mean exact in any order, so the variance is 0 on both sides."""
    dy, x, gamma = ln_inputs(5, 65, 11)
    x[2] = 0.75
    x[4] = 0.0
    got = check_ln_bwd(dy, x, gamma)
    assert np.isfinite(got["contiguous"][0]).all()


# The fp32 floor of the large-mean case below (M = 301, K = 130, rows of mean 1000 and unit spread, seed 5): a plain
# float32 numpy two-pass restatement (ln_bwd_f32_two_pass: the mean, then the variance and the sums around it, every
# array float32) measured against float64 on those inputs gives, as err / max|want|,
#     dx 8.92e-06, dgamma 3.73e-05, dbeta 4.34e-07
# (on unit-scale rows the same restatement gives 1.3e-07, 5.3e-07, 4.3e-07). The fp32 mean of values near 1000 is
# off by up to a few ulp(1000) = 6e-5: a common shift of the row's xhat, which dgamma = sum(dy xhat) collects in full
# and dx through xhat mean(u xhat). Any fp32 kernel shares that floor, so each bar is 4x the measured figure.
LN_LARGE_MEAN_FLOOR = {"dx": 8.92e-06, "dgamma": 3.73e-05, "dbeta": 4.34e-07}
LN_LARGE_MEAN_BAR = {k: 4 * v for k, v in LN_LARGE_MEAN_FLOOR.items()}


def ln_large_mean_inputs():
    rng = np.random.default_rng(5)
    M, K = 301, 130
    x = (1000.0 + rng.normal(size=(M, K))).astype(np.float32)
    dy = rng.normal(size=(M, K)).astype(np.float32)
    gamma = (1 + 0.3 * rng.normal(size=K)).astype(np.float32)
    return dy, x, gamma


def ln_bwd_f32_two_pass(dy, x, gamma, eps=LN_EPS):
    """The measurement behind LN_LARGE_MEAN_FLOOR: ln_bwd_ref with every array and scalar in float32."""
    f = np.float32
    K = f(x.shape[1])
    mu = x.sum(-1, keepdims=True, dtype=f) / K
    d = x - mu
    var = (d * d).sum(-1, keepdims=True, dtype=f) / K
    rstd = f(1) / np.sqrt(var + f(eps))
    xh = d * rstd
    u = dy * gamma
    dx = rstd * (u - u.sum(-1, keepdims=True, dtype=f) / K - xh * ((u * xh).sum(-1, keepdims=True, dtype=f) / K))
    return dx, (dy * xh).sum(0, dtype=f), dy.sum(0, dtype=f)


def test_layernorm_bwd_large_mean(cuda):
    dy, x, gamma = ln_large_mean_inputs()
    want = ln_bwd_ref(dy, x, gamma)
    for g, w, what in zip(ln_bwd_f32_two_pass(dy, x, gamma), want, ("dx", "dgamma", "dbeta")):
        print(f"float32 numpy two-pass {what}: err / max|want| = {np.abs(g - w).max() / np.abs(w).max():.3e}")
    for name, layout in ln_layouts(x.shape[1]).items():
        got = run_ln_bwd(dy, x, gamma, layout)
        for g, w, what in zip(got, want, ("dx", "dgamma", "dbeta")):
            close(g, w, LN_LARGE_MEAN_BAR[what], f"large mean {name} {what}")


def test_layernorm_bwd_refuses_a_short_workspace(cuda):
    M, K = 5, 12
    dy, x, gamma = ln_inputs(M, K, 3)
    bdy, bx, bg = Blk(M, K, K, 0, dy), Blk(M, K, K, 0, x), vec(K, gamma)
    bdx, bdg, bdb = Blk(M, K, K), vec(K), vec(K)
    n = ws_bytes("rf_layernorm_bwd_ws_bytes", M, K)
    ws = ws_buf(n)
    rc = L.load().rf_layernorm_bwd(bdy.ptr, K, bx.ptr, K, M, K, bg.ptr, LN_EPS, bdx.ptr, K, bdg.ptr, bdb.ptr, L.ptr(ws), n - 1,
                                   L.stream_ptr())
    assert rc < 0 and "rf_layernorm_bwd" in last_error(), (rc, last_error())
    for b in (bdx, bdg, bdb):
        b.assert_all_untouched("rf_layernorm_bwd")


# ---- rf_act_dropout_fwd / rf_act_dropout_bwd ----------------------------------------------------------------------
ACTS = ["none", "gelu", "relu", "selu"]


def act_inputs(M, N, seed):
    """pre with exact zeros (relu's value and derivative at the kink: 0 and 0) and negative values (selu's exponential
    branch); the one-element case is the zero."""
    rng = np.random.default_rng(seed)
    pre = (rng.normal(size=(M, N)) * 1.5).astype(np.float32)
    pre.reshape(-1)[::7] = 0.0
    dh = rng.normal(size=(M, N)).astype(np.float32)
    if M * N > 1:
        assert (pre < 0).any() and (pre > 0).any()
    assert (pre == 0).any()
    return pre, dh


def act_layouts(N):
    """(ld, off) of pre, h / dpre and dh: three distinct row strides. aligned: multiples of 4 (the float4 kernels when
    N % 4 == 0); misaligned: N + 1, N + 2, N + 3 with one base pointer a float in (the scalar kernels always)."""
    n4 = (N + 3) // 4 * 4
    return {"aligned": ((n4 + 4, 0), (n4 + 8, 4), (n4 + 12, 0)), "misaligned": ((N + 1, 0), (N + 2, 1), (N + 3, 0))}


ACT_SHAPES = [(1, 1), (9, 4), (9, 33), (7, 1025), (7, 1028), (4100, 8)]
_keep_cache = {}


def keep_mask(seed, M, N, rate):
    key = (seed, M, N, rate)
    if key not in _keep_cache:
        _keep_cache[key] = O.dropout_keep(seed, M, N, rate) if rate > 0 else np.ones((M, N), bool)
        _keep_cache[key].setflags(write=False)
    return _keep_cache[key]


@pytest.mark.parametrize("M,N", ACT_SHAPES)
@pytest.mark.parametrize("rate", [0.0, 0.3])
@pytest.mark.parametrize("act", ACTS)
def test_act_dropout_fwd_bwd_vs_float64(cuda, act, rate, M, N):
    """h = where(keep, act(pre) / (1 - rate), 0) with the dropped elements exactly 0; dpre = where(keep, dh / (1 -
    rate), 0) act'(pre) and its column sums db; a replay gives the same bits, and so do the float4 and the scalar
    kernels. N = 1025, 1028: a second column block; M = 4100: empty row chunks in the bias-gradient partials."""
    seed = 0x1234567 + M * 31 + N
    pre, dh = act_inputs(M, N, M * 10000 + N)
    keep = keep_mask(seed, M, N, rate)
    p64 = pre.astype(np.float64)
    want_h = np.where(keep, O.activation(p64, act) / (1.0 - rate), 0.0)
    want_dpre = np.where(keep, dh.astype(np.float64) / (1.0 - rate), 0.0) * O.activation_grad(p64, act)
    want_db = want_dpre.sum(0)
    a = L.ACT[act]
    n = ws_bytes("rf_tower_ws_bytes", M, N)
    got = {}
    for name, ((ldp, op), (ldo, oo), (lddh, odh)) in act_layouts(N).items():
        bpre, bdh = Blk(M, N, ldp, op, pre), Blk(M, N, lddh, odh, dh)
        bh = Blk(M, N, ldo, oo)
        L.call("rf_act_dropout_fwd", bpre.ptr, ldp, M, N, a, rate, seed, bh.ptr, ldo, L.stream_ptr())
        bh.assert_outside_untouched("h")
        h = bh.get()
        close(h, want_h, FWD, f"{name} h")
        assert (h[~keep] == 0).all()
        outs = []
        for _ in range(2):
            bdp, bdb = Blk(M, N, ldo, oo), vec(N)
            ws = ws_buf(n)
            L.call("rf_act_dropout_bwd", bdh.ptr, lddh, bpre.ptr, ldp, M, N, a, rate, seed, bdp.ptr, ldo, bdb.ptr, L.ptr(ws), n,
                   L.stream_ptr())
            bdp.assert_outside_untouched("dpre")
            bdb.assert_outside_untouched("db")
            outs.append((bdp.get(), bdb.get()[0]))
        assert same_bits(outs[0], outs[1]), "replay differs"
        close(outs[0][0], want_dpre, GRAD, f"{name} dpre")
        close(outs[0][1], want_db, GRAD, f"{name} db")
        assert (outs[0][0][~keep] == 0).all()
        got[name] = (h,) + outs[0]
    assert same_bits(got["aligned"], got["misaligned"]), "float4 and scalar results differ"


@pytest.mark.parametrize("N", [4, 2])
@pytest.mark.parametrize("B", [37, 4100])
def test_act_dropout_bwd_as_column_sum(cuda, B, N):
    """The head's bias gradient in models/ranking/esim_train.py: act none, rate 0, seed 0 on the padded [B, 4]
    logit gradient with dh and pre the same buffer; dpre is a copy and db the column sums (N = 2: the two real
    logit columns of the same rows)."""
    rng = np.random.default_rng(B)
    dz = (rng.normal(size=(B, 4)) / B).astype(np.float32)
    bdz = Blk(B, 4, 4, 0, dz)
    bdp, bdb = Blk(B, N, 4), vec(N)
    n = ws_bytes("rf_tower_ws_bytes", B, N)
    ws = ws_buf(n)
    L.call("rf_act_dropout_bwd", bdz.ptr, 4, bdz.ptr, 4, B, N, L.ACT["none"], 0.0, 0, bdp.ptr, 4, bdb.ptr, L.ptr(ws), n,
           L.stream_ptr())
    bdp.assert_outside_untouched("dpre")
    bdb.assert_outside_untouched("db")
    assert np.array_equal(bdp.get(), dz[:, :N])
    assert np.array_equal(bdz.get(), dz)  # the shared input is only read
    close(bdb.get()[0], dz[:, :N].astype(np.float64).sum(0), GRAD, "db")


def test_act_dropout_argument_checks(cuda):
    """Refused on the host, nothing launched: a negative code, rf_last_error() names the entry point, and the
    outputs keep their NaN fill."""
    lib = L.load()
    st = L.stream_ptr()
    M, N = 9, 4
    pre, dh = act_inputs(M, N, 1)
    bpre, bdh = Blk(M, N, N, 0, pre), Blk(M, N, N, 0, dh)
    n = ws_bytes("rf_tower_ws_bytes", M, N)
    ws = ws_buf(n)

    def fwd(M_, act, rate, bp=bpre):
        bh = Blk(M_, N, N)
        rc = lib.rf_act_dropout_fwd(bp.ptr, N, M_, N, act, rate, 5, bh.ptr, N, st)
        assert rc < 0 and "rf_act_dropout_fwd" in last_error(), (rc, last_error())
        bh.assert_all_untouched("rf_act_dropout_fwd")

    def bwd(act, rate, nbytes):
        bdp, bdb = Blk(M, N, N), vec(N)
        rc = lib.rf_act_dropout_bwd(bdh.ptr, N, bpre.ptr, N, M, N, act, rate, 5, bdp.ptr, N, bdb.ptr, L.ptr(ws), nbytes, st)
        assert rc < 0 and "rf_act_dropout_bwd" in last_error(), (rc, last_error())
        bdp.assert_all_untouched("rf_act_dropout_bwd")
        bdb.assert_all_untouched("rf_act_dropout_bwd")

    fwd(M, L.ACT["softmax"], 0.3)
    bwd(L.ACT["softmax"], 0.3, n)
    fwd(M, L.ACT["gelu"], 1.0)
    bwd(L.ACT["gelu"], 1.0, n)
    fwd(65536, L.ACT["gelu"], 0.3, Blk(65536, N, N, 0, np.zeros((65536, N), np.float32)))  # one row past the grid's y limit
    bwd(L.ACT["gelu"], 0.3, n - 1)
    # and the same arguments, valid, are accepted
    bh = Blk(M, N, N)
    assert lib.rf_act_dropout_fwd(bpre.ptr, N, M, N, L.ACT["gelu"], 0.3, 5, bh.ptr, N, st) == 0
    assert np.isfinite(bh.get()).all()


# ---- empty row chunks in the DSSM tower's column reductions -----------------------------------------------------
# tower_chunks caps at 512 chunks of ceil(M / 512) rows: M = 4100 -> 9 rows a chunk, 456 chunks hold rows, 56 are
# empty; M = 5000 -> 10 rows, 12 empty chunks. K = 8, 12: float4; K = 7: scalar.
CHUNK_SHAPES = [(4100, 8), (5000, 12), (4100, 7)]
SELU_SCALE, SELU_ALPHA = 1.0507009873554804934193349852946, 1.6732632423543772848170429916717


def tower_ld(K):
    return K + 4 if K % 4 == 0 else K + 1


@pytest.mark.parametrize("center", [0.1, 1000.0])
@pytest.mark.parametrize("M,K", CHUNK_SHAPES)
def test_col_stats_empty_chunks(cuda, M, K, center):
    """Chan's combine must skip the n = 0 chunks: with a column mean of 1000 an empty chunk counted as rows of zeros
    (or a skipped full one) moves the variance by orders of magnitude more than the bar."""
    rng = np.random.default_rng(M + K)
    x = (center + rng.normal(size=(M, K))).astype(np.float32)
    ld = tower_ld(K)
    bx = Blk(M, K, ld, 0, x)
    n = ws_bytes("rf_tower_ws_bytes", M, K)
    outs = []
    for _ in range(2):
        bm, bv = vec(K), vec(K)
        ws = ws_buf(n)
        L.call("rf_col_stats", bx.ptr, M, K, ld, bm.ptr, bv.ptr, L.ptr(ws), n, L.stream_ptr())
        bm.assert_outside_untouched("mean")
        bv.assert_outside_untouched("var")
        outs.append((bm.get()[0], bv.get()[0]))
    assert same_bits(outs[0], outs[1]), "replay differs"
    x64 = x.astype(np.float64)
    close(outs[0][0], x64.mean(0), FWD, "mean")
    close(outs[0][1], x64.var(0), FWD, "var")


@pytest.mark.parametrize("M,K", CHUNK_SHAPES)
def test_selu_dropout_bwd_empty_chunks(cuda, M, K):
    rate, seed = 0.3, 4242
    rng = np.random.default_rng(M * 3 + K)
    keep = O.dropout_keep(seed, M, K, rate)
    pre = rng.normal(size=(M, K)) * 1.5
    h = np.where(keep, O.selu(pre) / (1.0 - rate), 0.0).astype(np.float32)
    dh = rng.normal(size=(M, K)).astype(np.float32)
    y = h.astype(np.float64) * (1.0 - rate)
    want = np.where(keep, dh.astype(np.float64) / (1.0 - rate) * np.where(y < 0, y + SELU_SCALE * SELU_ALPHA, SELU_SCALE), 0.0)
    ld = tower_ld(K)
    bdh, bh = Blk(M, K, ld, 0, dh), Blk(M, K, ld + 4, 0, h)
    n = ws_bytes("rf_tower_ws_bytes", M, K)
    outs = []
    for _ in range(2):
        bdp, bdb = Blk(M, K, ld + 8), vec(K)
        ws = ws_buf(n)
        L.call("rf_selu_dropout_bwd", bdh.ptr, ld, bh.ptr, ld + 4, M, K, rate, seed, bdp.ptr, ld + 8, bdb.ptr, L.ptr(ws), n,
               L.stream_ptr())
        bdp.assert_outside_untouched("dpre")
        bdb.assert_outside_untouched("db")
        outs.append((bdp.get(), bdb.get()[0]))
    assert same_bits(outs[0], outs[1]), "replay differs"
    close(outs[0][0], want, GRAD, "dpre")
    close(outs[0][1], want.sum(0), GRAD, "db")


@pytest.mark.parametrize("M,K", CHUNK_SHAPES)
def test_bn_bwd_empty_chunks(cuda, M, K):
    eps = 1e-6
    rng = np.random.default_rng(M * 5 + K)
    x = (0.2 + rng.normal(size=(M, K)) * 0.7).astype(np.float32)
    dz = rng.normal(size=(M, K)).astype(np.float32)
    gamma = (1 + 0.3 * rng.normal(size=K)).astype(np.float32)
    mean = x.astype(np.float64).mean(0).astype(np.float32)
    var = x.astype(np.float64).var(0).astype(np.float32)
    x64, dz64 = x.astype(np.float64), dz.astype(np.float64)
    rstd = 1.0 / np.sqrt(var.astype(np.float64) + eps)
    xh = (x64 - mean.astype(np.float64)) * rstd
    w_db, w_dg = dz64.sum(0), (dz64 * xh).sum(0)
    w_dx = gamma.astype(np.float64) * rstd * (dz64 - w_db / M - xh * w_dg / M)
    ld = tower_ld(K)
    bdz, bx = Blk(M, K, ld, 0, dz), Blk(M, K, ld + 4, 0, x)
    bmean, bvar, bg = vec(K, mean), vec(K, var), vec(K, gamma)
    n = ws_bytes("rf_tower_ws_bytes", M, K)
    outs = []
    for _ in range(2):
        bdx, bdg, bdb = Blk(M, K, ld + 8), vec(K), vec(K)
        ws = ws_buf(n)
        L.call("rf_bn_bwd", bdz.ptr, ld, bx.ptr, ld + 4, M, K, bmean.ptr, bvar.ptr, bg.ptr, eps, bdx.ptr, ld + 8, bdg.ptr,
               bdb.ptr, L.ptr(ws), n, L.stream_ptr())
        for b, what in ((bdx, "dx"), (bdg, "dgamma"), (bdb, "dbeta")):
            b.assert_outside_untouched(what)
        outs.append((bdx.get(), bdg.get()[0], bdb.get()[0]))
    assert same_bits(outs[0], outs[1]), "replay differs"
    close(outs[0][0], w_dx, GRAD, "dx")
    close(outs[0][1], w_dg, GRAD, "dgamma")
    close(outs[0][2], w_db, GRAD, "dbeta")


# ---- rf_bn_fold / rf_bn_fold_grad ---------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(3, 7), (5, 1028), (2, 1025), (4, 64)])
@pytest.mark.parametrize("bias", [True, False])
def test_bn_fold_and_grad_vs_float64(cuda, N, K, bias):
    """W' = W diag(a), b' = b + W c (b may be null) and dW = G diag(a) + db c^T with a = gamma / sqrt(var + eps),
    c = beta - mean a; K = 7, 1025: scalar lanes, 1028: float4 with a second trip of the 256-thread row loop."""
    eps = 1e-6
    rng = np.random.default_rng(N * 100 + K)
    W, G = rng.normal(size=(N, K)).astype(np.float32), rng.normal(size=(N, K)).astype(np.float32)
    b, db = rng.normal(size=N).astype(np.float32), rng.normal(size=N).astype(np.float32)
    gamma, beta = (1 + 0.3 * rng.normal(size=K)).astype(np.float32), rng.normal(size=K).astype(np.float32) * 0.2
    mean, var = rng.normal(size=K).astype(np.float32), (0.1 + rng.random(K)).astype(np.float32)
    d = np.float64
    a = gamma.astype(d) / np.sqrt(var.astype(d) + eps)
    c = beta.astype(d) - mean.astype(d) * a
    bW, bG, bb, bdb = Blk(N, K, K, 0, W), Blk(N, K, K, 0, G), vec(N, b), vec(N, db)
    bga, bbe, bme, bva = vec(K, gamma), vec(K, beta.astype(np.float32)), vec(K, mean), vec(K, var)
    bWo, bbo, bdW = Blk(N, K, K), vec(N), Blk(N, K, K)
    L.call("rf_bn_fold", bW.ptr, N, K, bb.ptr if bias else None, bga.ptr, bbe.ptr, bme.ptr, bva.ptr, eps, bWo.ptr, bbo.ptr,
           L.stream_ptr())
    L.call("rf_bn_fold_grad", bG.ptr, N, K, bdb.ptr, bga.ptr, bbe.ptr, bme.ptr, bva.ptr, eps, bdW.ptr, L.stream_ptr())
    for blk, what in ((bWo, "W'"), (bbo, "b'"), (bdW, "dW")):
        blk.assert_outside_untouched(what)
    close(bWo.get(), W.astype(d) * a, FWD, "W'")
    close(bbo.get()[0], (b.astype(d) if bias else 0.0) + W.astype(d) @ c, FWD, "b'")
    close(bdW.get(), G.astype(d) * a + db.astype(d)[:, None] * c, GRAD, "dW")
