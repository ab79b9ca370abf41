"""The fused kernel's pooling pipeline (rf_fused.h phase 2) where a deeper pipeline can go wrong: every case bit-exact
against the C oracle.

The general path runs N stages of C tokens per team (N = 2; C = 2 for rows of one 16-byte chunk per lane, C = 1 for
wider rows; build options allow N up to 4), so per-team token counts must cover every remainder modulo N * C: slots
whose bags all hold L tokens for L = 0 .. 13 (past 2 * N * C + 1 for N = 2 and 3), slots whose lengths cycle with
runs of empty bags (several unit closes between two tokens), batches that end in a partial item, items that overflow the LDS row bucket (768 tokens), every combiner with
and without padding masks, Lmax equal to and larger than the longest bag, and the row widths that pick each kernel
instantiation.
"""
import numpy as np
import pytest
import torch

from recommendflow_amd.backend.encoder.sharded_encoder import GpuShardOps, ShardedFusedEncoder
from recommendflow_amd.backend.encoder.sparse_encoder import SLOT_DTYPE, FusedSparseEncoder, SlotSpec
from recommendflow_amd.backend.layers.preprocess_layers import DoubleHashingEmbedding
from recommendflow_amd.runtime.batch import from_lists

pytestmark = pytest.mark.gpu
COMBS = ["sum", "avg", "max", "min", "first", "last"]
F32, BF16 = torch.float32, torch.bfloat16
# (dim, table dtype, output dtype): CPL 1 / 2 / 4, not FULL, LPR 2, bf16 tables
WIDTHS = [(64, F32, F32), (128, F32, F32), (256, F32, F32), (48, F32, F32), (8, F32, F32), (64, BF16, BF16),
          (64, BF16, F32)]
CYCLE = [0, 0, 0, 1, 0, 0, 2, 3, 0, 0, 0, 0, 4, 5, 0, 6, 7, 0, 0, 8, 13, 0, 1, 1, 0, 12]


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else np.uint16)


def host(t):
    t = t.cpu()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.numpy()


def run_both(O, enc, hb):
    out = enc(hb.to("cuda"))
    flags = O.FLAG_MASK_PADDING if enc.mask_padding else 0
    odt = O.DT_F32 if enc.out_dtype == torch.float32 else O.DT_BF16
    ref, _ = O.fused_hash_embed(enc.host_desc, hb.tok_bytes, hb.tok_off, hb.bag_off, hb.lmax, hb.batch, host(enc.table),
                                enc.dim, enc.out_width, out_dtype=odt, flags=flags, emit_idx=False)
    return host(out), ref


def tokens(rng, n):
    return [b"" if rng.random() < 0.05 else b"t%d" % rng.integers(0, 500) for _ in range(n)]


def boundary_rows(B, half, seed):
    """10 slots: 7 whose bags all hold L tokens (L = 0 .. 6 or 7 .. 13), two whose lengths walk CYCLE (runs of empty
    bags; the second one unmasked), one single-valued (lean path)."""
    rng = np.random.default_rng(seed)
    rows = []
    for b in range(B):
        r = [tokens(rng, L) for L in range(7 * half, 7 * half + 7)]
        r.append(tokens(rng, CYCLE[b % len(CYCLE)]))
        r.append(tokens(rng, CYCLE[(b + 5) % len(CYCLE)]))
        r.append(tokens(rng, int(rng.random() < 0.7)))
        rows.append(r)
    # half 0: Lmax = the longest bag; half 1: Lmax larger than every bag
    lmax = None if half == 0 else [L + 2 for L in range(7, 14)] + [15, 16, 3]
    return from_lists(rows, lmax=lmax)


@pytest.fixture(scope="module")
def boundary_batches():
    return {(B, half): boundary_rows(B, half, 100 * half + B) for B in (1, 63, 65, 130) for half in (0, 1)}


@pytest.mark.parametrize("mask_padding", [False, True])
@pytest.mark.parametrize("B", [1, 63, 65, 130])
@pytest.mark.parametrize("dim,tdt,odt", WIDTHS)
def test_stage_boundaries(O, cuda, boundary_batches, dim, tdt, odt, B, mask_padding):
    for half in (0, 1):
        hb = boundary_batches[(B, half)]
        for comb in COMBS:
            specs = [SlotSpec(f"f{s}", 37 + 11 * s, (s, 50 + s), comb, mask_empty=s != 8) for s in range(10)]
            enc = FusedSparseEncoder(specs, dim, table_dtype=tdt, out_dtype=odt, seed=dim + half,
                                     mask_padding=mask_padding)
            got, ref = run_both(O, enc, hb)
            np.testing.assert_array_equal(bits(got), bits(ref), err_msg=f"{comb} half {half}")


@pytest.fixture(scope="module")
def overflow_batch():
    """B = 64 (one item per slot): 64 x 12 tokens = the bucket exactly, 64 x 13 just over it (the hot-to-cold hand-over
    falls inside a unit), and one bag longer than the bucket among short ones."""
    rng = np.random.default_rng(9)
    rows = []
    for b in range(64):
        rows.append([tokens(rng, 12), tokens(rng, 13), tokens(rng, 800 if b == 3 else b % 3),
                     tokens(rng, 20 if b % 2 else 5)])
    return from_lists(rows, lmax=[12, 14, 800, 21])


@pytest.mark.parametrize("mask_padding", [False, True])
@pytest.mark.parametrize("dim", [64, 128])
def test_bucket_overflow(O, cuda, overflow_batch, dim, mask_padding):
    for comb in COMBS:
        specs = [SlotSpec(f"f{s}", 90 + s, (3 + s, 77 - s), comb, mask_empty=s != 2) for s in range(4)]
        enc = FusedSparseEncoder(specs, dim, seed=dim, mask_padding=mask_padding)
        got, ref = run_both(O, enc, overflow_batch)
        np.testing.assert_array_equal(bits(got), bits(ref), err_msg=comb)


@pytest.mark.parametrize("mask_padding", [False, True])
@pytest.mark.parametrize("B", [1, 63, 65, 130])
@pytest.mark.parametrize("dim", [64, 128])
def test_null_combiner(O, cuda, dim, B, mask_padding):
    """null stores every position (per-feature operator, one slot): lengths walk CYCLE, Lmax = longest and longer,
    plus a batch whose single item overflows the bucket. With masked padding a bag is laid out by its own length
    ((k * len + l) * dim, both tables packed at the front) and the rest of the slot's 2 * Lmax positions is zero."""
    rng = np.random.default_rng(B)
    cases = [(from_lists([[tokens(rng, CYCLE[b % len(CYCLE)])] for b in range(B)], lmax=lm), True) for lm in ([1], [15])]
    if B == 65:
        cases.append((from_lists([[tokens(rng, 13 if b < 64 else 2)] for b in range(B)]), False))
    for hb, mask_empty in cases:
        emb = DoubleHashingEmbedding(211, dim, [5, 6], "null", mask_value="" if mask_empty else None, seed=dim,
                                     mask_padding=mask_padding)
        lm = int(hb.lmax[0])
        got = emb(hb.to("cuda")).reshape(B, -1)
        desc = emb._desc(0).cpu().numpy().view(SLOT_DTYPE)
        ref, _ = O.fused_hash_embed(desc, hb.tok_bytes, hb.tok_off, hb.bag_off, hb.lmax, B, host(emb.table), dim,
                                    2 * lm * dim, out_dtype=O.DT_F32,
                                    flags=O.FLAG_MASK_PADDING if mask_padding else 0, emit_idx=False)
        np.testing.assert_array_equal(bits(host(got)), bits(ref))


@pytest.mark.parametrize("mask_padding", [False, True])
@pytest.mark.parametrize("B", [63, 130])
@pytest.mark.parametrize("dim,tdt,odt", [(64, F32, F32), (128, F32, F32), (8, F32, F32), (64, BF16, BF16)])
def test_single_token_items_lean_vs_general(O, cuda, dim, tdt, odt, B, mask_padding):
    """Items of 0 / 1-token bags with Lmax = 1 take the lean phase 2; flag bit 15 forces the general pipeline on
    them. Both bit-exact with the oracle (a slot with one 2-token bag keeps the batch on the fused kernel)."""
    rng = np.random.default_rng(dim + B)
    rows = [[tokens(rng, 2 if (s == 4 and b == B // 2) else int(rng.random() < 0.75)) for s in range(5)]
            for b in range(B)]
    hb = from_lists(rows)
    assert list(hb.lmax) == [1, 1, 1, 1, 2]
    for comb in COMBS:
        specs = [SlotSpec(f"f{s}", 40 + 13 * s, (s, 7 + s), comb, mask_empty=s != 2) for s in range(5)]
        enc = FusedSparseEncoder(specs, dim, table_dtype=tdt, out_dtype=odt, seed=dim + 1, mask_padding=mask_padding)
        got, ref = run_both(O, enc, hb)
        np.testing.assert_array_equal(bits(got), bits(ref), err_msg=comb)
        enc.extra_flags = 1 << 15
        gen, _ = run_both(O, enc, hb)
        np.testing.assert_array_equal(bits(gen), bits(ref), err_msg=comb + " (general path)")


@pytest.mark.parametrize("mask_padding", [False, True])
def test_pool_rows_row_map_and_local_rows(O, cuda, boundary_batches, mask_padding):
    """The pre-gathered instantiation (rf_pool_rows_fwd) shares the pipeline: rows read through a row map, half of
    them in place from the local table (row map bit 31), equal the fused kernel's output, itself checked against
    the oracle."""
    dim, hb = 64, boundary_batches[(130, 1)]
    specs = [SlotSpec(f"f{s}", 37 + 11 * s, (s, 50 + s), COMBS[s % 6], mask_empty=s != 8) for s in range(10)]
    enc = FusedSparseEncoder(specs, dim, seed=4, mask_padding=mask_padding)
    want, ref = run_both(O, enc, hb)
    np.testing.assert_array_equal(bits(want), bits(ref))
    db, ops = hb.to("cuda"), GpuShardOps()
    sh = ShardedFusedEncoder(specs, dim, 0, 1, ops=ops, seed=4, mask_padding=mask_padding)
    req = torch.cat([ops.hash_rows(enc.desc, len(specs), db), sh.pad_rows])
    gathered = ops.gather(enc.table, req)
    g = torch.Generator().manual_seed(1)
    perm = torch.randperm(req.numel(), generator=g).cuda()
    shuffled = torch.empty_like(gathered)
    shuffled[perm] = gathered
    local = (torch.rand(req.numel(), generator=g) < 0.5).cuda()
    row_map = torch.where(local, req - (1 << 31), perm).to(torch.int32)  # bit 31 | row of the local table
    shuffled[perm[local]] = float("nan")  # a local row must not be read from the gathered buffer
    got = ops.pool(enc.desc, len(specs), db, shuffled, torch.empty((hb.batch, enc.out_width), device="cuda"),
                   1 if mask_padding else 0, row_map=row_map, local_table=enc.table)
    np.testing.assert_array_equal(bits(host(got)), bits(want))
