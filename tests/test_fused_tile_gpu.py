"""The fused kernel (rf_fused.h) over groups of kWaves = 4 adjacent slots x blocks of 64 examples: the work of one
workgroup, whether its waves walk their items independently (as they do now) or share phase 1 over a tile of 4 slots
(measured in round 8, not kept: DESIGN.md §4.1). Every case bit-exact against the C oracle (no tolerance).

Where the grouping can go wrong: a partial last slot group, a partial last example block, the slots of one group
differing in every descriptor field, a lean wave beside general ones, groups and blocks without any token, one slot of
a group overflowing its 768-token LDS bucket while its neighbours hold few (tokens past the bucket are hashed inline
by phase 2, or all in phase 1 when the ids are emitted), the register-staged hash of phase 1 (token lengths 0 .. 40
bytes at every start alignment), the work-order bijection of flag bit 11, a workgroup that walks several groups
(RF_FUSED_GRID_CAP, read once per process: a child process), and the pre-gathered instantiation (rf_pool_rows_fwd).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from recommendflow_amd.backend.encoder.sharded_encoder import GpuShardOps, ShardedFusedEncoder  # noqa: E402
from recommendflow_amd.backend.encoder.sparse_encoder import FusedSparseEncoder, SlotSpec  # noqa: E402
from recommendflow_amd.runtime.batch import from_lists  # noqa: E402

pytestmark = pytest.mark.gpu
COMBS = ["sum", "avg", "max", "min", "first", "last"]
F32, BF16 = torch.float32, torch.bfloat16
# (dim, table dtype, output dtype): one chunk per lane, LPR 2, four chunks per lane, bf16 tables / outputs
WIDTHS = [(64, F32, F32), (8, F32, F32), (256, F32, F32), (64, BF16, BF16), (64, BF16, F32)]
KCAP = 768  # rf_fused.h kCap


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else np.uint16)


def host(t):
    t = t.cpu()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.numpy()


def tokens(rng, n):
    return [b"" if rng.random() < 0.05 else b"t%d" % rng.integers(0, 500) for _ in range(n)]


def specs_for(S, rot=0):
    """Every slot of a group differs: bins, both salts, mask_empty and the combiner."""
    return [SlotSpec(f"f{s}", 29 + 17 * s, (3 * s + 1, 91 - s), COMBS[(s + rot) % 6], mask_empty=s % 3 != 2)
            for s in range(S)]


def is_multi(s):
    return s % 3 == 1  # groups 0 and 1 mix lean and general waves; slot 8 (group 2 of 9 slots) is lean alone


def mixed_rows(B, S, seed):
    rng = np.random.default_rng(seed)
    return [[tokens(rng, int(rng.integers(0, 6)) if is_multi(s) else int(rng.random() < 0.8)) for s in range(S)]
            for _ in range(B)]


def encoder(specs, dim=64, tdt=F32, odt=F32, mask_padding=False, seed=3):
    enc = FusedSparseEncoder(specs, dim, table_dtype=tdt, out_dtype=odt, seed=seed, mask_padding=mask_padding)
    enc.single_token = False  # all-single-valued batches stay on the fused kernel (its lean phase 2)
    return enc


def oracle(O, enc, hb, emit_idx=False):
    flags = O.FLAG_MASK_PADDING if enc.mask_padding else 0
    odt = O.DT_F32 if enc.out_dtype == torch.float32 else O.DT_BF16
    return O.fused_hash_embed(enc.host_desc, hb.tok_bytes, hb.tok_off, hb.bag_off, hb.lmax, hb.batch, host(enc.table),
                              enc.dim, enc.out_width, out_dtype=odt, flags=flags, emit_idx=emit_idx)


def check(O, enc, hb, msg=""):
    ref, _ = oracle(O, enc, hb)
    got = host(enc(hb.to("cuda")))
    np.testing.assert_array_equal(bits(got), bits(ref), err_msg=msg)
    return ref


@pytest.mark.parametrize("mask_padding", [False, True])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("S", [1, 3, 4, 5, 9])
def test_tile_edges(O, cuda, S, B, mask_padding):
    """One partial group, one exact group, a partial last group; partial and several example blocks. Slots of a group
    differ in every descriptor field and mix single- and multi-valued (a lean wave beside general ones)."""
    hb = from_lists(mixed_rows(B, S, 1000 * S + B))
    for rot in (0, 3):
        check(O, encoder(specs_for(S, rot), mask_padding=mask_padding), hb, f"rot {rot}")


@pytest.mark.parametrize("mask_padding", [False, True])
@pytest.mark.parametrize("dim,tdt,odt", WIDTHS)
def test_tile_widths(O, cuda, dim, tdt, odt, mask_padding):
    hb = from_lists(mixed_rows(65, 5, 77))
    for rot in (0, 2, 4):
        check(O, encoder(specs_for(5, rot), dim, tdt, odt, mask_padding, seed=dim), hb, f"rot {rot}")


@pytest.mark.parametrize("mask_padding", [False, True])
def test_tile_empty_cases(O, cuda, mask_padding):
    """Empty bags, a slot with Lmax = 0 inside a group, a slot group whose later example blocks (examples 64 ..) hold
    no token, and a batch without any token."""
    rng = np.random.default_rng(5)
    B, S = 130, 9
    rows = mixed_rows(B, S, 6)
    for b in range(B):
        rows[b][2] = []  # Lmax = 0, between a multi-valued and a single-valued slot
        if b >= 64:
            for s in range(4, 8):
                rows[b][s] = []  # group 1, blocks 1 and 2: no token at all
        if b % 7 == 0:
            rows[b][1] = []
        rows[b][5] = tokens(rng, 3) if b < 64 else []
    hb = from_lists(rows)
    assert hb.lmax[2] == 0
    for rot in range(6):
        check(O, encoder(specs_for(S, rot), mask_padding=mask_padding), hb, f"rot {rot}")
    nothing = from_lists([[[] for _ in range(5)] for _ in range(65)])
    assert nothing.tok_off.shape[0] == 1
    for rot in range(6):
        check(O, encoder(specs_for(5, rot), mask_padding=mask_padding), nothing, f"no token, rot {rot}")
    # the same empty batch with Lmax > 0: every position is padding
    padded = from_lists([[[] for _ in range(5)] for _ in range(65)], lmax=[1, 3, 0, 2, 1])
    for rot in range(6):
        check(O, encoder(specs_for(5, rot), mask_padding=mask_padding), padded, f"all padding, rot {rot}")


@pytest.fixture(scope="module")
def overflow_batch():
    """5 slots x 65 examples: slot 1 holds 64 x 13 = 832 tokens in the first example block (past the 768-token bucket:
    the hand-over falls inside a bag), slot 2 one 800-token bag among short ones; their neighbours hold 0 or 1."""
    rng = np.random.default_rng(9)
    rows = []
    for b in range(65):
        rows.append([tokens(rng, int(rng.random() < 0.8)), tokens(rng, 13), tokens(rng, 800 if b == 3 else b % 3),
                     tokens(rng, int(rng.random() < 0.5)), tokens(rng, 2)])
    hb = from_lists(rows)
    assert 64 * 13 > KCAP
    return hb


@pytest.mark.parametrize("mask_padding", [False, True])
@pytest.mark.parametrize("emit_idx", [False, True])
def test_tile_bucket_overflow(O, cuda, overflow_batch, emit_idx, mask_padding):
    hb = overflow_batch
    for rot in range(6):
        enc = encoder(specs_for(5, rot), mask_padding=mask_padding)
        ref, ref_idx = oracle(O, enc, hb, emit_idx=emit_idx)
        if emit_idx:  # the ids of every token, past the bucket included
            got, idx = enc(hb.to("cuda"), emit_idx=True)
            np.testing.assert_array_equal(idx.cpu().numpy(), ref_idx, err_msg=f"ids, rot {rot}")
        else:
            got = enc(hb.to("cuda"))
        np.testing.assert_array_equal(bits(host(got)), bits(ref), err_msg=f"rot {rot}")


@pytest.fixture(scope="module")
def token_shape_batch():
    """Token lengths 0 .. 40 bytes (past the 32-byte register window, every n & 7) at every start alignment 0 .. 3;
    the batch's last token ends at the last byte of tok_bytes. 4 slots per example taking 1, 2, 0 or 1, 1 tokens of
    the stream in turn."""
    rng = np.random.default_rng(21)
    stream = []
    for _ in range(4):  # sum(0 .. 40) is a multiple of 4: the 1-byte token moves the next cycle's alignments by one
        stream += [bytes(rng.integers(1, 256, L, dtype=np.uint8)) for L in range(41)] + [b"x"]
    stream.append(bytes(rng.integers(1, 256, 40, dtype=np.uint8)))
    rows, i, b = [], 0, 0
    while i < len(stream):
        take = [1, 2, b % 2, 1]
        row = []
        for n in take:
            row.append(stream[i:i + n])
            i += n
        rows.append(row)
        b += 1
    hb = from_lists(rows)
    n = np.diff(hb.tok_off)
    seen = {(int(a) & 3, int(l)) for a, l in zip(hb.tok_off[:-1], n)}
    assert all((sh, L) in seen for sh in range(4) for L in range(41))
    assert n[-1] == 40 and hb.tok_off[-1] == hb.tok_bytes.shape[0]
    return hb


@pytest.mark.parametrize("mask_padding", [False, True])
def test_tile_token_shapes(O, cuda, token_shape_batch, mask_padding):
    hb = token_shape_batch
    for rot in (0, 1):
        enc = encoder(specs_for(4, rot), mask_padding=mask_padding)
        ref, ref_idx = oracle(O, enc, hb, emit_idx=True)
        got, idx = enc(hb.to("cuda"), emit_idx=True)
        np.testing.assert_array_equal(idx.cpu().numpy(), ref_idx)
        np.testing.assert_array_equal(bits(host(got)), bits(ref))
        check(O, enc, hb)


@pytest.mark.parametrize("mask_padding", [False, True])
@pytest.mark.parametrize("B", [63, 130])
def test_tile_forced_general_path(O, cuda, B, mask_padding):
    """A single-valued group: the lean phase 2, and the general one forced by flag bit 15, bit for bit the same."""
    rng = np.random.default_rng(B)
    hb = from_lists([[tokens(rng, int(rng.random() < 0.75)) for _ in range(4)] for _ in range(B)])
    assert list(hb.lmax) == [1, 1, 1, 1]
    for rot in range(6):
        enc = encoder(specs_for(4, rot), mask_padding=mask_padding)
        ref = check(O, enc, hb, f"lean, rot {rot}")
        enc.extra_flags = 1 << 15
        np.testing.assert_array_equal(bits(host(enc(hb.to("cuda")))), bits(ref), err_msg=f"general, rot {rot}")


@pytest.mark.parametrize("S", [9, 33, 70])
def test_tile_xcd_order_flag(O, cuda, S):
    """Flag bit 11 permutes the work order over the first 8 * k slots (8 of 9, 32 of 33, 64 of 70; the rest keep the
    plain order) and changes no value."""
    hb = from_lists(mixed_rows(130, S, S))
    enc = encoder(specs_for(S))
    ref = check(O, enc, hb)
    enc.extra_flags = 1 << 11
    np.testing.assert_array_equal(bits(host(enc(hb.to("cuda")))), bits(ref))


@pytest.mark.parametrize("mask_padding", [False, True])
def test_tile_pool_rows(O, cuda, overflow_batch, mask_padding):
    """rf_pool_rows_fwd (the pre-gathered instantiation) shares phase 1 and the pooling: rows through a row map,
    half of them in place from the local table (bit 31), at 5 slots x 65 examples, equal the fused kernel's output."""
    dim, S, B = 64, 5, 65
    for hb in (from_lists(mixed_rows(B, S, 12)), overflow_batch):
        specs = specs_for(S, 1)
        enc = encoder(specs, dim, seed=4, mask_padding=mask_padding)
        want = check(O, enc, hb)
        db, ops = hb.to("cuda"), GpuShardOps()
        sh = ShardedFusedEncoder(specs, dim, 0, 1, ops=ops, seed=4, mask_padding=mask_padding)
        req = torch.cat([ops.hash_rows(enc.desc, S, db), sh.pad_rows])
        gathered = ops.gather(enc.table, req)
        g = torch.Generator().manual_seed(1)
        perm = torch.randperm(req.numel(), generator=g).cuda()
        shuffled = torch.empty_like(gathered)
        shuffled[perm] = gathered
        local = (torch.rand(req.numel(), generator=g) < 0.5).cuda()
        row_map = torch.where(local, req - (1 << 31), perm).to(torch.int32)  # bit 31 | row of the local table
        shuffled[perm[local]] = float("nan")  # a local row must not be read from the gathered buffer
        got = ops.pool(enc.desc, S, db, shuffled, torch.empty((B, enc.out_width), device="cuda"),
                       1 if mask_padding else 0, row_map=row_map, local_table=enc.table)
        np.testing.assert_array_equal(bits(host(got)), bits(want))


def grid_cap_child():
    """Runs in a child process started with RF_FUSED_GRID_CAP=2: 9 slots x 130 examples are 27 items for the 8 waves
    of two workgroups, so every wave walks 3 or 4 items (general, lean, empty and overflowing ones in turn)."""
    from oracle import oracle as O

    O.build()
    torch.cuda.set_device(0)
    rng = np.random.default_rng(31)
    rows = mixed_rows(130, 9, 32)
    for b in range(130):
        rows[b][6] = tokens(rng, 13)  # 832 tokens per full example block: past the bucket
        if b >= 64:
            rows[b][0] = rows[b][1] = rows[b][2] = rows[b][3] = []
    hb = from_lists(rows)
    for mask_padding in (False, True):
        for rot in range(6):
            enc = encoder(specs_for(9, rot), mask_padding=mask_padding)
            ref, ref_idx = oracle(O, enc, hb, emit_idx=True)
            got, idx = enc(hb.to("cuda"), emit_idx=True)
            np.testing.assert_array_equal(idx.cpu().numpy(), ref_idx)
            np.testing.assert_array_equal(bits(host(got)), bits(ref))
            check(O, enc, hb)
            enc.extra_flags = 1 << 11
            np.testing.assert_array_equal(bits(host(enc(hb.to("cuda")))), bits(ref))
    print("grid cap ok")


def test_tile_grid_cap_child_process(O, cuda):
    env = dict(os.environ, RF_FUSED_GRID_CAP="2")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "grid-cap-child"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "grid cap ok" in r.stdout


if __name__ == "__main__" and sys.argv[1:] == ["grid-cap-child"]:
    grid_cap_child()
