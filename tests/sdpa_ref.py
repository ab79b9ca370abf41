"""Restatement of the generic masked attention for the rf_sdpa_fwd tests (torch CPU; never the code under test), written
from the reference's formulas: scaled_dot_product_attention (layer_utils.py:4-24: logits = q k^T / sqrt(depth), a zero of
the [..., Lq, 1] mask marks a QUERY row, whose logits are all replaced by -4294967295, so its softmax is uniform over the
keys) between the split_heads and merge transposes of MultiHeadAttention.call (attention_layers.py:159-167).

sdpa(q, k, v, mask, heads) in float64 is "want". sdpa(..., round_p=dtype) in float32 is the emulation of the kernel's
precision policy: the probabilities are rounded once (RNE) to fp16 / bf16 before P @ v and everything else is fp32. The
inputs are values of `dtype` already (generated in fp32, rounded once, and the same rounded values go to want, to the
emulation and to the GPU), so q, k and v as MFMA operands round nothing. rel_err is the rule of tests/fusion_ref.py; the
bar of a GPU case is 4 x the emulation's rel_err against float64 on the same inputs, floor 2^-20, and may not exceed
CAP[dtype]: 2^-8 for fp16, 2^-5 for bf16 (tests/test_sdpa_cpu.py asserts it for every case).
"""
import math

import torch

from fusion_ref import FLOOR, rel_err  # noqa: F401

CAP = {torch.float16: 2.0 ** -8, torch.bfloat16: 2.0 ** -5}
FILL = -4294967295.0

# (B, heads, Lq, Lk, depth): the smallest shapes at which each mechanism can break
CASES = [
    (1, 1, 1, 1, 32),      # one query, one key
    (2, 3, 5, 5, 32),      # keys padded inside a tile, three heads (row stride 96): a masked row averaging 16 rows
                           # instead of 5 fails by O(1)
    (2, 2, 17, 16, 64),    # Lq one past a tile; Lk exactly one tile: the other half of the 32-key P block is the zero tile
    (2, 2, 16, 17, 64),    # Lk one past a tile
    (1, 2, 33, 48, 32),    # three key tiles in a 64-key P block: the odd tile count
    (2, 1, 65, 31, 128),   # five query tiles: wave 0 loops twice and reuses its P buffer; depth 128; last key invalid
    (1, 2, 130, 129, 64),  # nine key tiles, Lkp 160, 67,584 bytes of LDS (just past the 64 KiB opt-in); wave 0 loops 3 x
    (1, 1, 3, 256, 64),    # the Lk limit: all 16 key tiles, 107,520 bytes
    (1, 1, 3, 224, 128),   # the largest Lk that fits at depth 128: 151,552 bytes
    (1, 2, 7, 255, 32),    # the very last key slot invalid
    (1, 1, 4096, 16, 32),  # the Lq limit: 256 query tiles
    (70, 2, 8, 8, 32),     # 140 workgroups: the example and head indexing
]
SCALED_CASE = (2, 2, 17, 16, 64)  # run with scale = 6: logits in the hundreds, softmaxes nearly one-hot
SCALE = 6.0

# both zeros mask a row; 0.5 and -3.0 do not (the reference compares with == 0)
MASK_VALUES = (0.0, -0.0, 1.0, 1.0, 0.5, -3.0, 1.0)


def lds_bytes(Lk, depth):
    """The kernel's dynamic LDS: k and v images of Lkp rows of depth + 8 and four 16 x (Lkp + 8) P tiles, 2 bytes each."""
    Lkp = (Lk + 31) // 32 * 32
    return 2 * Lkp * (depth + 8) * 2 + 4 * 16 * (Lkp + 8) * 2


def split_heads(t, heads):
    B, L, w = t.shape
    return t.reshape(B, L, heads, w // heads).permute(0, 2, 1, 3)  # [B, heads, L, depth]


def sdpa(q, k, v, mask, heads, round_p=None):
    """q [B, Lq, heads*depth], k, v [B, Lk, heads*depth] in the dtype to compute in; mask [B, Lq] (or [B, Lq, 1]) or
    None. round_p: the probabilities are rounded once to this dtype before P @ v. -> [B, Lq, heads*depth]."""
    B, Lq, w = q.shape
    depth = w // heads
    qh, kh, vh = split_heads(q, heads), split_heads(k, heads), split_heads(v, heads)
    logits = torch.matmul(qh, kh.transpose(-1, -2)) / math.sqrt(depth)
    if mask is not None:
        m = mask.reshape(B, 1, Lq, 1).to(q.dtype)
        logits = torch.where(m == 0, torch.full_like(logits, FILL), logits)
    logits = logits - logits.max(dim=-1, keepdim=True).values
    e = torch.exp(logits)
    p = e / e.sum(dim=-1, keepdim=True)
    if round_p is not None:
        p = p.to(round_p).to(q.dtype)
    return torch.matmul(p, vh).permute(0, 2, 1, 3).reshape(B, Lq, w)


def inputs(case, dtype, seed, scale=1.0):
    """q, k ~ N(0, 1) * scale and v ~ N(0, 1), rounded to `dtype`; a mask drawn from MASK_VALUES, for B > 1 example 0
    fully masked and the last example unmasked. -> (q, k, v in dtype, mask f32 [B, Lq])."""
    B, heads, Lq, Lk, depth = case
    g = torch.Generator().manual_seed(seed)
    w = heads * depth
    q = (torch.randn(B, Lq, w, generator=g) * scale).to(dtype)
    k = (torch.randn(B, Lk, w, generator=g) * scale).to(dtype)
    v = torch.randn(B, Lk, w, generator=g).to(dtype)
    mask = torch.tensor(MASK_VALUES)[torch.randint(0, len(MASK_VALUES), (B, Lq), generator=g)]
    if B > 1:
        mask[0] = 0.0
        mask[-1] = 1.0
    return q, k, v, mask


def bar_of(emu, want):
    """4 x the emulation's error (the kernel rounds where the emulation rounds; its accumulation order, expf and the
    reciprocal of the row sum differ), floor 2^-20."""
    return max(4.0 * rel_err(emu, want), FLOOR)


_REF = {}


def reference(case, dtype, masked=True, scale=1.0):
    """(q, k, v in dtype, mask or None, want float64, emulation, bar) of one GPU case, computed once."""
    key = (tuple(case), dtype, masked, scale)
    if key not in _REF:
        B, heads, Lq, Lk, depth = case
        q, k, v, mask = inputs(case, dtype, seed=Lq + Lk + depth, scale=scale)
        if not masked:
            mask = None
        want = sdpa(q.double(), k.double(), v.double(), mask, heads)
        emu = sdpa(q.float(), k.float(), v.float(), mask, heads, round_p=dtype)
        _REF[key] = (q, k, v, mask, want, emu, bar_of(emu, want))
    return _REF[key]
