"""Float64 restatements of the feature-interaction layers (torch CPU; never the code under test), transcribed from the
reference backend/layers/network_layers.py: fm() :43-56 / :193-207, cross() :163-171, cin_literal() :238-255 step by
step (split on d, matmul with transpose_b, reshape, transpose, the 1x1 conv as a matmul), cin_einsum() the closed form
  X^{k+1}[h, d] = sum_{i, j} W_k[i H_k + j, h] X^0[i, d] X^k[j, d],  out = concat_k(sum_d X^{k+1}[:, d]).
cin_literal(..., bf16=True) is the kernel's precision policy: every outer-product tensor and every W rounded to bf16,
everything else in the dtype given. rel_err / bar are the rules of tests/fusion_ref.py.
"""
import torch

from fusion_ref import FLOOR, bar, rel_err  # noqa: F401


def to_bf16(t):
    """Round to bfloat16 (RNE) and return in t's dtype."""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def fm(e, w0=None, w=None, ids=None):
    """e [B, fields, dim] (embed_inputs, or embedding_lookup(V, inputs)); w [rows, 1], ids [B, n] -> [B, 1]."""
    square_sum = torch.square(torch.sum(e, dim=1, keepdim=True))
    sum_square = torch.sum(torch.square(e), dim=1, keepdim=True)
    out = 0.5 * torch.sum(square_sum - sum_square, dim=2)
    if w is not None:
        out = torch.sum(w[ids], dim=1) + out
    if w0 is not None:
        out = w0 + out
    return out


def fm_pairs(e):
    """The second-order term written out: sum_{f < g} <e_f, e_g> -> [B, 1]."""
    B, F, _ = e.shape
    out = torch.zeros(B, 1, dtype=e.dtype)
    for f in range(F):
        for g in range(f + 1, F):
            out[:, 0] += (e[:, f] * e[:, g]).sum(dim=1)
    return out


def cross(x, ws, bs):
    """x [B, dim]; ws, bs: lists of (dim, 1) weights -> [B, dim]."""
    x_0 = x.unsqueeze(2)
    x_l = x_0
    for w, b in zip(ws, bs):
        x_l1 = torch.tensordot(x_l, w, dims=([1], [0]))  # (B, 1, 1)
        x_l = torch.matmul(x_0, x_l1) + b + x_l
    return x_l.squeeze(2)


def cin_literal(x, Ws, bf16=False):
    """x [B, fields, dim]; Ws: Keras filters (1, fields * H_k, H_{k+1}) -> [B, sum H]."""
    dim = x.shape[-1]
    embedding_nums = x.shape[1]
    field_nums = [embedding_nums] + [W.shape[2] for W in Ws]
    hidden = [x]
    split_X_0 = torch.stack(torch.split(hidden[0], 1, dim=2))  # dim * (B, fields, 1)
    for idx, W in enumerate(Ws):
        split_X_K = torch.stack(torch.split(hidden[-1], 1, dim=2))  # dim * (B, H_k, 1)
        result_1 = torch.matmul(split_X_0, split_X_K.transpose(-1, -2))  # (dim, B, fields, H_k)
        result_2 = result_1.reshape(dim, -1, embedding_nums * field_nums[idx])
        result_3 = result_2.permute(1, 0, 2)  # (B, dim, fields * H_k)
        filt = W[0]
        if bf16:
            result_3, filt = to_bf16(result_3), to_bf16(filt)
        result_4 = torch.matmul(result_3, filt)  # conv1d, kernel 1, stride 1, VALID
        result_5 = result_4.permute(0, 2, 1)  # (B, H_{k+1}, dim)
        hidden.append(result_5)
    result = torch.cat(hidden[1:], dim=1)
    return torch.sum(result, dim=-1)


def cin_einsum(x, Ws):
    F0 = x.shape[1]
    xk, outs = x, []
    for W in Ws:
        Hk, Hn = xk.shape[1], W.shape[2]
        xk = torch.einsum("ijh,bid,bjd->bhd", W[0].reshape(F0, Hk, Hn), x, xk)
        outs.append(xk.sum(dim=-1))
    return torch.cat(outs, dim=1)


def cin_inputs(B, F0, D, sizes, seed=0):
    """x uniform in [-1, 1], W_k ~ N(0, 1 / (F0 H_k)) (float32 values)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, F0, D, generator=g) * 2 - 1
    Ws, Hk = [], F0
    for H in sizes:
        Ws.append(torch.randn(1, F0 * Hk, H, generator=g) / (F0 * Hk) ** 0.5)
        Hk = H
    return x, Ws
