"""Restatements for the CIN training tests (torch CPU; never the code under test), built on tests/interact_ref.py.

cin_grads          autograd through interact_ref.cin_einsum in the dtype given: float64 is the reference.
cin_bwd_emulated   the backward formulas of rf_cin_bwd (include/rf_api.h) in float64 with interact_ref.to_bf16 at exactly
                   the points of the kernel's precision policy: Z_k and W_k in the forward, Z_k, W_k and G^{k+1} in the
                   backward; X^k, dZ and both contractions of dZ are carried in float64.
CinEmu             a torch.autograd.Function: forward = cin_literal(bf16=True), backward = cin_bwd_emulated.
xdeepfm / xdeepfm_loss  TrainableXDeepFM composed from a model's own parameters, like interact_train_ref.dcn.
cin_bar            the tolerance of one tensor: max(4 x rel_err(emulated, float64), 2^-20); CAP = 2^-7 is the largest
                   error the emulation itself may have for the bar to mean anything.
"""
import torch

import interact_ref as R
from interact_train_ref import bce, mlp

CAP = 2.0 ** -7

# (B, F0, D, sizes): the forward's shapes (tests/test_interact_gpu.py CIN_SHAPES) and one with 4800 rows, which is five
# row chunks of the dW contraction (1024 rows each) with a partial last one
SHAPES = [(1, 1, 1, [1]), (3, 5, 10, [6, 4]), (2, 7, 16, [8]), (4, 33, 24, [16, 16, 8]), (5, 40, 130, [20]),
          (70, 3, 8, [4]), (64, 64, 32, [64, 64]), (2, 5, 10, [130, 3]), (2, 8, 4, [260, 260, 4]), (1, 512, 3, [8]),
          (1, 8, 3, [512, 512, 4]), (300, 4, 16, [8, 8])]


def cin_bar(emulated, want64):
    return max(4.0 * R.rel_err(emulated, want64), R.FLOOR)


def inputs(B, F0, D, sizes, bf16_x=False):
    """(x, Ws, g): interact_ref.cin_inputs(seed = F0 + D), x rounded to bf16 if asked, g ~ N(0, 1) [B, sum H]."""
    x, Ws = R.cin_inputs(B, F0, D, sizes, seed=F0 + D)
    if bf16_x:
        x = R.to_bf16(x)
    g = torch.randn(B, sum(sizes), generator=torch.Generator().manual_seed(7))
    return x, Ws, g


def cin_grads(x, Ws, g, dtype=torch.float64):
    """(out, dx, [dW_k]) of L = sum(out * g) by autograd through cin_einsum."""
    x = x.detach().cpu().to(dtype).requires_grad_(True)
    Ws = [W.detach().cpu().to(dtype).requires_grad_(True) for W in Ws]
    out = R.cin_einsum(x, Ws)
    (out * g.detach().cpu().to(dtype)).sum().backward()
    return out.detach(), x.grad, [W.grad for W in Ws]


def _emulated_forward(x, Ws):
    """X^0 .. X^{K-1} and out, the products and W rounded to bf16 (float64 otherwise)."""
    B, F0, D = x.shape
    Xs, outs = [x], []
    for W in Ws:
        Xk = Xs[-1]
        Z = R.to_bf16(x[:, :, None, :] * Xk[:, None, :, :]).reshape(B, F0 * Xk.shape[1], D)
        Xn = torch.einsum("mh,bmd->bhd", R.to_bf16(W[0]), Z)
        outs.append(Xn.sum(dim=-1))
        Xs.append(Xn)
    return Xs[:-1], torch.cat(outs, dim=1)


def cin_bwd_emulated(x, Ws, g):
    """(out, dx, [dW_k]) in float64 under the kernel's precision policy."""
    x = x.detach().cpu().double()
    Ws = [W.detach().cpu().double() for W in Ws]
    g = g.detach().cpu().double()
    B, F0, D = x.shape
    Xs, out = _emulated_forward(x, Ws)
    K = len(Ws)
    ooff = [0]
    for W in Ws:
        ooff.append(ooff[-1] + W.shape[2])
    dx = torch.zeros_like(x)
    dXn = None
    dWs = [None] * K
    for k in range(K - 1, -1, -1):
        Xk, W = Xs[k], Ws[k]
        Hk, Hn = Xk.shape[1], W.shape[2]
        G = g[:, ooff[k]: ooff[k + 1], None].expand(B, Hn, D)
        if dXn is not None:
            G = G + dXn
        Gb = R.to_bf16(G.contiguous())
        Zb = R.to_bf16(x[:, :, None, :] * Xk[:, None, :, :]).reshape(B, F0 * Hk, D)
        Wb = R.to_bf16(W[0])
        dWs[k] = torch.einsum("bmd,bhd->mh", Zb, Gb).reshape(1, F0 * Hk, Hn)
        dZ = torch.einsum("mh,bhd->bmd", Wb, Gb).reshape(B, F0, Hk, D)
        dXk = torch.einsum("bid,bijd->bjd", x, dZ)
        dx = dx + torch.einsum("bjd,bijd->bid", Xk, dZ)
        if k == 0:
            dx = dx + dXk
        dXn = dXk
    return out, dx, dWs


class CinEmu(torch.autograd.Function):
    """cin(x, *Ws) under the kernel's precision policy, forward and backward (results in x's dtype)."""

    @staticmethod
    def forward(ctx, x, *Ws):
        ctx.save_for_backward(x, *Ws)
        return R.cin_literal(x.double(), [W.double() for W in Ws], bf16=True).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        x, *Ws = ctx.saved_tensors
        _, dx, dWs = cin_bwd_emulated(x, Ws, g)
        return (dx.to(x.dtype), *[d.to(W.dtype) for d, W in zip(dWs, Ws)])


def cin_emu(x, Ws):
    return CinEmu.apply(x, *Ws)


def xdeepfm(model, P, x, training=True, cin=R.cin_einsum):
    """The [B] logits of a TrainableXDeepFM from its parameters P and the embed output x [B, S*2D] (CPU, P's dtype);
    cin(x3, Ws) is the interaction: cin_einsum (exact in P's dtype) or cin_emu (the kernel's precision policy)."""
    B = x.shape[0]
    Ws = [P[f"cin.cin_W.CIN_W_{i}"] for i in range(len(model.cin.cin_size))]
    c = cin(x.reshape(B, model.n_slots, model.width), Ws)
    h = mlp(model.tower, P, "tower.", x, training)
    cat = torch.cat([c, h], dim=1)
    return (cat @ P["head.W"].t() + P["head.b"]).reshape(B)


def xdeepfm_loss(model, P, x, y, cin=R.cin_einsum):
    lv = bce(xdeepfm(model, P, x, True, cin), y)
    for i in range(len(model.cin.cin_size)):
        lv = lv + model.cin.l2_reg * torch.sum(torch.square(P[f"cin.cin_W.CIN_W_{i}"]))
    return lv
