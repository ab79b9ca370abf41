"""Float64 restatements for the Que2Search tests (torch CPU autograd; never the code under test).

fusion(): AttentionFusion (reference backend/layers/fusion_layers.py:40-46) with tf.nn.l2_normalize written as
u * rsqrt(clamp(ss, min=1e-12)). fusion_grads() differentiates it with autograd in the dtype given: float64 is the
reference, float32 calibrates the tolerance (bar()). que2search(): the two-tower model composed from a
TrainableQue2Search's own parameters (training-mode BatchNormalization -> Dense(selu) per channel, the fusions, the
linear embedding denses, the loss).
"""
import torch

FLOOR = 2.0 ** -20


def fusion(x, W, C, d, is_norm):
    """x [B, C*d], W [C*d, C] -> (out [B, d], att [B, C])."""
    att = torch.softmax(x @ W, dim=1)
    u = (x.reshape(x.shape[0], C, d) * att.unsqueeze(-1)).sum(dim=1)
    if is_norm:
        ss = (u * u).sum(dim=1, keepdim=True)
        u = u * torch.rsqrt(torch.clamp(ss, min=1e-12))
    return u, att


def fusion_grads(x, W, g, C, d, is_norm, dtype=torch.float64):
    """(out, att, dx, dW) of L = sum(out * g), evaluated in `dtype` on the CPU."""
    x = x.detach().cpu().to(dtype).requires_grad_(True)
    W = W.detach().cpu().to(dtype).requires_grad_(True)
    out, att = fusion(x, W, C, d, is_norm)
    (out * g.detach().cpu().to(dtype)).sum().backward()
    return out.detach(), att.detach(), x.grad, W.grad


def rel_err(got, want, scale=None):
    """max|got - want| / max|want| (0 when want is all zero and got equals it). `scale` replaces max|want| where the
    exact result is identically zero and max|want| is only float64 rounding noise (cancel_scale)."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    den = float(want.abs().max()) if want.numel() else 0.0
    if scale is not None:
        den = float(scale)
    num = float((got - want).abs().max()) if want.numel() else 0.0
    if den == 0.0:
        return 0.0 if num == 0.0 else float("inf")
    return num / den


def cancel_scale(x, W, g, C, d):
    """dim 1 under is_norm: out = u / |u| = +-1 whatever x and W are, so dx and dW are identically zero and what any
    precision returns is the rounding left over from g_u = r g - r^3 (u g) u, two terms of size |r g| that cancel.
    max|want| is then noise (1e-17 in float64) and no denominator; the size of the cancelling terms is:
    (max_b |r_b g_b| for dx, times max|x| for one example's share of dW)."""
    x, W, g = x.detach().cpu().double(), W.detach().cpu().double(), g.detach().cpu().double()
    u, _ = fusion(x, W, C, d, False)
    r = torch.rsqrt(torch.clamp((u * u).sum(dim=1, keepdim=True), min=1e-12))
    t = float((r * g).abs().max())
    return t, t * float(x.abs().max())


def bar(f32, f64, scale=None):
    """The tolerance of one output tensor: 8 x the error of the float32 CPU evaluation against float64 (the wave
    shuffle tree, the batch chunks and expf sum and round in another order than the CPU), floor 2^-20."""
    return max(8.0 * rel_err(f32, f64, scale), FLOOR)


def selu(x):
    return torch.nn.functional.selu(x)


def tower(x, W, b, gamma, beta, eps, mean=None, var=None):
    """BatchNormalization(eps) -> Dense(selu). Batch statistics (biased variance) unless moving mean / var are given."""
    if mean is None:
        mean = x.mean(dim=0)
        var = ((x - mean) ** 2).mean(dim=0)
    xn = (x - mean) * torch.rsqrt(var + eps) * gamma + beta
    return selu(xn @ W.t() + b)


def cosent(y, q, a, scale=20.0):
    s = (q * a).sum(dim=1) * scale
    diff = s[:, None] - s[None, :]
    mask = (y[:, None] < y[None, :])
    terms = torch.cat([torch.zeros(1, dtype=s.dtype), diff[mask]])
    return torch.logsumexp(terms, dim=0)


def inbatch_ce(y, q, a, scale=20.0):
    logits = scale * (q @ a.t())
    lse = torch.logsumexp(logits, dim=1)
    return ((lse - torch.diagonal(logits)) * y).mean()


def model_params(model, dtype=torch.float64):
    """Every trainable parameter of a TrainableQue2Search as leaf CPU tensors of `dtype`, keyed by its name."""
    return {n: p.detach().cpu().to(dtype).requires_grad_(True) for n, p in model.named_parameters()}


def que2search(model, P, x, training=True):
    """(q, a) of the model from its parameters P (model_params) and the embed output x [B, S*2D] (CPU, P's dtype)."""
    w2 = 2 * model.enc.dim
    outs = []
    for s, t in enumerate(model.towers):
        pre = f"towers.{s}."
        mean = var = None
        if not training:
            mean = t.moving_mean[0].detach().cpu().to(x.dtype)
            var = t.moving_var[0].detach().cpu().to(x.dtype)
        outs.append(tower(x[:, s * w2: (s + 1) * w2], P[pre + "W.0"], P[pre + "b.0"], P[pre + "gamma.0"],
                          P[pre + "beta.0"], t.eps, mean, var))
    nu = model.n_user_slots
    C_a = len(outs) - nu
    d = model.dim
    qf, _ = fusion(torch.cat(outs[:nu], dim=1), P["query_fusion.W"], nu, d, False)
    af, _ = fusion(torch.cat(outs[nu:], dim=1), P["app_fusion.W"], C_a, d, True)
    q = qf @ P["query_dense.W"].t() + P["query_dense.b"]
    a = af @ P["app_dense.W"].t() + P["app_dense.b"]
    return q, a
