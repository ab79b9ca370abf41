"""Float64 restatements for the FM / CrossNetwork training tests (torch CPU autograd; never the code under test), built
on tests/interact_ref.py (fm, cross: transcribed from the reference) and differentiated by autograd in the dtype given:
float64 is the reference, float32 calibrates the tolerance (fusion_ref.bar: 8 x the float32 CPU error, floor 2^-20).
deepfm() / dcn(): the rankers composed from a model's own parameters (training-mode BatchNormalization -> Dense(selu)
per hidden size, the interaction layer, the Dense(1) head, sigmoid cross-entropy plus the l2 penalties).
"""
import torch

import interact_ref as R
from fusion_ref import FLOOR, bar, model_params, rel_err, tower  # noqa: F401


def _leaf(t, dtype):
    return t.detach().cpu().to(dtype).requires_grad_(True)


def fm_grads(e, g, dtype=torch.float64):
    """e [B, fields, dim], g [B] -> (out [B, 1], de) of L = sum_b g[b] out[b] (second order only)."""
    e = _leaf(e, dtype)
    out = R.fm(e)
    (out[:, 0] * g.detach().cpu().to(dtype)).sum().backward()
    return out.detach(), e.grad


def new_fm_grads(e, w, ids, g, dtype=torch.float64):
    """New_FM: (out, de, dw) with the first order over w [rows, 1], ids [B, n]."""
    e, w = _leaf(e, dtype), _leaf(w, dtype)
    out = R.fm(e, w=w, ids=ids.cpu())
    (out[:, 0] * g.detach().cpu().to(dtype)).sum().backward()
    return out.detach(), e.grad, w.grad


def fm_layer_grads(V, w, w0, ids, g, dtype=torch.float64):
    """FM_Layer: e = V[ids] -> (out, dV, dw, dw0), dense gradients (untouched rows zero)."""
    V, w, w0 = _leaf(V, dtype), _leaf(w, dtype), _leaf(w0, dtype)
    ids = ids.cpu()
    out = R.fm(V[ids], w0=w0, w=w, ids=ids)
    (out[:, 0] * g.detach().cpu().to(dtype)).sum().backward()
    return out.detach(), V.grad, w.grad, w0.grad


def cross_grads(x, w, b, g, dtype=torch.float64):
    """x [B, dim], w, b [L, dim] (a layer's (dim, 1) weight as one row), g [B, dim] -> (out, dx, dw, db)."""
    x, w, b = _leaf(x, dtype), _leaf(w, dtype), _leaf(b, dtype)
    out = R.cross(x, [w[i].unsqueeze(1) for i in range(w.shape[0])], [b[i].unsqueeze(1) for i in range(b.shape[0])])
    (out * g.detach().cpu().to(dtype)).sum().backward()
    return out.detach(), x.grad, w.grad, b.grad


def central_differences(fn, t, h=1e-6):
    """d fn(t) / dt of a scalar float64 function by central differences, element by element."""
    t = t.detach().clone()
    out = torch.zeros_like(t)
    flat, oflat = t.view(-1), out.view(-1)
    for i in range(flat.numel()):
        v = flat[i].item()
        flat[i] = v + h
        up = float(fn(t))
        flat[i] = v - h
        dn = float(fn(t))
        flat[i] = v
        oflat[i] = (up - dn) / (2 * h)
    return out


def bce(logits, y):
    """Keras BinaryCrossentropy(from_logits=True): the batch mean of softplus(z) - y z."""
    return (torch.nn.functional.softplus(logits) - y * logits).mean()


def mlp(t, P, pre, x, training):
    """create_mlp: [BatchNormalization -> Dense(selu)] per hidden size (dropout 0), from the TrainTower t's parameters."""
    h = x
    for l in range(len(t.units)):
        mean = var = None
        if not training:
            mean = t.moving_mean[l].detach().cpu().to(x.dtype)
            var = t.moving_var[l].detach().cpu().to(x.dtype)
        h = tower(h, P[f"{pre}W.{l}"], P[f"{pre}b.{l}"], P[f"{pre}gamma.{l}"], P[f"{pre}beta.{l}"], t.eps, mean, var)
    return h


def deepfm(model, P, x, first_ids=None, training=True):
    """The [B] logits of a TrainableDeepFM from its parameters P and the embed output x [B, S*2D] (CPU, P's dtype)."""
    B = x.shape[0]
    e = x.reshape(B, model.n_slots, model.width)
    if first_ids is None:
        fm = R.fm(e)
    else:
        fm = R.fm(e, w=P["fm.w"], ids=first_ids.cpu())
    h = mlp(model.tower, P, "tower.", x, training)
    deep = h @ P["head.W"].t() + P["head.b"]
    return (fm + deep).reshape(B)


def deepfm_loss(model, P, x, y, first_ids=None):
    lv = bce(deepfm(model, P, x, first_ids), y)
    if first_ids is not None:
        lv = lv + model.fm.w_reg * torch.sum(torch.square(P["fm.w"]))
    return lv


def dcn(model, P, x, training=True):
    w, b = P["cross.w"], P["cross.b"]
    c = R.cross(x, [w[i].unsqueeze(1) for i in range(w.shape[0])], [b[i].unsqueeze(1) for i in range(b.shape[0])])
    h = mlp(model.tower, P, "tower.", x, training)
    cat = torch.cat([c, h], dim=1)
    return (cat @ P["head.W"].t() + P["head.b"]).reshape(x.shape[0])


def dcn_loss(model, P, x, y):
    lv = bce(dcn(model, P, x), y)
    return lv + model.cross.reg_w * torch.sum(torch.square(P["cross.w"])) + \
        model.cross.reg_b * torch.sum(torch.square(P["cross.b"]))
