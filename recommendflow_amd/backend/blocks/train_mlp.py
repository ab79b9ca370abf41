"""create_mlp under model.fit for the DSSM towers (reference: backend/blocks/mlp.py:4-15 with
models/matching/dssm.py:25-26 `create_mlp([1024, 512, 256], 0.3, "selu", BatchNormalization(1e-6))`, trained by
example/ranking_search/train.py:96-104) on librf.so, replacing torch.nn.BatchNorm1d / Linear / SELU / Dropout.

Per layer, forward (training):
  mean, var = rf_col_stats(h)                          batch statistics (Keras tf.nn.moments: biased variance)
  W', b'    = rf_bn_fold(W, b, gamma, beta, mean, var) BatchNormalization folded into the Dense
  y         = selu(h W'^T + b')                        rf_gemm_f32, exact-fp32 MFMA, bias + SELU in its epilogue
  h_next    = rf_dropout_fwd(y)                        Keras Dropout(rate): kept / (1 - rate), counter-hash mask
and the moving statistics move as Keras does (moving = moving * momentum + batch * (1 - momentum), momentum
0.99, the biased batch variance). Backward: rf_selu_dropout_bwd (dpre and the bias gradient), the Dense weight
gradient G = dpre^T h (rf_gemm_f32) through rf_bn_fold_grad, dz = dpre W (rf_gemm_f32), rf_bn_bwd. In eval mode
the moving statistics fold into the weights (no dropout).
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Sequence

import torch

from ...runtime import gemm as GM
from ...runtime import lib as L

_SEED_MIX = 0x9E3779B97F4A7C15


def layer_seed(base: int, step: int, layer: int) -> int:
    """The dropout mask seed of (tower seed, training step, layer): a 64-bit mix, any value is valid."""
    x = (base * 0x100000001B3 + step * _SEED_MIX + layer * 0xC2B2AE3D27D4EB4F) & 0xFFFFFFFFFFFFFFFF
    return x


def _gemm_layer(probs, trans_a: bool, trans_b: bool, stream):
    """One layer's GEMMs of every tower (forward, weight gradient or input gradient): probs = [(a, b, bias, act name,
    out)]. librf (rf_gemm_f32: stream-K exact-fp32 MFMA, grouped into one launch where runtime.gemm.group_pays) when
    every operand qualifies; otherwise torch one by one, counted (runtime.gemm.torch_fallbacks)."""
    if all(GM.supported_gemm(a, b, trans_a, trans_b, o) for a, b, _, _, o in probs):
        return GM.gemm_f32_layer(probs, trans_a=trans_a, trans_b=trans_b, stream=stream)
    GM.note_torch_fallback("a tower backward layer (operand layout or size outside rf_gemm_f32's checks)")
    outs = []
    for a, b, bias, act, o in probs:
        A = a.t() if trans_a else a
        B = b.t() if trans_b else b
        r = torch.mm(A, B) if bias is None else torch.addmm(bias, A, B)
        r = {"selu": torch.selu, "relu": torch.relu, "none": lambda t: t}[act](r)
        if o is not None:
            o.copy_(r)
            r = o
        outs.append(r)
    return outs


def _towers_forward(towers, xs, params_list):
    """The training forward of several towers of equal depth on their inputs xs (2-D fp32 views with unit column
    stride; any row stride), layer by layer: per tower the batch statistics and the BatchNormalization fold, then ONE
    grouped GEMM (bias + SELU epilogue) for the layer of every tower, then per tower the dropout.
    Returns per tower (outputs per layer, batch means, batch variances, the step number that seeded the masks)."""
    for x in xs:
        if x.dim() != 2 or x.stride(1) != 1 or x.dtype != torch.float32:
            raise ValueError("TrainTower input must be a 2-D fp32 tensor with unit column stride")
    n = len(towers[0].units)
    if any(len(t.units) != n for t in towers):
        raise ValueError("towers of one grouped forward need equal depth")
    dev, st = xs[0].device, L.stream_ptr(None)
    steps = []
    for t in towers:
        steps.append(t.steps)
        t.steps += 1
    hs = list(xs)
    res = [([], [], []) for _ in towers]
    for l in range(n):
        probs, folded = [], []
        for ti, (tower, h, params) in enumerate(zip(towers, hs, params_list)):
            W, b, g, be = params[4 * l: 4 * l + 4]
            N, K = W.shape
            M = h.shape[0]
            mean = torch.empty(K, dtype=torch.float32, device=dev)
            var = torch.empty(K, dtype=torch.float32, device=dev)
            ws = L.workspace("rf_tower_ws_bytes", dev, M, K)
            L.call("rf_col_stats", L.ptr(h), M, K, h.stride(0), L.ptr(mean), L.ptr(var), L.ptr(ws), ws.numel(), st)
            Wf = torch.empty_like(W)
            bf = torch.empty(N, dtype=torch.float32, device=dev)
            L.call("rf_bn_fold", L.ptr(W), N, K, L.ptr(b), L.ptr(g), L.ptr(be), L.ptr(mean), L.ptr(var), tower.eps,
                   L.ptr(Wf), L.ptr(bf), st)
            y = torch.empty((M, N), dtype=torch.float32, device=dev)
            res[ti][1].append(mean)
            res[ti][2].append(var)
            folded.append(Wf)
            probs.append((h, Wf, bf, "selu", y))
        ys = _gemm_layer(probs, False, True, st)
        for ti, (tower, y) in enumerate(zip(towers, ys)):
            M, N = y.shape
            L.call("rf_dropout_fwd", L.ptr(y), M, N, N, tower.rate, layer_seed(tower.seed, steps[ti], l), L.ptr(y), N, st)
            with torch.no_grad():
                tower.moving_mean[l].mul_(tower.momentum).add_(res[ti][1][l], alpha=1.0 - tower.momentum)
                tower.moving_var[l].mul_(tower.momentum).add_(res[ti][2][l], alpha=1.0 - tower.momentum)
            res[ti][0].append(y)
        hs = ys
    return [(o, m, v, stp) for (o, m, v), stp in zip(res, steps)]


class _TowerBlock(NamedTuple):
    """One tower of a _TowersFn call, as the forward leaves it for the backward."""
    tower: "TrainTower"
    off: int  # its column block of x: x[:, off: off + width]
    width: int
    step: int  # the training step that seeded its dropout masks
    params: slice  # its W, b, gamma, beta per layer among the call's parameters
    saved: slice  # its outputs, batch means, batch variances per layer among the tensors saved after them


class _TowerViews(NamedTuple):
    """What _towers_backward reads and writes for one tower."""
    tower: "TrainTower"
    step: int
    x: torch.Tensor  # the input, as the forward saw it
    params: Sequence[torch.Tensor]  # W, b, gamma, beta per layer
    outs: Sequence[torch.Tensor]  # per layer, from the forward: the output after dropout,
    means: Sequence[torch.Tensor]  # the batch mean,
    vars: Sequence[torch.Tensor]  # the batch variance
    dout: torch.Tensor  # the gradient of the last output
    dx: torch.Tensor  # where the input gradient goes (x's shape; any row stride)


def _towers_backward(runs: Sequence[_TowerViews]):
    """Backward of _towers_forward: per tower the parameter gradients (W, b, gamma, beta per layer) returned, the
    input gradient written into its dx. Per layer, last to first: per tower the SELU / dropout backward (dpre, the
    bias gradient); ONE grouped GEMM for every tower's Dense weight gradient G = dpre^T h, per tower its fold
    (rf_bn_fold_grad); ONE grouped GEMM for dz = dpre W; per tower the BatchNormalization backward."""
    n = len(runs[0].tower.units)
    dev, st = runs[0].x.device, L.stream_ptr(None)
    dhs = [r.dout if r.dout.stride(1) == 1 else r.dout.contiguous() for r in runs]
    grads = [[None] * (4 * n) for _ in runs]
    for l in reversed(range(n)):
        dpres, dbs, wss, hins = [], [], [], []
        for r, dh in zip(runs, dhs):
            N, K = r.params[4 * l].shape
            h_in = r.x if l == 0 else r.outs[l - 1]
            M = h_in.shape[0]
            ws = L.workspace("rf_tower_ws_bytes", dev, M, max(K, N))
            dpre = torch.empty((M, N), dtype=torch.float32, device=dev)
            db = torch.empty(N, dtype=torch.float32, device=dev)
            L.call("rf_selu_dropout_bwd", L.ptr(dh), dh.stride(0), L.ptr(r.outs[l]), N, M, N, r.tower.rate,
                   layer_seed(r.tower.seed, r.step, l), L.ptr(dpre), N, L.ptr(db), L.ptr(ws), ws.numel(), st)
            dpres.append(dpre)
            dbs.append(db)
            wss.append(ws)
            hins.append(h_in)
        dWs = [torch.empty_like(r.params[4 * l]) for r in runs]
        Gs = _gemm_layer([(dp, h, None, "none", None) for dp, h in zip(dpres, hins)], True, False, st)
        for r, G, db, dW in zip(runs, Gs, dbs, dWs):
            W, b, g, be = r.params[4 * l: 4 * l + 4]
            N, K = W.shape
            L.call("rf_bn_fold_grad", L.ptr(G), N, K, L.ptr(db), L.ptr(g), L.ptr(be), L.ptr(r.means[l]),
                   L.ptr(r.vars[l]), r.tower.eps, L.ptr(dW), st)
        dzs = _gemm_layer([(dp, r.params[4 * l], None, "none", None) for r, dp in zip(runs, dpres)], False, False, st)
        for ti, r in enumerate(runs):
            g = r.params[4 * l + 2]
            K = r.params[4 * l].shape[1]
            h_in = hins[ti]
            M = h_in.shape[0]
            dx = r.dx if l == 0 else torch.empty((M, K), dtype=torch.float32, device=dev)
            dgamma = torch.empty(K, dtype=torch.float32, device=dev)
            dbeta = torch.empty(K, dtype=torch.float32, device=dev)
            dz = dzs[ti]
            L.call("rf_bn_bwd", L.ptr(dz), dz.stride(0), L.ptr(h_in), h_in.stride(0), M, K, L.ptr(r.means[l]),
                   L.ptr(r.vars[l]), L.ptr(g), r.tower.eps, L.ptr(dx), dx.stride(0), L.ptr(dgamma), L.ptr(dbeta),
                   L.ptr(wss[ti]), wss[ti].numel(), st)
            grads[ti][4 * l: 4 * l + 4] = [dWs[ti], dbs[ti], dgamma, dbeta]
            dhs[ti] = dx
    return grads


class _TowersFn(torch.autograd.Function):
    """Towers over column blocks of ONE input (the DSSM user and ad blocks of the fused encoder's output):
    the backward writes every tower's input gradient into its block of one full-width gradient, so autograd
    never materialises zero-filled slice gradients and adds them. Towers of equal depth run layer by layer
    together (one grouped GEMM per layer and pass)."""

    @staticmethod
    def forward(ctx, x, blocks, *params):
        towers = [t for t, _, _ in blocks]
        pslices, p0 = [], 0
        for t in towers:
            pslices.append(slice(p0, p0 + 4 * len(t.units)))
            p0 = pslices[-1].stop
        xs = [x[:, off: off + width] for _, off, width in blocks]
        groups = [[i] for i in range(len(towers))]
        if len({len(t.units) for t in towers}) == 1:
            groups = [list(range(len(towers)))]
        res = [None] * len(towers)
        for grp in groups:
            for i, r in zip(grp, _towers_forward([towers[i] for i in grp], [xs[i] for i in grp],
                                                 [params[pslices[i]] for i in grp])):
                res[i] = r
        saved, meta = [], []
        for (tower, off, width), ps, (outs, means, vars_, step) in zip(blocks, pslices, res):
            s0 = len(saved)
            saved += [*outs, *means, *vars_]
            meta.append(_TowerBlock(tower, off, width, step, ps, slice(s0, len(saved))))
        ctx.meta = meta
        ctx.groups = groups
        ctx.save_for_backward(x, *params, *saved)
        return tuple(r[0][-1] for r in res)

    @staticmethod
    def backward(ctx, *douts):
        x = ctx.saved_tensors[0]
        nparams = ctx.meta[-1].params.stop
        params = ctx.saved_tensors[1: 1 + nparams]
        saved = ctx.saved_tensors[1 + nparams:]
        dx = torch.zeros_like(x) if sum(m.width for m in ctx.meta) != x.shape[1] else torch.empty_like(x)
        grads: List[Optional[torch.Tensor]] = [None] * nparams
        runs = []
        for m, dout in zip(ctx.meta, douts):
            n = len(m.tower.units)
            mine = saved[m.saved]
            outs, means, vars_ = mine[:n], mine[n: 2 * n], mine[2 * n:]
            if dout is None:
                dout = torch.zeros_like(outs[-1])
            cols = slice(m.off, m.off + m.width)
            runs.append(_TowerViews(m.tower, m.step, x[:, cols], params[m.params], outs, means, vars_, dout, dx[:, cols]))
        for grp in ctx.groups:
            for i, g in zip(grp, _towers_backward([runs[i] for i in grp])):
                grads[ctx.meta[i].params] = g
        return (dx, None, *grads)


def towers_forward(x: torch.Tensor, blocks) -> tuple:
    """blocks: [(TrainTower, column offset, width)]: each tower's training forward on its block of x."""
    params = [p for t, _, _ in blocks for p in t.params()]
    return _TowersFn.apply(x, list(blocks), *params)


class TrainTower(torch.nn.Module):
    """One DSSM tower: [BatchNormalization(eps) -> Dense(units, selu) -> Dropout(rate)] per hidden size, fp32,
    glorot_uniform kernels and zero biases (Keras Dense defaults), gamma 1 / beta 0 / moving stats 0 and 1."""

    def __init__(self, in_features: int, units: Sequence[int], rate: float = 0.3, eps: float = 1e-6,
                 momentum: float = 0.99, seed: int = 0, generator: Optional[torch.Generator] = None, device="cuda"):
        super().__init__()
        L.load()
        L.require_gpu()
        self.units, self.rate, self.eps, self.momentum, self.seed = list(units), float(rate), float(eps), float(momentum), int(seed)
        self.steps = 0
        g = generator if generator is not None else torch.Generator().manual_seed(seed)
        self.W, self.b, self.gamma, self.beta = (torch.nn.ParameterList() for _ in range(4))
        self.moving_mean, self.moving_var = [], []
        width = int(in_features)
        for i, u in enumerate(self.units):
            lim = math.sqrt(6.0 / (width + u))
            self.W.append(torch.nn.Parameter(((torch.rand(u, width, generator=g) * 2 - 1) * lim).to(device)))
            self.b.append(torch.nn.Parameter(torch.zeros(u, device=device)))
            self.gamma.append(torch.nn.Parameter(torch.ones(width, device=device)))
            self.beta.append(torch.nn.Parameter(torch.zeros(width, device=device)))
            mm = torch.zeros(width, device=device)
            mv = torch.ones(width, device=device)
            self.register_buffer(f"moving_mean_{i}", mm)
            self.register_buffer(f"moving_var_{i}", mv)
            self.moving_mean.append(mm)
            self.moving_var.append(mv)
            width = u
        self.out_features = width

    def _apply(self, fn, *args, **kw):  # keep the moving-stat lists pointing at the registered buffers
        r = super()._apply(fn, *args, **kw)
        self.moving_mean = [getattr(self, f"moving_mean_{i}") for i in range(len(self.units))]
        self.moving_var = [getattr(self, f"moving_var_{i}") for i in range(len(self.units))]
        return r

    def params(self) -> List[torch.nn.Parameter]:
        out = []
        for l in range(len(self.units)):
            out += [self.W[l], self.b[l], self.gamma[l], self.beta[l]]
        return out

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.training:
            if x.stride(1) != 1:
                x = x.contiguous()
            return towers_forward(x, [(self, 0, x.shape[1])])[0]
        # inference: the moving statistics folded into the weights, no dropout
        st = L.stream_ptr(None)
        h = x if x.stride(1) == 1 else x.contiguous()
        for l in range(len(self.units)):
            W = self.W[l].detach()
            N, K = W.shape
            Wf = torch.empty_like(W)
            bf = torch.empty(N, dtype=torch.float32, device=x.device)
            L.call("rf_bn_fold", L.ptr(W), N, K, L.ptr(self.b[l]), L.ptr(self.gamma[l]), L.ptr(self.beta[l]),
                   L.ptr(self.moving_mean[l]), L.ptr(self.moving_var[l]), self.eps, L.ptr(Wf), L.ptr(bf), st)
            y = torch.empty((h.shape[0], N), dtype=torch.float32, device=x.device)
            h = GM.linear(h, Wf, bf, "selu", y, st)
        return h


class _LinearFn(torch.autograd.Function):
    """y = x W^T + b and its three backward products on rf_gemm_f32 (through _gemm_layer: the supported_gemm guard
    and the counted torch fallback for layouts the library refuses, e.g. a batch that is no multiple of 4 as the
    weight gradient's contraction length)."""

    @staticmethod
    def forward(ctx, x, W, b):
        st = L.stream_ptr(None)
        y = torch.empty((x.shape[0], W.shape[0]), dtype=torch.float32, device=x.device)
        _gemm_layer([(x, W, b, "none", y)], False, True, st)
        ctx.save_for_backward(x, W)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, W = ctx.saved_tensors
        st = L.stream_ptr(None)
        dy = dy.float()
        if dy.dim() != 2 or dy.stride(1) != 1:
            dy = dy.contiguous()
        dx = _gemm_layer([(dy, W, None, "none", None)], False, False, st)[0] if ctx.needs_input_grad[0] else None
        dW = _gemm_layer([(dy, x, None, "none", None)], True, False, st)[0] if ctx.needs_input_grad[1] else None
        db = dy.sum(dim=0) if ctx.needs_input_grad[2] else None
        return dx, dW, db


class TrainLinear(torch.nn.Module):
    """Keras Dense(units, activation="linear") under training: glorot_uniform kernel (stored [units][in]), zero bias,
    fp32, forward and backward on librf.so."""

    def __init__(self, in_features: int, units: int, seed: int = 0, generator: Optional[torch.Generator] = None,
                 device="cuda"):
        super().__init__()
        L.load()
        L.require_gpu()
        g = generator if generator is not None else torch.Generator().manual_seed(seed)
        lim = math.sqrt(6.0 / (in_features + units))
        self.W = torch.nn.Parameter(((torch.rand(units, in_features, generator=g) * 2 - 1) * lim).to(device))
        self.b = torch.nn.Parameter(torch.zeros(units, device=device))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = x.float()
        if x.stride(1) != 1:
            x = x.contiguous()
        return _LinearFn.apply(x, self.W, self.b)
