"""Feature-interaction layers (reference: backend/layers/network_layers.py) on rf_interact.hip and rf_tfenc.hip:

  FM_Layer, New_FM    -> rf_fm_fwd     (:43-56, :193-207)
  CrossNetwork        -> rf_cross_fwd  (:163-171)
  CIN                 -> rf_cin_fwd    (:238-255)
  FFN                 -> two Dense     (:301-316)
  TransformerEncoder  -> rf_tfenc_fwd  (:319-352), transformer_encoder_stack: several blocks in one launch

Weights are created on the first call from the input shape, as Keras `build` does: 'random_normal' and
tf.random_normal_initializer() are N(0, 0.05^2), w0 starts at zero. FM_Layer, New_FM, CrossNetwork and CIN are the
inference layers: their parameters do not require gradients and their regularisation coefficients have no effect.

TrainFMLayer, TrainNewFM, TrainCrossNetwork and TrainCIN are the same layers under training: the parameters require
gradients, the forward joins torch autograd through rf_fm_fwd / rf_fm_bwd (the first-order and the gathered gradients
reduced per id by rf_segment_sum_rows), rf_cross_fwd / rf_cross_bwd and rf_cin_fwd / rf_cin_bwd, and regularization()
is Keras' l2(c) penalty c * sum(w^2) of the weights (w_reg, v_reg, reg_w, reg_b, l2_reg), which a model adds to its
loss.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, Optional, Sequence

import torch

from ...runtime import lib as L
from .attention_layers import MultiHeadAttention
from .core import Dense, LayerNormalization, Norm
from .layer_utils import index_mapping


def _normal(shape, gen, device):
    return (torch.randn(*shape, generator=gen) * 0.05).to(device)


def _concat_ids(inputs: Dict[str, torch.Tensor], device) -> torch.Tensor:
    """tf.concat([value for _, value in inputs.items()], axis=-1) of [B, n_i] id tensors -> int64 [B, n]."""
    cols = [torch.as_tensor(v).to(device=device, dtype=torch.int64) for v in inputs.values()]
    cols = [c.reshape(c.shape[0], -1) for c in cols]
    return torch.cat(cols, dim=-1).contiguous()


def _dense_view(x: torch.Tensor) -> torch.Tensor:
    """A [B, fields, dim] view the kernels read in place: f32 or bf16, dim contiguous, any batch / field stride."""
    if x.dtype not in (torch.float32, torch.bfloat16):
        x = x.float()
    if x.dim() != 3:
        raise ValueError(f"expected [batch, fields, dim], got {tuple(x.shape)}")
    if x.shape[2] > 1 and x.stride(2) != 1:
        x = x.contiguous()
    return x


def fm_forward(embed: Optional[torch.Tensor] = None, V: Optional[torch.Tensor] = None, ids: Optional[torch.Tensor] = None,
               w0: Optional[torch.Tensor] = None, w: Optional[torch.Tensor] = None,
               w_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
    """rf_fm_fwd: the dense form (embed [B, fields, dim]) or the gathered form (V [rows, k], ids [B, fields]) -> [B, 1]."""
    L.require_gpu()
    if (embed is None) == (V is None):
        raise ValueError("give exactly one of embed and V")
    n, ldw, w_rows = 0, 0, 0
    if w is not None:
        n, ldw, w_rows = w_ids.shape[1], w_ids.stride(0), w.numel()
    if embed is not None:
        x = _dense_view(embed)
        B, fields, dim = x.shape
        out = torch.empty((B, 1), dtype=torch.float32, device=x.device)
        L.call("rf_fm_fwd", L.ptr(x), L.torch_dtype_code(x.dtype), x.stride(0), x.stride(1), None, None, 0, 0, B, fields, dim,
               L.ptr(w0), L.ptr(w), L.ptr(w_ids), n, ldw, w_rows, L.ptr(out), L.stream_ptr())
    else:
        B, fields = ids.shape
        out = torch.empty((B, 1), dtype=torch.float32, device=V.device)
        L.call("rf_fm_fwd", None, L.DT_F32, 0, 0, L.ptr(V), L.ptr(ids), ids.stride(0), V.shape[0], B, fields, V.shape[1],
               L.ptr(w0), L.ptr(w), L.ptr(w_ids), n, ldw, w_rows, L.ptr(out), L.stream_ptr())
    return out


class FM_Layer(torch.nn.Module):
    """Factorization machine over a dict of id tensors (network_layers.py:8-56). The [B, fields, k] lookup of V is
    never written: the kernel gathers the rows."""

    def __init__(self, feature_columns, k, w_reg=0., v_reg=0., seed: int = 0, device="cuda"):
        super().__init__()
        L.load()
        L.require_gpu()
        self.feature_columns = feature_columns
        self.field_num = len(feature_columns)
        self.map_dict = {}
        self.feature_length = 0
        for feat in self.feature_columns:
            self.map_dict[feat['feat_name']] = self.feature_length
            self.feature_length += feat['feat_num']
        self.k, self.w_reg, self.v_reg = int(k), w_reg, v_reg
        self.seed, self.device = seed, device
        self.w0 = self.w = self.V = None

    def build(self, input_shape=None):
        g = torch.Generator().manual_seed(self.seed)
        self.w0 = torch.nn.Parameter(torch.zeros(1, device=self.device), requires_grad=False)
        self.w = torch.nn.Parameter(_normal((self.feature_length, 1), g, self.device), requires_grad=False)
        self.V = torch.nn.Parameter(_normal((self.feature_length, self.k), g, self.device), requires_grad=False)

    def forward(self, inputs: Dict[str, torch.Tensor]) -> torch.Tensor:
        if self.V is None:
            self.build()
        ids = _concat_ids(index_mapping(inputs, self.map_dict), self.V.device)
        return fm_forward(V=self.V.data, ids=ids, w0=self.w0.data, w=self.w.data, w_ids=ids)


class New_FM(torch.nn.Module):
    """The FM of DeepFM (network_layers.py:174-207): first order over the sparse ids (no w0), second order over the
    embeddings [B, fields, dim], read in place (f32 or bf16, any batch / field stride)."""

    def __init__(self, feature_length, w_reg=1e-6, seed: int = 0, device="cuda"):
        super().__init__()
        L.load()
        L.require_gpu()
        self.feature_length, self.w_reg = int(feature_length), w_reg
        self.seed, self.device = seed, device
        self.w = None

    def build(self, input_shape=None):
        g = torch.Generator().manual_seed(self.seed)
        self.w = torch.nn.Parameter(_normal((self.feature_length, 1), g, self.device), requires_grad=False)

    def forward(self, inputs, **kwargs) -> torch.Tensor:
        if self.w is None:
            self.build()
        sparse_inputs, embed_inputs = inputs['sparse_inputs'], inputs['embed_inputs']
        ids = _concat_ids(sparse_inputs, self.w.device)
        return fm_forward(embed=embed_inputs, w=self.w.data, w_ids=ids)


class CrossNetwork(torch.nn.Module):
    """The cross network of DCN (network_layers.py:130-171), every layer in one launch. cross_weights / cross_bias are
    the reference's per-layer (dim, 1) weights (views of one [layer_num, dim] buffer each). The reference's stray
    print of x_l1 (:168) is dropped."""

    def __init__(self, layer_num, reg_w=0., reg_b=0., seed: int = 0, device="cuda"):
        super().__init__()
        L.load()
        L.require_gpu()
        self.layer_num, self.reg_w, self.reg_b = int(layer_num), reg_w, reg_b
        self.seed, self.device = seed, device
        self.w = self.b = None

    def build(self, input_shape):
        dim = int(input_shape[-1])
        g = torch.Generator().manual_seed(self.seed)
        self.w = torch.nn.Parameter(_normal((self.layer_num, dim), g, self.device), requires_grad=False)
        self.b = torch.nn.Parameter(_normal((self.layer_num, dim), g, self.device), requires_grad=False)

    @property
    def cross_weights(self):
        return [self.w.data[i].unsqueeze(1) for i in range(self.layer_num)]

    @property
    def cross_bias(self):
        return [self.b.data[i].unsqueeze(1) for i in range(self.layer_num)]

    def forward(self, inputs: torch.Tensor) -> torch.Tensor:
        if self.w is None:
            self.build(inputs.shape)
        if self.layer_num == 0:
            return inputs
        x = inputs if inputs.dtype in (torch.float32, torch.bfloat16) else inputs.float()
        if x.dim() != 2:
            raise ValueError(f"expected [batch, dim], got {tuple(x.shape)}")
        if x.shape[1] > 1 and x.stride(1) != 1:
            x = x.contiguous()
        B, dim = x.shape
        out = torch.empty((B, dim), dtype=torch.float32, device=x.device)
        L.call("rf_cross_fwd", L.ptr(x), L.torch_dtype_code(x.dtype), x.stride(0), B, dim, self.layer_num, L.ptr(self.w.data),
               L.ptr(self.b.data), L.ptr(out), out.stride(0), L.stream_ptr())
        return out


class CIN(torch.nn.Module):
    """The compressed interaction network of xDeepFM (network_layers.py:210-255): [B, fields, dim] -> [B, sum(cin_size)]
    (the reference docstring's "(None, dim)" is wrong). cin_W['CIN_W_i'] are the fp32 master weights in the Keras
    filter shape (1, fields * H_i, H_{i+1}); the kernel reads a packed bf16 image of them, built on the device on the
    first call and again after load_state_dict or refresh() (assign to a master weight in place, then call refresh())."""

    def __init__(self, cin_size: Sequence[int], l2_reg=0., seed: int = 0, device="cuda"):
        super().__init__()
        L.load()
        L.require_gpu()
        self.cin_size, self.l2_reg = [int(s) for s in cin_size], l2_reg
        self.seed, self.device = seed, device
        self.cin_W = torch.nn.ParameterDict()
        self.embedding_nums = None
        self._packed = None
        self._sizes = (ctypes.c_int32 * len(self.cin_size))(*self.cin_size)

    def build(self, input_shape):
        self.embedding_nums = int(input_shape[1])
        self.field_nums = [self.embedding_nums] + self.cin_size
        g = torch.Generator().manual_seed(self.seed)
        for i in range(len(self.cin_size)):
            shape = (1, self.field_nums[0] * self.field_nums[i], self.field_nums[i + 1])
            self.cin_W['CIN_W_' + str(i)] = torch.nn.Parameter(_normal(shape, g, self.device), requires_grad=False)
        self._packed = None

    def refresh(self):
        """Rebuild the bf16 kernel image from the fp32 master weights."""
        K = len(self.cin_size)
        nbytes = int(L.load().rf_cin_packed_w_bytes(self.embedding_nums, self._sizes, K))
        if nbytes == 0:
            L.check(L.RF_EINVAL, "rf_cin_packed_w_bytes")
        packed = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        for i in range(K):
            W = self.cin_W['CIN_W_' + str(i)].data.float().contiguous()
            L.call("rf_cin_pack_w", L.ptr(W), i, self.embedding_nums, self._sizes, K, L.ptr(packed), L.stream_ptr())
        self._packed = packed

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        # not built yet: the first filter is (1, fields * fields, H_1), which gives the field count
        key = prefix + "cin_W.CIN_W_0"
        if self.embedding_nums is None and key in state_dict:
            self.build((None, math.isqrt(state_dict[key].shape[1]), None))
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        self._packed = None

    def forward(self, inputs: torch.Tensor) -> torch.Tensor:
        x = _dense_view(inputs)
        if self.embedding_nums is None:
            self.build(x.shape)
        B, fields, dim = x.shape
        if fields != self.embedding_nums:
            raise ValueError(f"CIN was built for {self.embedding_nums} fields, got {fields}")
        if self._packed is None:
            self.refresh()
        K = len(self.cin_size)
        lib = L.load()
        wsb = int(lib.rf_cin_ws_bytes(B, fields, dim, self._sizes, K))
        if wsb == 0:
            L.check(L.RF_EINVAL, "rf_cin_ws_bytes")
        ws = torch.empty(wsb, dtype=torch.uint8, device=x.device)
        out = torch.empty((B, sum(self.cin_size)), dtype=torch.float32, device=x.device)
        L.call("rf_cin_fwd", L.ptr(x), L.torch_dtype_code(x.dtype), x.stride(0), x.stride(1), B, fields, dim, self._sizes, K,
               L.ptr(self._packed), L.ptr(out), out.stride(0), L.ptr(ws), ws.numel(), L.stream_ptr())
        return out


class FFN(torch.nn.Module):
    """The position-wise feed-forward network (network_layers.py:301-316): Conv1D with kernel size 1 is a Dense over
    the last axis. conv1: d_model -> hidden_unit with relu, conv2: hidden_unit -> d_model, both with bias, fp32
    (glorot_uniform kernels, zero biases). On its own it is two Dense launches; inside TransformerEncoder the fused
    kernel reads its weights."""

    def __init__(self, hidden_unit, d_model, seed: int = 0, device="cuda"):
        super().__init__()
        self.hidden_unit, self.d_model = int(hidden_unit), int(d_model)
        self.conv1 = Dense(self.d_model, self.hidden_unit, activation="relu", dtype=torch.float32, seed=seed + 1, device=device)
        self.conv2 = Dense(self.hidden_unit, self.d_model, activation=None, dtype=torch.float32, seed=seed + 2, device=device)

    def forward(self, inputs: torch.Tensor) -> torch.Tensor:
        shape = inputs.shape
        x = inputs.reshape(-1, shape[-1])
        return self.conv2(self.conv1(x)).reshape(*shape[:-1], self.d_model)


class TransformerEncoder(torch.nn.Module):
    """One encoder block (network_layers.py:319-352): out1 = LN1(x + MHA(x, x, x, mask)), out = LN2(out1 + FFN(out1)),
    both dropouts the identity (inference), in one rf_tfenc_fwd launch. forward([x, mask]): x [B, L, d_model] f32 or
    bf16, read in place (any batch / row stride, e.g. the fused encoder's [B, S * 2D] output viewed as [B, S, 2D]);
    mask [B, L], [B, L, 1] or None, zero marking a QUERY row (its attention is the mean of v over all keys, as the
    reference's broadcast gives). Returns F32 [B, L, d_model], or fills `out` (a view with unit stride on d_model).

    mha (wq / wk / wv in fp32), ffn (conv1 / conv2), layernorm1 and layernorm2 hold the fp32 master parameters; the
    kernel reads a packed image of them, built on the device on the first call and again after load_state_dict or
    refresh() (assign to a parameter in place, then call refresh()). The state dict holds the parameters in the
    layers' own layouts (Dense keeps its kernel as [out][in])."""

    _STATE = (("wq_kernel", "mha.wq.weight"), ("wq_bias", "mha.wq.bias"), ("wk_kernel", "mha.wk.weight"),
              ("wk_bias", "mha.wk.bias"), ("wv_kernel", "mha.wv.weight"), ("wv_bias", "mha.wv.bias"),
              ("conv1_kernel", "ffn.conv1.weight"), ("conv1_bias", "ffn.conv1.bias"),
              ("conv2_kernel", "ffn.conv2.weight"), ("conv2_bias", "ffn.conv2.bias"),
              ("ln1_gamma", "layernorm1.gamma"), ("ln1_beta", "layernorm1.beta"),
              ("ln2_gamma", "layernorm2.gamma"), ("ln2_beta", "layernorm2.beta"))

    def __init__(self, d_model, num_heads=1, ffn_hidden_unit=128, dropout=0., layer_norm_eps=1e-6, seed: int = 0,
                 device="cuda"):
        super().__init__()
        L.load()
        L.require_gpu()
        self.d_model, self.num_heads, self.ffn_hidden_unit = int(d_model), int(num_heads), int(ffn_hidden_unit)
        self.dropout, self.layer_norm_eps = dropout, float(layer_norm_eps)
        self.seed, self.device = seed, device
        self.mha = MultiHeadAttention(self.d_model, self.num_heads, seed=seed, device=device, proj_dtype=torch.float32)
        self.ffn = FFN(self.ffn_hidden_unit, self.d_model, seed=seed + 3, device=device)
        self.layernorm1 = Norm(LayerNormalization(epsilon=self.layer_norm_eps), self.d_model, device=device)
        self.layernorm2 = Norm(LayerNormalization(epsilon=self.layer_norm_eps), self.d_model, device=device)
        # the sub-layers keep plain tensors; the same tensors are this module's buffers, so that state_dict /
        # load_state_dict (an in-place copy) see them
        for name, path in self._STATE:
            obj = self
            for part in path.split("."):
                obj = getattr(obj, part)
            self.register_buffer(name, obj)
        self._gen = 0          # bumped whenever the masters may have changed
        self._stack = None     # (key, image) of the last stack this block led

    def shape_key(self):
        return (self.d_model, self.num_heads, self.ffn_hidden_unit, self.layer_norm_eps)

    def refresh(self):
        """Drop the packed image: the next call packs it again from the fp32 masters."""
        self._gen += 1
        self._stack = None

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        self.refresh()

    def _pack_into(self, packed: torch.Tensor, block: int, n_blocks: int):
        f = lambda name: L.ptr(getattr(self, name))  # noqa: E731
        # Dense keeps [out][in]; the ABI takes the Keras (in, out) kernels
        kern = {n: getattr(self, n).t().contiguous() for n in ("wq_kernel", "wk_kernel", "wv_kernel", "conv1_kernel", "conv2_kernel")}
        L.call("rf_tfenc_pack", block, self.d_model, self.ffn_hidden_unit, n_blocks, L.ptr(kern["wq_kernel"]), f("wq_bias"),
               L.ptr(kern["wk_kernel"]), f("wk_bias"), L.ptr(kern["wv_kernel"]), f("wv_bias"), f("ln1_gamma"), f("ln1_beta"),
               L.ptr(kern["conv1_kernel"]), f("conv1_bias"), L.ptr(kern["conv2_kernel"]), f("conv2_bias"), f("ln2_gamma"),
               f("ln2_beta"), L.ptr(packed), L.stream_ptr())

    def forward(self, inputs, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        x, mask = inputs
        return transformer_encoder_stack([self], x, mask, out=out)


def transformer_encoder_stack(blocks: Sequence[TransformerEncoder], x: torch.Tensor, mask: Optional[torch.Tensor] = None,
                              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """blocks[-1](... blocks[0]([x, mask]) ..., mask) in ONE rf_tfenc_fwd launch through one packed image of all blocks
    (cached on blocks[0] until one of them is refreshed or reloaded). The blocks must have equal shapes (d_model,
    num_heads, ffn_hidden_unit, layer_norm_eps): ValueError otherwise."""
    L.require_gpu()
    blocks = list(blocks)
    if not blocks:
        raise ValueError("transformer_encoder_stack needs at least one block")
    lead = blocks[0]
    for blk in blocks[1:]:
        if blk.shape_key() != lead.shape_key():
            raise ValueError(f"blocks of one stack must have equal shapes: {blk.shape_key()} != {lead.shape_key()}")
    x = _dense_view(x)
    B, Ln, d = x.shape
    if d != lead.d_model:
        raise ValueError(f"TransformerEncoder was built for d_model {lead.d_model}, got {d}")
    n = len(blocks)
    lib = L.load()
    key = tuple((id(blk), blk._gen) for blk in blocks)
    if lead._stack is None or lead._stack[0] != key:
        nbytes = int(lib.rf_tfenc_packed_bytes(lead.d_model, lead.ffn_hidden_unit, n))
        if nbytes == 0:
            L.check(L.RF_EINVAL, "rf_tfenc_packed_bytes")
        packed = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        for i, blk in enumerate(blocks):
            blk._pack_into(packed, i, n)
        lead._stack = (key, packed)
    packed = lead._stack[1]
    m = None
    if mask is not None:
        m = mask.reshape(B, Ln).to(device=x.device, dtype=torch.float32).contiguous()
    if out is None:
        out = torch.empty((B, Ln, d), dtype=torch.float32, device=x.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B, Ln, d) or (d > 1 and out.stride(2) != 1):
        raise ValueError(f"out must be an F32 [{B}, {Ln}, {d}] view with unit stride on the last axis")
    L.call("rf_tfenc_fwd", L.ptr(x), L.torch_dtype_code(x.dtype), x.stride(0), x.stride(1), L.ptr(m), B, Ln, d, lead.num_heads,
           lead.ffn_hidden_unit, n, L.ptr(packed), lead.layer_norm_eps, L.ptr(out), out.stride(0), out.stride(1),
           L.stream_ptr())
    return out


# ---- training ----------------------------------------------------------------------------------------------------------
def _segment_sum(ids: torch.Tensor, vals: torch.Tensor, id_range: int):
    """rf_segment_sum_rows: ids int64 [n], vals f32 [n, D] (D a multiple of 4, at most 256) -> (distinct ids ascending,
    their rows summed in input order); ids outside [0, id_range) are dropped. Reads the device count (one sync)."""
    n, D = vals.shape
    cap = max(1, min(n, id_range))
    dev = vals.device
    uid = torch.empty(cap, dtype=torch.int64, device=dev)
    uval = torch.empty((cap, D), dtype=torch.float32, device=dev)
    n_uniq = torch.zeros(1, dtype=torch.int32, device=dev)
    wsb = int(L.load().rf_segment_sum_ws_bytes(n, id_range))
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=dev)
    L.call("rf_segment_sum_rows", L.ptr(ids), L.ptr(vals), n, D, id_range, L.ptr(uid), L.ptr(uval), cap, L.ptr(n_uniq),
           L.ptr(ws), ws.numel(), L.stream_ptr())
    k = int(n_uniq.item())
    return uid[:k], uval[:k]


def _dense_row_grad(ids: torch.Tensor, vals: torch.Tensor, rows: int, width: int) -> torch.Tensor:
    """The dense [rows, width] gradient of a table from its per-position gradient rows vals [n, >= width] (columns past
    `width` are padding to rf_segment_sum_rows' multiple of 4): per-id sums in position order, untouched rows zero."""
    out = torch.zeros((rows, width), dtype=torch.float32, device=vals.device)
    ids = ids.reshape(-1).contiguous()
    for c0 in range(0, vals.shape[1], 256):
        blk = vals[:, c0: c0 + 256]
        if vals.shape[1] > 256:
            blk = blk.contiguous()
        uid, uval = _segment_sum(ids, blk, rows)
        w = min(width - c0, blk.shape[1])
        if w > 0:
            out[uid, c0: c0 + w] = uval[:, :w]
    return out


def _first_order_grad(dout: torch.Tensor, w_ids: torch.Tensor, rows: int) -> torch.Tensor:
    """dw [rows, 1]: dout[b] added to every id of example b, in (b, i) order."""
    B, n = w_ids.shape
    vals = torch.zeros((B * n, 4), dtype=torch.float32, device=dout.device)
    vals[:, 0] = dout.repeat_interleave(n)
    return _dense_row_grad(w_ids, vals, rows, 1)


def _row_grad(dout: torch.Tensor) -> torch.Tensor:
    return dout.float().reshape(-1).contiguous()


class _FmDenseFn(torch.autograd.Function):
    """New_FM: out = rf_fm_fwd(x, w[w_ids]); dx = rf_fm_bwd, dw = the per-id sums of dout."""

    @staticmethod
    def forward(ctx, x, w, w_ids):
        ctx.save_for_backward(x, w_ids)
        ctx.w_rows = None if w is None else w.shape[0]
        return fm_forward(embed=x, w=w, w_ids=w_ids)

    @staticmethod
    def backward(ctx, dout):
        x, w_ids = ctx.saved_tensors
        g = _row_grad(dout)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            B, fields, dim = x.shape
            dx = torch.empty((B, fields, dim), dtype=torch.float32, device=x.device)
            L.call("rf_fm_bwd", L.ptr(x), L.torch_dtype_code(x.dtype), x.stride(0), x.stride(1), None, None, 0, 0, B, fields,
                   dim, L.ptr(g), L.ptr(dx), dx.stride(0), dx.stride(1), L.stream_ptr())
            if dx.dtype != x.dtype:
                dx = dx.to(x.dtype)
        if ctx.w_rows is not None and ctx.needs_input_grad[1]:
            dw = _first_order_grad(g, w_ids, ctx.w_rows)
        return dx, dw, None


class _FmGatherFn(torch.autograd.Function):
    """FM_Layer: out = rf_fm_fwd(V[ids], w0, w[ids]); dV = rf_fm_bwd's position rows summed per id, dw, dw0."""

    @staticmethod
    def forward(ctx, V, w, w0, ids):
        ctx.save_for_backward(V, ids)
        return fm_forward(V=V, ids=ids, w0=w0, w=w, w_ids=ids)

    @staticmethod
    def backward(ctx, dout):
        V, ids = ctx.saved_tensors
        g = _row_grad(dout)
        B, fields = ids.shape
        rows, k = V.shape
        dV = dw = dw0 = None
        if ctx.needs_input_grad[0]:
            kp = (k + 3) // 4 * 4
            pos = (torch.empty if kp == k else torch.zeros)((B * fields, kp), dtype=torch.float32, device=V.device)
            L.call("rf_fm_bwd", None, L.DT_F32, 0, 0, L.ptr(V), L.ptr(ids), ids.stride(0), rows, B, fields, k, L.ptr(g),
                   L.ptr(pos), fields * kp, kp, L.stream_ptr())
            dV = _dense_row_grad(ids, pos, rows, k)
        if ctx.needs_input_grad[1]:
            dw = _first_order_grad(g, ids, rows)
        if ctx.needs_input_grad[2]:
            dw0 = g.sum().reshape(1)
        return dV, dw, dw0, None


class _CrossFn(torch.autograd.Function):
    """out[:, :dim] = rf_cross_fwd(x) written through ldo into a [B, dim + right width] buffer whose right columns
    take `right` (the concat of DCN); backward = rf_cross_bwd reading its dout in place (lddo)."""

    @staticmethod
    def forward(ctx, x, w, b, right):
        B, dim = x.shape
        extra = 0 if right is None else right.shape[1]
        out = torch.empty((B, dim + extra), dtype=torch.float32, device=x.device)
        L.call("rf_cross_fwd", L.ptr(x), L.torch_dtype_code(x.dtype), x.stride(0), B, dim, w.shape[0], L.ptr(w), L.ptr(b),
               L.ptr(out), out.stride(0), L.stream_ptr())
        if right is not None:
            out[:, dim:] = right
        ctx.save_for_backward(x, w, b)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w, b = ctx.saved_tensors
        B, dim = x.shape
        layers = w.shape[0]
        dout = dout.float()
        if dout.stride(1) != 1:
            dout = dout.contiguous()
        dx = torch.empty((B, dim), dtype=torch.float32, device=x.device)
        dw, db = torch.empty_like(w), torch.empty_like(b)
        if B == 0:
            dw.zero_()
            db.zero_()
        wsb = int(L.load().rf_cross_bwd_ws_bytes(B, dim, layers))
        if wsb == 0:
            L.check(L.RF_EINVAL, "rf_cross_bwd_ws_bytes")
        ws = torch.empty(wsb, dtype=torch.uint8, device=x.device)
        L.call("rf_cross_bwd", L.ptr(x), L.torch_dtype_code(x.dtype), x.stride(0), B, dim, layers, L.ptr(w), L.ptr(b),
               L.ptr(dout), dout.stride(0), L.ptr(dx), dx.stride(0), L.ptr(dw), L.ptr(db), L.ptr(ws), ws.numel(),
               L.stream_ptr())
        if dx.dtype != x.dtype:
            dx = dx.to(x.dtype)
        dright = dout[:, dim:] if ctx.needs_input_grad[3] else None
        return dx, dw, db, dright


def _l2(c, t):
    return c * torch.sum(torch.square(t))


class TrainFMLayer(FM_Layer):
    """FM_Layer under training: gradients reach V, w and w0. The per-id sums of the batch are scattered into dense
    .grad tensors whose untouched rows are zero, which is what Keras' non-lazy Adam sees for an IndexedSlices gradient.
    That suits a vocabulary-sized feature_length (a dense optimizer walks every row each step), not the hashed table
    of the fused encoder, which trains through SparseAdam."""

    def build(self, input_shape=None):
        super().build(input_shape)
        for p in (self.w0, self.w, self.V):
            p.requires_grad_(True)

    def forward(self, inputs: Dict[str, torch.Tensor]) -> torch.Tensor:
        if self.V is None:
            self.build()
        ids = _concat_ids(index_mapping(inputs, self.map_dict), self.V.device)
        return _FmGatherFn.apply(self.V, self.w, self.w0, ids)

    def regularization(self) -> torch.Tensor:
        return _l2(self.w_reg, self.w) + _l2(self.v_reg, self.V)


class TrainNewFM(New_FM):
    """New_FM under training: the gradient reaches embed_inputs (rf_fm_bwd, f32 written once) and w (the per-id sums of
    dout). inputs['sparse_inputs'] may be None or absent: no first-order term (and feature_length may be 0)."""

    def build(self, input_shape=None):
        super().build(input_shape)
        self.w.requires_grad_(True)

    def forward(self, inputs, **kwargs) -> torch.Tensor:
        x = _dense_view(inputs['embed_inputs'])
        sparse_inputs = inputs.get('sparse_inputs')
        if sparse_inputs is None:
            return _FmDenseFn.apply(x, None, None)
        if self.w is None:
            self.build()
        return _FmDenseFn.apply(x, self.w, _concat_ids(sparse_inputs, self.w.device))

    def regularization(self) -> torch.Tensor:
        return _l2(self.w_reg, self.w)


class TrainCrossNetwork(CrossNetwork):
    """CrossNetwork under training: gradients reach the input, w and b (rf_cross_bwd). forward(x, concat=t) returns
    [B, dim + t.shape[1]]: the cross output written straight into the left columns of the concat buffer, t in the right
    ones."""

    def build(self, input_shape):
        super().build(input_shape)
        self.w.requires_grad_(True)
        self.b.requires_grad_(True)

    def forward(self, inputs: torch.Tensor, concat: Optional[torch.Tensor] = None) -> torch.Tensor:
        if self.w is None:
            self.build(inputs.shape)
        if self.layer_num == 0:
            return inputs if concat is None else torch.cat([inputs.float(), concat], dim=1)
        x = inputs if inputs.dtype in (torch.float32, torch.bfloat16) else inputs.float()
        if x.dim() != 2:
            raise ValueError(f"expected [batch, dim], got {tuple(x.shape)}")
        if x.shape[1] > 1 and x.stride(1) != 1:
            x = x.contiguous()
        return _CrossFn.apply(x, self.w, self.b, concat)

    def regularization(self) -> torch.Tensor:
        return _l2(self.reg_w, self.w) + _l2(self.reg_b, self.b)


class _CinFn(torch.autograd.Function):
    """out[:, :sum H] = rf_cin_fwd(x) written through ldo into a [B, sum H + right width] buffer whose right columns
    take `right` (the concat of xDeepFM); backward = rf_cin_bwd reading its dout in place (lddo). Ws are the layer's
    master weights (autograd hands their gradients back in the Keras filter shape); the kernels read layer._packed,
    and the backward packs the transposed image from the master weights."""

    @staticmethod
    def forward(ctx, x, layer, right, *Ws):
        B, fields, dim = x.shape
        K, sumH = len(layer.cin_size), sum(layer.cin_size)
        extra = 0 if right is None else right.shape[1]
        lib = L.load()
        wsb = int(lib.rf_cin_ws_bytes(B, fields, dim, layer._sizes, K))
        if wsb == 0:
            L.check(L.RF_EINVAL, "rf_cin_ws_bytes")
        ws = torch.empty(wsb, dtype=torch.uint8, device=x.device)
        out = torch.empty((B, sumH + extra), dtype=torch.float32, device=x.device)
        L.call("rf_cin_fwd", L.ptr(x), L.torch_dtype_code(x.dtype), x.stride(0), x.stride(1), B, fields, dim, layer._sizes, K,
               L.ptr(layer._packed), L.ptr(out), out.stride(0), L.ptr(ws), ws.numel(), L.stream_ptr())
        if right is not None:
            out[:, sumH:] = right
        ctx.save_for_backward(x)
        ctx.layer, ctx.packed = layer, layer._packed
        return out

    @staticmethod
    def backward(ctx, dout):
        (x,) = ctx.saved_tensors
        layer = ctx.layer
        B, fields, dim = x.shape
        K, sumH = len(layer.cin_size), sum(layer.cin_size)
        dout = dout.float()
        if dout.stride(1) != 1:
            dout = dout.contiguous()
        dx = torch.empty((B, fields, dim), dtype=torch.float32, device=x.device)
        dWs = [torch.empty_like(layer.cin_W['CIN_W_' + str(i)], dtype=torch.float32) for i in range(K)]
        if B == 0:
            for d in dWs:
                d.zero_()
        lib = L.load()
        wsb = int(lib.rf_cin_bwd_ws_bytes(B, fields, dim, layer._sizes, K))
        if wsb == 0:
            L.check(L.RF_EINVAL, "rf_cin_bwd_ws_bytes")
        ws = torch.empty(wsb, dtype=torch.uint8, device=x.device)
        packed_t = layer._pack_transposed()
        ptrs = (ctypes.c_void_p * K)(*[d.data_ptr() for d in dWs])
        L.call("rf_cin_bwd", L.ptr(x), L.torch_dtype_code(x.dtype), x.stride(0), x.stride(1), B, fields, dim, layer._sizes, K,
               L.ptr(ctx.packed), L.ptr(packed_t), L.ptr(dout), dout.stride(0), L.ptr(dx), dx.stride(0), dx.stride(1),
               ptrs, L.ptr(ws), ws.numel(), L.stream_ptr())
        if dx.dtype != x.dtype:
            dx = dx.to(x.dtype)
        dright = dout[:, sumH:] if ctx.needs_input_grad[2] else None
        return (dx if ctx.needs_input_grad[0] else None, None, dright, *dWs)


class TrainCIN(CIN):
    """CIN under training: gradients reach the input and every cin_W (rf_cin_bwd; the activations are recomputed, the
    forward saves x only). forward(x, concat=t) returns [B, sum(cin_size) + t.shape[1]]: the CIN output written
    straight into the left columns of the concat buffer, t in the right ones.

    The optimizer writes the master weights through raw pointers, which no torch version counter sees, so in
    training mode the bf16 image is packed from them on every forward (and its transpose in the backward); in eval
    mode it is packed lazily as CIN does. train() / eval() and load_state_dict drop the cached image."""

    def build(self, input_shape):
        super().build(input_shape)
        for p in self.cin_W.values():
            p.requires_grad_(True)

    def train(self, mode: bool = True):
        self._packed = None
        return super().train(mode)

    def _pack_transposed(self) -> torch.Tensor:
        K = len(self.cin_size)
        nbytes = int(L.load().rf_cin_bwd_packed_w_bytes(self.embedding_nums, self._sizes, K))
        if nbytes == 0:
            L.check(L.RF_EINVAL, "rf_cin_bwd_packed_w_bytes")
        packed = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        for i in range(K):
            W = self.cin_W['CIN_W_' + str(i)].data.float().contiguous()
            L.call("rf_cin_bwd_pack_w", L.ptr(W), i, self.embedding_nums, self._sizes, K, L.ptr(packed), L.stream_ptr())
        return packed

    def forward(self, inputs: torch.Tensor, concat: Optional[torch.Tensor] = None) -> torch.Tensor:
        x = _dense_view(inputs)
        if self.embedding_nums is None:
            self.build(x.shape)
        if x.shape[1] != self.embedding_nums:
            raise ValueError(f"CIN was built for {self.embedding_nums} fields, got {x.shape[1]}")
        if self.training or self._packed is None:
            self.refresh()
        Ws = [self.cin_W['CIN_W_' + str(i)] for i in range(len(self.cin_size))]
        return _CinFn.apply(x, self, concat, *Ws)

    def regularization(self) -> torch.Tensor:
        return sum(_l2(self.l2_reg, p) for p in self.cin_W.values())


# the order of rf_tfenc_pack's parameters and of rf_tfenc_bwd's grads, per block
_TFENC_ABI = ("wq_kernel", "wq_bias", "wk_kernel", "wk_bias", "wv_kernel", "wv_bias", "ln1_gamma", "ln1_beta",
              "conv1_kernel", "conv1_bias", "conv2_kernel", "conv2_bias", "ln2_gamma", "ln2_beta")


def _tfenc_pack_transposed(blocks) -> torch.Tensor:
    """rf_tfenc_bwd_pack: the bf16 copies of every block's five kernels that rf_tfenc_bwd reads, from the masters."""
    lead, n = blocks[0], len(blocks)
    nbytes = int(L.load().rf_tfenc_bwd_packed_bytes(lead.d_model, lead.ffn_hidden_unit, n))
    if nbytes == 0:
        L.check(L.RF_EINVAL, "rf_tfenc_bwd_packed_bytes")
    packed = torch.empty(nbytes, dtype=torch.uint8, device=lead.wq_kernel.device)
    with torch.no_grad():
        for i, blk in enumerate(blocks):
            # Dense keeps [out][in]; the ABI takes the Keras (in, out) kernels
            kern = [getattr(blk, nm).detach().t().contiguous()
                    for nm in ("wq_kernel", "wk_kernel", "wv_kernel", "conv1_kernel", "conv2_kernel")]
            L.call("rf_tfenc_bwd_pack", i, lead.d_model, lead.ffn_hidden_unit, n, *[L.ptr(k) for k in kern], L.ptr(packed),
                   L.stream_ptr())
    return packed


class _TfencFn(torch.autograd.Function):
    """out = rf_tfenc_fwd(x) over the whole stack (into `out` if given: a view of the caller's buffer, marked dirty, so
    that the gradient of whatever reads the buffer comes back here; autograd's in-place bookkeeping needs it to be the
    first input); backward = rf_tfenc_bwd reading dout in place through its strides. Saves x and the mask only: the kernel recomputes.
    params are the blocks' 14 master parameters each, in _TFENC_ABI order (autograd hands their gradients back in the
    masters' own layouts); the kernels read the packed images."""

    @staticmethod
    def forward(ctx, out, x, blocks, mask, packed, *params):
        B, Ln, d = x.shape
        lead, n = blocks[0], len(blocks)
        if out is None:
            out = torch.empty((B, Ln, d), dtype=torch.float32, device=x.device)
        else:
            ctx.mark_dirty(out)
        L.call("rf_tfenc_fwd", L.ptr(x), L.torch_dtype_code(x.dtype), x.stride(0), x.stride(1), L.ptr(mask), B, Ln, d,
               lead.num_heads, lead.ffn_hidden_unit, n, L.ptr(packed), lead.layer_norm_eps, L.ptr(out), out.stride(0),
               out.stride(1), L.stream_ptr())
        ctx.save_for_backward(x, mask)
        ctx.blocks, ctx.packed = blocks, packed
        return out

    @staticmethod
    def backward(ctx, dout):
        x, mask = ctx.saved_tensors
        blocks = ctx.blocks
        lead, n = blocks[0], len(blocks)
        B, Ln, d = x.shape
        ffn = lead.ffn_hidden_unit
        dout = dout.float()
        if (d > 1 and dout.stride(2) != 1) or dout.stride(1) < d or dout.stride(0) < 0:  # e.g. an expanded scalar
            dout = dout.contiguous()
        dev = x.device
        if B == 0:  # an empty tensor keeps whatever strides it has
            dout = torch.empty((0, Ln, d), dtype=torch.float32, device=dev)
        dx = torch.empty((B, Ln, d), dtype=torch.float32, device=dev)
        keras = {"wq_kernel": (d, d), "wk_kernel": (d, d), "wv_kernel": (d, d), "conv1_kernel": (d, ffn),
                 "conv2_kernel": (ffn, d), "conv1_bias": (ffn,)}
        alloc = torch.zeros if B == 0 else torch.empty
        grads = [alloc(keras.get(nm, (d,)), dtype=torch.float32, device=dev) for _ in blocks for nm in _TFENC_ABI]
        wsb = int(L.load().rf_tfenc_bwd_ws_bytes(B, Ln, d, lead.num_heads, ffn, n))
        if wsb == 0:
            L.check(L.RF_EINVAL, "rf_tfenc_bwd_ws_bytes")
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        packed_t = _tfenc_pack_transposed(blocks)
        ptrs = (ctypes.c_void_p * len(grads))(*[g.data_ptr() for g in grads])
        L.call("rf_tfenc_bwd", L.ptr(x), L.torch_dtype_code(x.dtype), x.stride(0), x.stride(1), L.ptr(mask), B, Ln, d,
               lead.num_heads, ffn, n, L.ptr(ctx.packed), L.ptr(packed_t), lead.layer_norm_eps, L.ptr(dout), dout.stride(0),
               dout.stride(1), L.ptr(dx), dx.stride(0), dx.stride(1), ptrs, L.ptr(ws), ws.numel(), L.stream_ptr())
        if dx.dtype != x.dtype:
            dx = dx.to(x.dtype)
        # the masters' layouts: Dense keeps its kernel as [out][in]
        grads = [g.t().contiguous() if g.dim() == 2 else g for g in grads]
        return (None, dx if ctx.needs_input_grad[1] else None, None, None, None, *grads)


class TrainTransformerEncoder(TransformerEncoder):
    """TransformerEncoder under training: the fourteen tensors are Parameters under the names of TransformerEncoder's
    buffers (the two classes load each other's state dicts; mha, ffn, layernorm1 and layernorm2 still see the same
    storage), gradients reach them and the input through rf_tfenc_bwd (everything is recomputed; the forward saves x and
    the mask only). regularization() is l2_reg * the sum of the five kernels squared.

    The optimizer writes the masters through raw pointers, which no torch version counter sees, so in training mode the
    forward image is packed from them on every forward and the transposed image in the backward; eval packs lazily as
    TransformerEncoder does. train() / eval() and load_state_dict drop the cached image. The kernel has no dropout:
    dropout > 0 in training mode raises ValueError (deviation D-tfenc-dropout; the reference's default is 0)."""

    def __init__(self, d_model, num_heads=1, ffn_hidden_unit=128, dropout=0., layer_norm_eps=1e-6, l2_reg: float = 0.,
                 seed: int = 0, device="cuda"):
        super().__init__(d_model, num_heads=num_heads, ffn_hidden_unit=ffn_hidden_unit, dropout=dropout,
                         layer_norm_eps=layer_norm_eps, seed=seed, device=device)
        self.l2_reg = float(l2_reg)
        for name, _ in self._STATE:
            t = self._buffers.pop(name)
            self.register_parameter(name, torch.nn.Parameter(t))  # the sub-layer's tensor: the same storage

    def train(self, mode: bool = True):
        self.refresh()
        return super().train(mode)

    def forward(self, inputs, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        x, mask = inputs
        return train_transformer_encoder_stack([self], x, mask, out=out)

    def regularization(self) -> torch.Tensor:
        return sum(_l2(self.l2_reg, getattr(self, n)) for n in ("wq_kernel", "wk_kernel", "wv_kernel", "conv1_kernel",
                                                                "conv2_kernel"))


def train_transformer_encoder_stack(blocks: Sequence[TrainTransformerEncoder], x: torch.Tensor,
                                    mask: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """transformer_encoder_stack under training: ONE autograd node over the whole stack, rf_tfenc_fwd forward (into `out`
    if given, e.g. the left columns of a concat buffer viewed as [B, L, d_model]) and rf_tfenc_bwd backward. dx comes
    back in x's dtype, rounded once. With every block in eval mode, or without grad, it is transformer_encoder_stack."""
    blocks = list(blocks)
    if not blocks:
        raise ValueError("train_transformer_encoder_stack needs at least one block")
    training = any(blk.training for blk in blocks)
    if training:
        for blk in blocks:
            if blk.dropout > 0:
                raise ValueError(f"TrainTransformerEncoder: dropout ({blk.dropout}) > 0 cannot be trained: rf_tfenc_fwd has "
                                 "no dropout")
    if not training or not torch.is_grad_enabled():
        with torch.no_grad():
            if training:
                for blk in blocks:
                    blk.refresh()
            return transformer_encoder_stack(blocks, x, mask, out=out)
    L.require_gpu()
    lead = blocks[0]
    for blk in blocks[1:]:
        if blk.shape_key() != lead.shape_key():
            raise ValueError(f"blocks of one stack must have equal shapes: {blk.shape_key()} != {lead.shape_key()}")
    x = _dense_view(x)
    B, Ln, d = x.shape
    if d != lead.d_model:
        raise ValueError(f"TransformerEncoder was built for d_model {lead.d_model}, got {d}")
    n = len(blocks)
    nbytes = int(L.load().rf_tfenc_packed_bytes(lead.d_model, lead.ffn_hidden_unit, n))
    if nbytes == 0:
        L.check(L.RF_EINVAL, "rf_tfenc_packed_bytes")
    if int(L.load().rf_tfenc_bwd_ws_bytes(B, Ln, d, lead.num_heads, lead.ffn_hidden_unit, n)) == 0:
        L.check(L.RF_EINVAL, "rf_tfenc_bwd_ws_bytes")  # fail before the forward
    packed = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    with torch.no_grad():
        for i, blk in enumerate(blocks):
            blk._pack_into(packed, i, n)
    m = None
    if mask is not None:
        m = mask.reshape(B, Ln).to(device=x.device, dtype=torch.float32).contiguous()
    if out is not None and (out.dtype != torch.float32 or tuple(out.shape) != (B, Ln, d) or (d > 1 and out.stride(2) != 1)):
        raise ValueError(f"out must be an F32 [{B}, {Ln}, {d}] view with unit stride on the last axis")
    params = [getattr(blk, nm) for blk in blocks for nm in _TFENC_ABI]
    return _TfencFn.apply(out, x, blocks, m, packed, *params)
