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
from ...runtime.segment import segment_sum_rows
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
        x = _cross_input(inputs)
        return _cross_fwd(x, self.w.data, self.b.data, torch.empty(x.shape, dtype=torch.float32, device=x.device))


def _cross_input(x: torch.Tensor) -> torch.Tensor:
    """A [B, dim] view rf_cross_fwd reads in place: f32 or bf16, dim contiguous, any batch stride."""
    if x.dtype not in (torch.float32, torch.bfloat16):
        x = x.float()
    if x.dim() != 2:
        raise ValueError(f"expected [batch, dim], got {tuple(x.shape)}")
    if x.shape[1] > 1 and x.stride(1) != 1:
        x = x.contiguous()
    return x


def _cross_fwd(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """rf_cross_fwd of x [B, dim] through the layers w, b [layer_num, dim] into the left dim columns of out (F32, at
    least dim wide: its row stride is the kernel's ldo)."""
    B, dim = x.shape
    L.call("rf_cross_fwd", L.ptr(x), L.torch_dtype_code(x.dtype), x.stride(0), B, dim, w.shape[0], L.ptr(w), L.ptr(b),
           L.ptr(out), out.stride(0), L.stream_ptr())
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

    def _pack(self, transposed: bool) -> torch.Tensor:
        """The bf16 image of the fp32 master weights that rf_cin_fwd reads, or the transposed one of rf_cin_bwd."""
        K = len(self.cin_size)
        size_fn = "rf_cin_bwd_packed_w_bytes" if transposed else "rf_cin_packed_w_bytes"
        packed = L.workspace(size_fn, self.device, self.embedding_nums, self._sizes, K, must=True)
        for i in range(K):
            W = self.cin_W['CIN_W_' + str(i)].data.float().contiguous()
            if transposed:
                L.call("rf_cin_bwd_pack_w", L.ptr(W), i, self.embedding_nums, self._sizes, K, L.ptr(packed), L.stream_ptr())
            else:
                L.call("rf_cin_pack_w", L.ptr(W), i, self.embedding_nums, self._sizes, K, L.ptr(packed), L.stream_ptr())
        return packed

    def refresh(self):
        """Rebuild the bf16 kernel image from the fp32 master weights."""
        self._packed = self._pack(False)

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
        return _cin_fwd(x, self, torch.empty((B, sum(self.cin_size)), dtype=torch.float32, device=x.device))


def _cin_fwd(x: torch.Tensor, layer: "CIN", out: torch.Tensor) -> torch.Tensor:
    """rf_cin_fwd of x [B, fields, dim] through layer._packed into the left sum(cin_size) columns of out (F32, at least
    that wide: its row stride is the kernel's ldo)."""
    B, fields, dim = x.shape
    K = len(layer.cin_size)
    ws = L.workspace("rf_cin_ws_bytes", x.device, B, fields, dim, layer._sizes, K, must=True)
    L.call("rf_cin_fwd", L.ptr(x), L.torch_dtype_code(x.dtype), x.stride(0), x.stride(1), B, fields, dim, layer._sizes, K,
           L.ptr(layer._packed), L.ptr(out), out.stride(0), L.ptr(ws), ws.numel(), L.stream_ptr())
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

    def _pack_into(self, packed: torch.Tensor, block: int, n_blocks: int, transposed: bool = False):
        """This block's part of a stack's image (_tfenc_image): the fourteen masters for rf_tfenc_fwd, or, transposed,
        the five kernels for rf_tfenc_bwd."""
        with torch.no_grad():
            src = [getattr(self, nm).detach() for nm in (_TFENC_KERNELS if transposed else _TFENC_ABI)]
            # Dense keeps [out][in]; the ABI takes the Keras (in, out) kernels
            src = [t.t().contiguous() if t.dim() == 2 else t for t in src]
            ptrs = [L.ptr(t) for t in src]
            if transposed:
                L.call("rf_tfenc_bwd_pack", block, self.d_model, self.ffn_hidden_unit, n_blocks, *ptrs, L.ptr(packed),
                       L.stream_ptr())
            else:
                L.call("rf_tfenc_pack", block, self.d_model, self.ffn_hidden_unit, n_blocks, *ptrs, L.ptr(packed),
                       L.stream_ptr())

    def forward(self, inputs, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        x, mask = inputs
        return transformer_encoder_stack([self], x, mask, out=out)


# the order of rf_tfenc_pack's parameters and of rf_tfenc_bwd's grads, per block
_TFENC_ABI = ("wq_kernel", "wq_bias", "wk_kernel", "wk_bias", "wv_kernel", "wv_bias", "ln1_gamma", "ln1_beta",
              "conv1_kernel", "conv1_bias", "conv2_kernel", "conv2_bias", "ln2_gamma", "ln2_beta")
# the five matrices among them, in the order of rf_tfenc_bwd_pack's parameters
_TFENC_KERNELS = tuple(nm for nm in _TFENC_ABI if nm.endswith("_kernel"))


def _tfenc_inputs(who: str, blocks, x: torch.Tensor, mask: Optional[torch.Tensor]):
    """The checks of a stack and its inputs -> (blocks[0], len(blocks), x as rf_tfenc_fwd reads it, the mask as F32
    [B, L] or None)."""
    L.require_gpu()
    if not blocks:
        raise ValueError(f"{who} needs at least one block")
    lead = blocks[0]
    for blk in blocks[1:]:
        if blk.shape_key() != lead.shape_key():
            raise ValueError(f"blocks of one stack must have equal shapes: {blk.shape_key()} != {lead.shape_key()}")
    x = _dense_view(x)
    B, Ln, d = x.shape
    if d != lead.d_model:
        raise ValueError(f"TransformerEncoder was built for d_model {lead.d_model}, got {d}")
    m = None
    if mask is not None:
        m = mask.reshape(B, Ln).to(device=x.device, dtype=torch.float32).contiguous()
    return lead, len(blocks), x, m


def _tfenc_check_out(out: Optional[torch.Tensor], x: torch.Tensor):
    B, Ln, d = x.shape
    if out is not None and (out.dtype != torch.float32 or tuple(out.shape) != (B, Ln, d) or (d > 1 and out.stride(2) != 1)):
        raise ValueError(f"out must be an F32 [{B}, {Ln}, {d}] view with unit stride on the last axis")


def _tfenc_image(blocks, transposed: bool = False) -> torch.Tensor:
    """The packed image of every block's fp32 masters: the one rf_tfenc_fwd reads (rf_tfenc_pack, all fourteen tensors),
    or the bf16 copies of the five kernels that rf_tfenc_bwd reads beside it (rf_tfenc_bwd_pack)."""
    lead, n = blocks[0], len(blocks)
    size_fn = "rf_tfenc_bwd_packed_bytes" if transposed else "rf_tfenc_packed_bytes"
    packed = L.workspace(size_fn, lead.wq_kernel.device, lead.d_model, lead.ffn_hidden_unit, n, must=True)
    for i, blk in enumerate(blocks):
        blk._pack_into(packed, i, n, transposed)
    return packed


def _tfenc_pack_transposed(blocks) -> torch.Tensor:
    """rf_tfenc_bwd_pack: the bf16 copies of every block's five kernels that rf_tfenc_bwd reads, from the masters."""
    return _tfenc_image(blocks, transposed=True)


def _tfenc_fwd(lead: TransformerEncoder, n: int, x: torch.Tensor, m: Optional[torch.Tensor], packed: torch.Tensor,
               out: Optional[torch.Tensor]) -> torch.Tensor:
    """rf_tfenc_fwd of the n blocks in `packed` into out (checked by _tfenc_check_out), or into a new F32 [B, L, d]."""
    B, Ln, d = x.shape
    if out is None:
        out = torch.empty((B, Ln, d), dtype=torch.float32, device=x.device)
    L.call("rf_tfenc_fwd", L.ptr(x), L.torch_dtype_code(x.dtype), x.stride(0), x.stride(1), L.ptr(m), B, Ln, d, lead.num_heads,
           lead.ffn_hidden_unit, n, L.ptr(packed), lead.layer_norm_eps, L.ptr(out), out.stride(0), out.stride(1),
           L.stream_ptr())
    return out


def transformer_encoder_stack(blocks: Sequence[TransformerEncoder], x: torch.Tensor, mask: Optional[torch.Tensor] = None,
                              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """blocks[-1](... blocks[0]([x, mask]) ..., mask) in ONE rf_tfenc_fwd launch through one packed image of all blocks
    (cached on blocks[0] until one of them is refreshed or reloaded). The blocks must have equal shapes (d_model,
    num_heads, ffn_hidden_unit, layer_norm_eps): ValueError otherwise."""
    blocks = list(blocks)
    lead, n, x, m = _tfenc_inputs("transformer_encoder_stack", blocks, x, mask)
    key = tuple((id(blk), blk._gen) for blk in blocks)
    if lead._stack is None or lead._stack[0] != key:
        lead._stack = (key, _tfenc_image(blocks))
    _tfenc_check_out(out, x)
    return _tfenc_fwd(lead, n, x, m, lead._stack[1], out)


# ---- training ----------------------------------------------------------------------------------------------------------
def _dense_row_grad(ids: torch.Tensor, vals: torch.Tensor, rows: int, width: int) -> torch.Tensor:
    """The dense [rows, width] gradient of a table from its per-position gradient rows vals [n, >= width] (columns past
    `width` are padding to rf_segment_sum_rows' multiple of 4): per-id sums in position order, untouched rows zero.
    Reads the device count of distinct ids (one sync per 256 columns)."""
    out = torch.zeros((rows, width), dtype=torch.float32, device=vals.device)
    ids = ids.reshape(-1)
    for c0 in range(0, vals.shape[1], 256):
        blk = vals[:, c0: c0 + 256]
        uid, uval, n_uniq, _ = segment_sum_rows(ids, blk, rows)
        k = int(n_uniq.item())
        w = min(width - c0, blk.shape[1])
        if w > 0:
            out[uid[:k], c0: c0 + w] = uval[:k, :w]
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
        out = _cross_fwd(x, w, b, torch.empty((B, dim + extra), dtype=torch.float32, device=x.device))
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
        ws = L.workspace("rf_cross_bwd_ws_bytes", x.device, B, dim, layers, must=True)
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
        return _CrossFn.apply(_cross_input(inputs), self.w, self.b, concat)

    def regularization(self) -> torch.Tensor:
        return _l2(self.reg_w, self.w) + _l2(self.reg_b, self.b)


class _CinFn(torch.autograd.Function):
    """out[:, :sum H] = rf_cin_fwd(x) written through ldo into a [B, sum H + right width] buffer whose right columns
    take `right` (the concat of xDeepFM); backward = rf_cin_bwd reading its dout in place (lddo). Ws are the layer's
    master weights (autograd hands their gradients back in the Keras filter shape); the kernels read layer._packed,
    and the backward packs the transposed image from the master weights."""

    @staticmethod
    def forward(ctx, x, layer, right, *Ws):
        sumH = sum(layer.cin_size)
        extra = 0 if right is None else right.shape[1]
        out = _cin_fwd(x, layer, torch.empty((x.shape[0], sumH + extra), dtype=torch.float32, device=x.device))
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
        ws = L.workspace("rf_cin_bwd_ws_bytes", x.device, B, fields, dim, layer._sizes, K, must=True)
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
        return self._pack(True)

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


class _TfencFn(torch.autograd.Function):
    """out = rf_tfenc_fwd(x) over the whole stack (into `out` if given: a view of the caller's buffer, marked dirty, so
    that the gradient of whatever reads the buffer comes back here; autograd's in-place bookkeeping needs it to be the
    first input); backward = rf_tfenc_bwd reading dout in place through its strides. Saves x and the mask only: the kernel recomputes.
    params are the blocks' 14 master parameters each, in _TFENC_ABI order (autograd hands their gradients back in the
    masters' own layouts); the kernels read the packed images."""

    @staticmethod
    def forward(ctx, out, x, blocks, mask, packed, *params):
        if out is not None:
            ctx.mark_dirty(out)
        out = _tfenc_fwd(blocks[0], len(blocks), x, mask, packed, out)
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
        alloc = torch.zeros if B == 0 else torch.empty
        # in the Keras layouts: a master's shape reversed (Dense keeps its kernel as [out][in])
        grads = [alloc(getattr(lead, nm).shape[::-1], dtype=torch.float32, device=dev) for _ in blocks for nm in _TFENC_ABI]
        ws = L.workspace("rf_tfenc_bwd_ws_bytes", dev, B, Ln, d, lead.num_heads, ffn, n, must=True)
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
        return sum(_l2(self.l2_reg, getattr(self, n)) for n in _TFENC_KERNELS)


def train_transformer_encoder_stack(blocks: Sequence[TrainTransformerEncoder], x: torch.Tensor,
                                    mask: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """transformer_encoder_stack under training: ONE autograd node over the whole stack, rf_tfenc_fwd forward (into `out`
    if given, e.g. the left columns of a concat buffer viewed as [B, L, d_model]) and rf_tfenc_bwd backward. dx comes
    back in x's dtype, rounded once. With every block in eval mode, or without grad, it is transformer_encoder_stack."""
    blocks = list(blocks)
    training = any(blk.training for blk in blocks)
    if training:
        for blk in blocks:
            if blk.dropout > 0:
                raise ValueError(f"TrainTransformerEncoder: dropout ({blk.dropout}) > 0 cannot be trained: rf_tfenc_fwd has "
                                 "no dropout")
    if blocks and (not training or not torch.is_grad_enabled()):  # an empty stack is _tfenc_inputs' error below
        with torch.no_grad():
            if training:
                for blk in blocks:
                    blk.refresh()
            return transformer_encoder_stack(blocks, x, mask, out=out)
    lead, n, x, m = _tfenc_inputs("train_transformer_encoder_stack", blocks, x, mask)
    packed = _tfenc_image(blocks)  # on every forward: the optimizer writes the masters through raw pointers
    B, Ln, d = x.shape
    if int(L.load().rf_tfenc_bwd_ws_bytes(B, Ln, d, lead.num_heads, lead.ffn_hidden_unit, n)) == 0:
        L.check(L.RF_EINVAL, "rf_tfenc_bwd_ws_bytes")  # fail before the forward
    _tfenc_check_out(out, x)
    params = [getattr(blk, nm) for blk in blocks for nm in _TFENC_ABI]
    return _TfencFn.apply(out, x, blocks, m, packed, *params)
