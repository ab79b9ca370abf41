"""Feature-interaction layers (reference: backend/layers/network_layers.py), forward on rf_interact.hip:

  FM_Layer, New_FM  -> rf_fm_fwd     (:43-56, :193-207)
  CrossNetwork      -> rf_cross_fwd  (:163-171)
  CIN               -> rf_cin_fwd    (:238-255)

Weights are created on the first call from the input shape, as Keras `build` does: 'random_normal' and
tf.random_normal_initializer() are N(0, 0.05^2), w0 starts at zero. The regularisation coefficients are kept and have
no effect on a forward. Inference only: the backward of these layers is not implemented.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, Optional, Sequence

import torch

from ...runtime import lib as L
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
