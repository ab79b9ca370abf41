"""rf_segment_sum_rows: the per-id sums of gradient rows (the dense layers' table gradients, the sharded and the data
parallel sparse gradients)."""
from __future__ import annotations

import torch

from . import lib as L


def segment_sum_rows(ids: torch.Tensor, vals: torch.Tensor, id_range: int):
    """ids int64 [n], vals f32 [n, D] (D a multiple of 4, at most 256) -> (uid int64 [cap], uval f32 [cap, D], n_uniq
    int32 [1] on the device, cap): the first n_uniq entries are the distinct ids ascending and their rows summed in
    input order; ids outside [0, id_range) are dropped. No host read."""
    ids, vals = ids.contiguous(), vals.contiguous()
    n, D = vals.shape
    cap = max(1, min(n, id_range))
    dev = vals.device
    uid = torch.empty(cap, dtype=torch.int64, device=dev)
    uval = torch.empty((cap, D), dtype=torch.float32, device=dev)
    n_uniq = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = L.workspace("rf_segment_sum_ws_bytes", dev, n, id_range)
    L.call("rf_segment_sum_rows", L.ptr(ids), L.ptr(vals), n, D, id_range, L.ptr(uid), L.ptr(uval), cap, L.ptr(n_uniq),
           L.ptr(ws), ws.numel(), L.stream_ptr())
    return uid, uval, n_uniq, cap
