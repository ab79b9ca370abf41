"""DeepFM on the MI355X hot path. The reference's models/ranking/deepfm.py is an empty file; the model is defined by
New_FM's docstring ("New Factorization Machine for DeepFm", backend/layers/network_layers.py:174-207), create_mlp
(backend/blocks/mlp.py:4-15) and the paper (Guo et al. 2017): logit = FM(embeddings) + Dense(1)(MLP(embeddings))
(deviation D-rankers-empty).

Here: ONE fused encoder (runtime.train.embed); its [B, S*2D] output is the FM's [B, S, 2D] embed_inputs read in place
(rf_fm_fwd / rf_fm_bwd) and the tower's input (TrainTower: BatchNormalization -> Dense(selu) -> Dropout per hidden
size, rf_gemm_f32), TrainLinear(1) on the tower, sigmoid cross-entropy plus w_reg * sum(w^2).

Deviation D-deepfm-first-order: the hashed encoder has no per-feature vocabulary, so New_FM's first-order ids cannot
come from it. With first_order_rows > 0 the caller passes first_ids (int64 [B, n], each in [0, first_order_rows)) and
the model owns the [first_order_rows, 1] weight; with 0 there is no first-order term.
"""
from __future__ import annotations

import torch

from .ranker_base import TrainableRanker


class TrainableDeepFM(TrainableRanker):
    def __init__(self, encoder, hidden_units=(256, 128), dropout: float = 0.3, first_order_rows: int = 0,
                 w_reg: float = 1e-6, learning_rate: float = 1e-3, seed: int = 0, lazy_adam: bool = False,
                 deferred_adam=None):
        super().__init__(encoder)
        from ...backend.blocks.train_mlp import TrainLinear, TrainTower
        from ...backend.layers.network_layers import TrainNewFM

        g = torch.Generator().manual_seed(seed)
        dev = encoder.table.device
        self.first_order_rows = int(first_order_rows)
        self.tower = TrainTower(encoder.out_width, list(hidden_units), rate=dropout, eps=1e-6, seed=64 * seed + 1,
                                generator=g, device=dev)
        self.head = TrainLinear(self.tower.out_features, 1, generator=g, device=dev)
        self.fm = TrainNewFM(self.first_order_rows, w_reg=w_reg, seed=seed, device=dev)
        if self.first_order_rows > 0:
            self.fm.build()
        self._init_optimizers(learning_rate, lazy_adam, deferred_adam)

    def _logits(self, x: torch.Tensor, first_ids=None) -> torch.Tensor:
        B = x.shape[0]
        if (first_ids is not None) != (self.first_order_rows > 0):
            raise ValueError("TrainableDeepFM: first_ids goes with first_order_rows > 0, and only with it")
        sparse = None if first_ids is None else {"first": first_ids}
        fm = self.fm({"embed_inputs": x.view(B, self.n_slots, self.width), "sparse_inputs": sparse})
        deep = self.head(self.tower(x))
        return (fm + deep).reshape(B)

    def regularization(self):
        return self.fm.regularization() if self.first_order_rows > 0 else 0.0
