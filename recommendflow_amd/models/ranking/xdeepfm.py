"""xDeepFM on the MI355X hot path. The reference's models/ranking/xdeepfm.py is an empty file; the model is defined by
CIN's docstring ("CIN of xDeepFM", backend/layers/network_layers.py:210-255), create_mlp (backend/blocks/mlp.py:4-15)
and the paper (Lian et al. 2018): logit = Dense(1)(concat(CIN(x as [B, S, 2D]), MLP(x))) (deviation D-rankers-empty,
DESIGN §4.9.2). The paper's linear (first-order) part over the raw sparse ids is left out for the reason given for
DeepFM's (deviation D-deepfm-first-order): the fused encoder hashes tokens into one shared table and keeps no
per-feature vocabulary that a first-order weight could be indexed by.

Here: ONE fused encoder (runtime.train.embed); TrainCIN (rf_cin_fwd / rf_cin_bwd) reads the embed output in place as
[B, S, 2D] and writes its [B, sum(cin_size)] output through ldo straight into the left columns of the concat buffer,
the TrainTower output takes the right columns, and TrainLinear(1) reads the buffer. Sigmoid cross-entropy plus
l2_reg * sum_k sum(W_k^2).
"""
from __future__ import annotations

import torch

from .ranker_base import TrainableRanker


class TrainableXDeepFM(TrainableRanker):
    def __init__(self, encoder, cin_size=(128, 128), hidden_units=(256, 128), dropout: float = 0.3, l2_reg: float = 0.,
                 learning_rate: float = 1e-3, seed: int = 0, lazy_adam: bool = False, deferred_adam=None):
        super().__init__(encoder)
        from ...backend.blocks.train_mlp import TrainLinear, TrainTower
        from ...backend.layers.network_layers import TrainCIN

        g = torch.Generator().manual_seed(seed)
        dev = encoder.table.device
        width = int(encoder.out_width)
        self.tower = TrainTower(width, list(hidden_units), rate=dropout, eps=1e-6, seed=64 * seed + 1, generator=g,
                                device=dev)
        self.cin = TrainCIN(list(cin_size), l2_reg=l2_reg, seed=seed, device=dev)
        self.cin.build((None, self.n_slots, self.width))
        self.head = TrainLinear(sum(self.cin.cin_size) + self.tower.out_features, 1, generator=g, device=dev)
        self._init_optimizers(learning_rate, lazy_adam, deferred_adam)

    def _logits(self, x: torch.Tensor) -> torch.Tensor:
        B = x.shape[0]
        cat = self.cin(x.view(B, self.n_slots, self.width), concat=self.tower(x))
        return self.head(cat).reshape(B)

    def regularization(self):
        return self.cin.regularization()
