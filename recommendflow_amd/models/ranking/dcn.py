"""Deep & Cross Network on the MI355X hot path. The reference's models/ranking/dcn.py is an empty file; the model is
defined by CrossNetwork's docstring ("CrossNetwork of DCN", backend/layers/network_layers.py:130-171), create_mlp
(backend/blocks/mlp.py:4-15) and the paper (Wang et al. 2017): logit = Dense(1)(concat(Cross(x), MLP(x)))
(deviation D-rankers-empty).

Here: ONE fused encoder (runtime.train.embed); TrainCrossNetwork (rf_cross_fwd / rf_cross_bwd) writes its output
through ldo straight into the left columns of the concat buffer, the TrainTower output takes the right columns, and
TrainLinear(1) reads the buffer. Sigmoid cross-entropy plus reg_w * sum(w^2) + reg_b * sum(b^2).
"""
from __future__ import annotations

import torch

from .ranker_base import TrainableRanker


class TrainableDCN(TrainableRanker):
    def __init__(self, encoder, layer_num: int = 3, hidden_units=(256, 128), dropout: float = 0.3, reg_w: float = 0.,
                 reg_b: float = 0., learning_rate: float = 1e-3, seed: int = 0, lazy_adam: bool = False,
                 deferred_adam=None):
        super().__init__(encoder)
        from ...backend.blocks.train_mlp import TrainLinear, TrainTower
        from ...backend.layers.network_layers import TrainCrossNetwork

        g = torch.Generator().manual_seed(seed)
        dev = encoder.table.device
        width = int(encoder.out_width)
        self.tower = TrainTower(width, list(hidden_units), rate=dropout, eps=1e-6, seed=64 * seed + 1, generator=g,
                                device=dev)
        self.cross = TrainCrossNetwork(layer_num, reg_w=reg_w, reg_b=reg_b, seed=seed, device=dev)
        self.cross.build((None, width))
        self.head = TrainLinear(width + self.tower.out_features, 1, generator=g, device=dev)
        self._init_optimizers(learning_rate, lazy_adam, deferred_adam)

    def _logits(self, x: torch.Tensor) -> torch.Tensor:
        cat = self.cross(x, concat=self.tower(x))
        return self.head(cat).reshape(x.shape[0])

    def regularization(self):
        return self.cross.regularization()
