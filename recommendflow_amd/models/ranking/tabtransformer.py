"""TabTransformer on the MI355X hot path. The reference's models/ranking/tabtransformer.py is an empty file (deviation
D-rankers-empty); the model is Huang et al. 2020 with the reference's own block: a stack of
network_layers.TransformerEncoder over the fields, flattened into create_mlp (backend/blocks/mlp.py:4-15) and a Dense(1)
head: logit = Dense(1)(MLP(flatten(stack(x as [B, S, 2D])))). The reference's backend/blocks/transformer.py builder,
which uses Keras' own MultiHeadAttention, stays out of scope (deviation D-tabtransformer-block).

Here: ONE fused encoder (runtime.train.embed); train_transformer_encoder_stack (rf_tfenc_fwd / rf_tfenc_bwd) reads the
embed output in place as [B, S, 2D]; TrainTower and TrainLinear(1) follow. Sigmoid cross-entropy plus
l2_reg * the blocks' five kernels squared. The kernel has no dropout: `dropout` is the tower's.
"""
from __future__ import annotations

import torch

from .ranker_base import TrainableRanker


class TrainableTabTransformer(TrainableRanker):
    def __init__(self, encoder, n_blocks: int = 2, num_heads: int = 1, ffn_hidden_unit: int = 128, hidden_units=(256, 128),
                 dropout: float = 0.3, l2_reg: float = 0., layer_norm_eps: float = 1e-6, learning_rate: float = 1e-3,
                 seed: int = 0, lazy_adam: bool = False, deferred_adam=None):
        super().__init__(encoder)
        from ...backend.blocks.train_mlp import TrainLinear, TrainTower
        from ...backend.layers.network_layers import TrainTransformerEncoder
        from ...runtime import lib as L

        n_blocks, num_heads, ffn_hidden_unit = int(n_blocks), int(num_heads), int(ffn_hidden_unit)
        if self.width % 16:
            raise ValueError(f"TrainableTabTransformer: encoder.dim ({encoder.dim}): the field width 2 * dim = {self.width} "
                             "must be a multiple of 16")
        if num_heads < 1 or self.width % num_heads or (self.width // num_heads) % 16:
            raise ValueError(f"TrainableTabTransformer: num_heads ({num_heads}) must divide the field width {self.width} "
                             "with a depth that is a multiple of 16")
        lib = L.load()
        if int(lib.rf_tfenc_bwd_ws_bytes(1, self.n_slots, self.width, num_heads, ffn_hidden_unit, n_blocks)) == 0:
            msg = lib.rf_last_error().decode(errors="replace")
            raise ValueError(f"TrainableTabTransformer: n_blocks / ffn_hidden_unit / the encoder's slots: {msg}")
        g = torch.Generator().manual_seed(seed)
        dev = encoder.table.device
        self.tower = TrainTower(int(encoder.out_width), list(hidden_units), rate=dropout, eps=1e-6, seed=64 * seed + 1,
                                generator=g, device=dev)
        self.blocks = torch.nn.ModuleList(
            TrainTransformerEncoder(self.width, num_heads=num_heads, ffn_hidden_unit=ffn_hidden_unit, dropout=0.,
                                    layer_norm_eps=layer_norm_eps, l2_reg=l2_reg, seed=64 * seed + 8 * i + 2, device=dev)
            for i in range(n_blocks))
        self.head = TrainLinear(self.tower.out_features, 1, generator=g, device=dev)
        self._init_optimizers(learning_rate, lazy_adam, deferred_adam)

    def _logits(self, x: torch.Tensor, mask=None) -> torch.Tensor:
        from ...backend.layers.network_layers import train_transformer_encoder_stack

        B = x.shape[0]
        h = train_transformer_encoder_stack(list(self.blocks), x.view(B, self.n_slots, self.width), mask)
        return self.head(self.tower(h.reshape(B, self.n_slots * self.width))).reshape(B)

    def regularization(self):
        return sum(blk.regularization() for blk in self.blocks)
