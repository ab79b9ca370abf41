"""Que2Search two-tower model on the MI355X hot path (reference: models/matching/que2search.py:12-157).

The reference model is the consumer of DoubleHashingEmbedding: every sparse feature is one *channel*. A channel's
pooled [B, 2D] embedding goes through its own `create_mlp([dim], 0.3, "selu", BatchNormalization(1e-6))`
(que2search.py:48-62); the query channels and the app channels are fused by AttentionFusion (query: is_norm=False,
app: is_norm=True, :41-42), each side passes a linear Dense(dim) (:45-46, :127-128), and the training loss is
loss(y_true, q, a) with y_pred = sum(q * a) (:137-138).

Here: ONE fused encoder over the user slots then the ad slots (runtime.train.embed), every channel tower in one
towers_forward call over the column blocks of the embed output (grouped rf_gemm_f32 launches), TrainAttentionFusion
(rf_attention_fusion_fwd / _bwd), TrainLinear (rf_gemm_f32), the library losses, SparseAdam on the table and
KerasAdam on everything dense.

Deviation D-q2s-bert: the reference also feeds BERT sentence channels (get_query_bert_embedding /
get_app_bert_embedding, :96-112) into the fusions. The BERT encoder is out of scope; only the sparse
channels exist, so the fusions see the sparse channels alone.
"""
from __future__ import annotations

import torch

from ...runtime.batch import SparseBatch
from ..trainable import TableTrainedModel

MAX_CHANNELS = 16  # rf_attention_fusion_fwd / _bwd: 1 <= channels <= 16


class TrainableQue2Search(TableTrainedModel):
    """Training and evaluation graph of Que2Search over the sparse channels. `encoder` holds the user slots first,
    then the ad slots; each slot is one channel. step() = forward, backward, SparseAdam on the table (deferred per
    row by default, as TrainableDssm) and KerasAdam on towers, fusions and embedding denses (Keras defaults)."""

    def __init__(self, encoder, n_user_slots: int, dim: int, dropout: float = 0.3, loss: str = "cosent",
                 learning_rate: float = 1e-3, seed: int = 0, lazy_adam: bool = False, deferred_adam=None):
        super().__init__()
        n_slots = int(encoder.out_width) // (2 * int(encoder.dim))
        self.n_user_slots, self.n_ad_slots, self.dim = int(n_user_slots), n_slots - int(n_user_slots), int(dim)
        for side, n in (("user", self.n_user_slots), ("ad", self.n_ad_slots)):
            if not 1 <= n <= MAX_CHANNELS:
                raise ValueError(f"TrainableQue2Search: the {side} tower has {n} channels, AttentionFusion takes 1..{MAX_CHANNELS}")
        if loss not in ("cosent", "inbatch_ce"):
            raise ValueError(f"TrainableQue2Search: unknown loss {loss!r}")
        from ...backend.blocks.train_mlp import TrainLinear, TrainTower
        from ...backend.layers.fusion_layers import TrainAttentionFusion
        from ...backend.losses import match_losses

        self.enc = encoder
        self.width = 2 * encoder.dim
        g = torch.Generator().manual_seed(seed)
        dev = encoder.table.device
        self.towers = torch.nn.ModuleList(
            TrainTower(self.width, [self.dim], rate=dropout, eps=1e-6, seed=64 * seed + s + 1, generator=g, device=dev)
            for s in range(n_slots))
        self.query_fusion = TrainAttentionFusion(self.dim, self.n_user_slots, is_norm=False, name="query_fusion",
                                                 seed=2 * seed + 1, device=dev)
        self.app_fusion = TrainAttentionFusion(self.dim, self.n_ad_slots, is_norm=True, name="app_fusion",
                                               seed=2 * seed + 2, device=dev)
        self.query_dense = TrainLinear(self.dim, self.dim, generator=g, device=dev)
        self.app_dense = TrainLinear(self.dim, self.dim, generator=g, device=dev)
        self.loss_fn = {"cosent": match_losses.cosent_loss,
                        "inbatch_ce": match_losses.batch_neg_sample_scaled_multi_class_ce_loss}[loss]
        self._init_optimizers(learning_rate, lazy_adam, deferred_adam)

    # ---- forward
    def _heads(self, chans):
        nu = self.n_user_slots
        q = self.query_dense(self.query_fusion(chans[:nu], self.training))
        a = self.app_dense(self.app_fusion(chans[nu:], self.training))
        return q, a

    def forward(self, batch: SparseBatch, embed_hook=None):
        """Training: (q, a), the two [B, dim] embeddings the loss takes (embed_hook: a tensor hook registered on the
        embed output, i.e. called with the gradient that reaches the encoder's backward). Evaluation:
        {"query": q, "app": a} with the moving statistics folded into the towers and no dropout
        (que2search.py:143-146)."""
        w = self.width
        if self.training:
            from ...backend.blocks.train_mlp import towers_forward
            from ...runtime.train import embed

            x = embed(self.enc, batch)
            if embed_hook is not None:
                x.register_hook(embed_hook)
            chans = towers_forward(x, [(t, s * w, w) for s, t in enumerate(self.towers)])
            return self._heads(list(chans))
        with torch.no_grad():
            self.sparse_opt.materialize()
            x = self.enc(batch)
            q, a = self._heads([t(x[:, s * w: (s + 1) * w]) for s, t in enumerate(self.towers)])
        return {"query": q, "app": a}

    def train_towers(self):
        return list(self.towers)

    def batch_loss(self, batch: SparseBatch, labels: torch.Tensor) -> torch.Tensor:
        return self.loss_fn(labels, *self(batch))

    def get_fusion_weights(self):
        """The batch-averaged attention of each side since init_attention() (que2search.py:152-157)."""
        return {"query": self.query_fusion.get_fusion_weights(), "app": self.app_fusion.get_fusion_weights()}
