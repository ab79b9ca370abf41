"""What the trainable rankers over the fused encoder (DeepFM, DCN, xDeepFM) add to models.trainable.TableTrainedModel: ONE fused
encoder through runtime.train.embed, the logits of a batch, sigmoid cross-entropy plus the layers' l2 penalties."""
from __future__ import annotations

import torch

from ...runtime.batch import SparseBatch
from ..trainable import TableTrainedModel


class TrainableRanker(TableTrainedModel):
    """Subclasses create their dense modules (self.tower is the TrainTower whose dropout step counter a checkpoint
    carries), then call _init_optimizers(); they implement _logits(x, **inputs) -> [B] and regularization()."""

    def __init__(self, encoder):
        super().__init__()
        self.enc = encoder
        self.width = 2 * int(encoder.dim)
        self.n_slots = int(encoder.out_width) // self.width

    def train_towers(self):
        return [self.tower]

    def forward(self, batch: SparseBatch, embed_hook=None, **inputs) -> torch.Tensor:
        """Training: the [B] logits (embed_hook: a tensor hook on the embed output, i.e. called with the gradient that
        reaches the encoder's backward). Evaluation: the [B] probabilities sigmoid(logit), the moving statistics
        folded into the tower and no dropout."""
        if self.training:
            from ...runtime.train import embed

            x = embed(self.enc, batch)
            if embed_hook is not None:
                x.register_hook(embed_hook)
            return self._logits(x, **inputs)
        with torch.no_grad():
            self.sparse_opt.materialize()
            return torch.sigmoid(self._logits(self.enc(batch), **inputs))

    def loss(self, labels: torch.Tensor, logits: torch.Tensor) -> torch.Tensor:
        """Keras BinaryCrossentropy(from_logits=True) (the batch mean) plus the layers' l2 penalties."""
        y = labels.to(logits.dtype).reshape(-1)
        ce = torch.nn.functional.binary_cross_entropy_with_logits(logits, y)
        return ce + self.regularization()

    def batch_loss(self, batch: SparseBatch, labels: torch.Tensor, **inputs) -> torch.Tensor:
        return self.loss(labels, self(batch, **inputs))
