"""What the trainable rankers over the fused encoder (DeepFM, DCN) share, shaped like TrainableQue2Search: ONE fused
encoder through runtime.train.embed, SparseAdam on the table (deferred per row by default), KerasAdam on everything
dense, step() = forward, sigmoid cross-entropy plus the layers' l2 penalties, backward, both optimizers."""
from __future__ import annotations

import torch

from ...runtime.batch import SparseBatch
from ..matching.dssm import SparseTableState


class TrainableRanker(SparseTableState, torch.nn.Module):
    """Subclasses create their dense modules (self.tower is the TrainTower whose dropout step counter a checkpoint
    carries), then call _init_optimizers(); they implement _logits(x, **inputs) -> [B] and regularization()."""

    def __init__(self, encoder):
        super().__init__()
        self.enc = encoder
        self.width = 2 * int(encoder.dim)
        self.n_slots = int(encoder.out_width) // self.width

    def _init_optimizers(self, learning_rate: float, lazy_adam: bool, deferred_adam):
        from ...backend.optim import KerasAdam, SparseAdam

        if deferred_adam is None:
            deferred_adam = not lazy_adam
        self.sparse_opt = SparseAdam(self.enc.table, learning_rate=learning_rate, lazy=lazy_adam, deferred=deferred_adam)
        self.dense_opt = KerasAdam(list(self.parameters()), learning_rate=learning_rate)

    # ---- checkpoint: the mixin's table / m / v / step count, plus the dense optimizer and the dropout step counter
    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        for i, (m, v) in enumerate(zip(self.dense_opt.m, self.dense_opt.v)):
            destination[f"{prefix}dense_m.{i}"] = m
            destination[f"{prefix}dense_v.{i}"] = v
        destination[prefix + "dense_iterations"] = torch.tensor(self.dense_opt.iterations, dtype=torch.int64)
        destination[prefix + "tower_steps"] = torch.tensor([self.tower.steps], dtype=torch.int64)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        n = len(self.dense_opt.m)
        keys = [f"{prefix}dense_{k}.{i}" for i in range(n) for k in ("m", "v")]
        keys += [prefix + "dense_iterations", prefix + "tower_steps"]
        present = [k in state_dict for k in keys]
        if all(present):
            for i in range(n):
                self.dense_opt.m[i].copy_(state_dict[f"{prefix}dense_m.{i}"])
                self.dense_opt.v[i].copy_(state_dict[f"{prefix}dense_v.{i}"])
            self.dense_opt.iterations = int(state_dict[prefix + "dense_iterations"])
            self.tower.steps = int(state_dict[prefix + "tower_steps"][0])
        elif strict:
            missing_keys.extend(k for k, p in zip(keys, present) if not p)
        drop = set(keys)
        rest = {k: v for k, v in state_dict.items() if k not in drop}
        super()._load_from_state_dict(rest, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    # ---- forward
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

    def step(self, batch: SparseBatch, labels: torch.Tensor, dp=None, **inputs) -> torch.Tensor:
        """One training step on one replica; returns the loss."""
        if dp is not None:
            raise NotImplementedError(f"{type(self).__name__}.step: data-parallel replicas are not implemented")
        self.train()
        self.dense_opt.zero_grad(set_to_none=True)
        if self.sparse_opt.deferred:
            # the batch's rows current before the forward reads them; the backward's reduce reuses the plan
            plan = self.enc.backward_plan(batch)
            self.sparse_opt.prepare(plan.rows, plan.n_uniq, plan.cap)
            self.enc._plan, self.enc._plan_batch, self.enc._plan_stream = plan, batch, None
        loss = self.loss(labels, self(batch, **inputs))
        loss.backward()
        self.sparse_opt.apply(self.enc.grad)
        self.dense_opt.step()
        return loss.detach()
