"""What the models trained over a fused table share (TrainableDssm, TrainableQue2Search, TrainableDeepFM,
TrainableDCN): self.enc is the FusedSparseEncoder, self.sparse_opt the SparseAdam on its table (deferred per row by
default), self.dense_opt the KerasAdam on everything dense.

SparseTableState      the table made current, the two optimizers, the rows staged for deferred Adam, and a state_dict
                      that carries the table with its optimizer's m, v and step count.
TableTrainedModel     on top of it, for the single-replica models: the dense optimizer's moments and the towers'
                      dropout step counters in the checkpoint, and step().
"""
from __future__ import annotations

import torch

from ..runtime.batch import SparseBatch


class SparseTableState:
    def _init_optimizers(self, learning_rate: float, lazy_adam: bool, deferred_adam, dense_params=None):
        """SparseAdam on the table and KerasAdam on dense_params (default: every parameter of the module; the order
        fixes the dense_m.{i} / dense_v.{i} checkpoint keys). deferred_adam None = not lazy_adam."""
        from ..backend.optim import KerasAdam, SparseAdam

        if deferred_adam is None:
            deferred_adam = not lazy_adam
        if dense_params is None:
            dense_params = list(self.parameters())
        self.sparse_opt = SparseAdam(self.enc.table, learning_rate=learning_rate, lazy=lazy_adam, deferred=deferred_adam)
        self.dense_opt = KerasAdam(dense_params, learning_rate=learning_rate)

    def _stage_rows(self, batch: SparseBatch):
        """Deferred Adam: the batch's rows current before the forward reads them; the backward's reduce reuses the
        plan."""
        if self.sparse_opt.deferred:
            plan = self.enc.backward_plan(batch)
            self.sparse_opt.prepare(plan.rows, plan.n_uniq, plan.cap)
            self.enc.stage_plan(plan, batch)

    def materialize(self):
        """Bring every table row current (deferred Adam) before anything outside step() reads the table."""
        self.sparse_opt.materialize()

    def embedding_table(self) -> torch.Tensor:
        """The fused table with every row current: the accessor for readers outside step() / the eval forward
        (export, search index builds). enc.table itself may hold rows behind by deferred steps."""
        self.materialize()
        return self.enc.table

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        # the fused table is a plain attribute of the encoder, not a parameter: a checkpoint gets it here, with the
        # table optimizer's m, v and step count, every row current (the dense step's values bit for bit)
        super()._save_to_state_dict(destination, prefix, keep_vars)
        st = self.sparse_opt.state()
        for k in ("table", "m", "v"):
            t = st[k]
            destination[prefix + "sparse_" + k] = t if keep_vars else t.detach()
        destination[prefix + "sparse_iterations"] = torch.tensor(st["iterations"], dtype=torch.int64)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        keys = [prefix + "sparse_" + k for k in ("table", "m", "v", "iterations")]
        present = [k in state_dict for k in keys]
        if all(present):
            t, m, v, it = (state_dict[k] for k in keys)
            # rows loaded are current through the checkpoint's step: the deferred replay starts from there
            self.sparse_opt.load_state(t, m, v, int(it))
        elif strict:
            missing_keys.extend(k for k, p in zip(keys, present) if not p)
        rest = {k: v for k, v in state_dict.items() if k not in keys}
        super()._load_from_state_dict(rest, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)


class TableTrainedModel(SparseTableState, torch.nn.Module):
    """Subclasses create their dense modules, call _init_optimizers(), and implement forward, train_towers() (the
    TrainTowers whose dropout step counters a checkpoint carries) and batch_loss()."""

    def train_towers(self):
        raise NotImplementedError

    def batch_loss(self, batch: SparseBatch, labels: torch.Tensor, **inputs) -> torch.Tensor:
        raise NotImplementedError

    # ---- checkpoint: the table / m / v / step count above, plus the dense optimizer and the dropout step counters
    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        for i, (m, v) in enumerate(zip(self.dense_opt.m, self.dense_opt.v)):
            destination[f"{prefix}dense_m.{i}"] = m
            destination[f"{prefix}dense_v.{i}"] = v
        destination[prefix + "dense_iterations"] = torch.tensor(self.dense_opt.iterations, dtype=torch.int64)
        destination[prefix + "tower_steps"] = torch.tensor([t.steps for t in self.train_towers()], dtype=torch.int64)

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
            for t, s in zip(self.train_towers(), state_dict[prefix + "tower_steps"].tolist()):
                t.steps = int(s)
        elif strict:
            missing_keys.extend(k for k, p in zip(keys, present) if not p)
        drop = set(keys)
        rest = {k: v for k, v in state_dict.items() if k not in drop}
        super()._load_from_state_dict(rest, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def step(self, batch: SparseBatch, labels: torch.Tensor, dp=None, **inputs) -> torch.Tensor:
        """One training step on one replica; returns the loss."""
        if dp is not None:
            raise NotImplementedError(f"{type(self).__name__}.step: data-parallel replicas are not implemented")
        self.train()
        self.dense_opt.zero_grad(set_to_none=True)
        self._stage_rows(batch)
        loss = self.batch_loss(batch, labels, **inputs)
        loss.backward()
        self.sparse_opt.apply(self.enc.grad)
        self.dense_opt.step()
        return loss.detach()
