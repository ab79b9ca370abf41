"""GPU: a DSSM training step on the fused encoder — the sparse gradient autograd hands back equals the
C oracle's for the dout torch computed, and the loss falls when overfitting one batch."""
import numpy as np
import pytest
import torch

from model_helpers import state_layout
from recommendflow_amd.backend.encoder.sparse_encoder import FusedSparseEncoder, SlotSpec
from recommendflow_amd.models.matching.dssm import TrainableDssm
from recommendflow_amd.runtime.batch import synthetic_batch
from recommendflow_amd.runtime.train import embed

pytestmark = pytest.mark.gpu


def _model(loss="cosent", lazy=False, deferred=None):
    S = 16
    specs = [SlotSpec(f"f{s}", 500, (2022, 2023), ["sum", "avg"][s % 2]) for s in range(S)]
    enc = FusedSparseEncoder(specs, 16, seed=4)
    return TrainableDssm(enc, 6, units=(64, 32), dropout=0.0, learning_rate=0.01, loss=loss, lazy_adam=lazy, seed=1,
                         deferred_adam=deferred), S


def test_sparse_grad_through_autograd_matches_oracle(O, cuda):
    model, S = _model()
    hb = synthetic_batch(128, [s % 4 == 0 for s in range(S)], seed=3, id_max=300)
    dev = hb.to("cuda")
    seen = {}
    x = embed(model.enc, dev)
    x.register_hook(lambda g: seen.setdefault("dout", g.detach().clone()))
    u = torch.nn.functional.normalize(model.user_tower(x[:, : model.wu]), dim=-1)
    v = torch.nn.functional.normalize(model.ad_tower(x[:, model.wu:]), dim=-1)
    y = torch.randint(0, 2, (128,), device="cuda").float()
    model.loss_fn(y, u, v).backward()
    g = model.enc.grad
    n = g.count()
    wr, wg = O.fused_hash_embed_bwd(model.enc.host_desc, hb.tok_bytes, hb.tok_off, hb.bag_off, hb.lmax, 128,
                                    model.enc.table.cpu().numpy(), 16, x.detach().cpu().numpy(),
                                    seen["dout"].cpu().numpy())
    np.testing.assert_array_equal(g.rows[:n].cpu().numpy(), wr)
    assert np.array_equal(g.grad[:n].cpu().numpy().view(np.uint32), wg.view(np.uint32))


@pytest.mark.parametrize("loss,lazy", [("cosent", False), ("inbatch_ce", True)])
def test_loss_decreases(cuda, loss, lazy):
    torch.manual_seed(0)
    model, S = _model(loss, lazy)
    hb = synthetic_batch(256, [s % 4 == 0 for s in range(S)], seed=5, id_max=2000).to("cuda")
    y = (torch.arange(256, device="cuda") % 2).float() if loss == "cosent" else torch.ones(256, device="cuda")
    t0 = model.enc.table.clone()
    losses = [float(model.step(hb, y)) for _ in range(30)]
    assert min(losses[-5:]) < losses[0] * 0.8, losses
    assert not torch.equal(t0, model.enc.table)  # the table trained
    assert model.sparse_opt.iterations == 30


def test_data_parallel_world1_matches_single(cuda):
    """runtime.dist.DataParallel over RCCL with one rank: the bucketed all-reduce, the sparse all-gather and
    the rank-ordered segment sum are identities, so three steps give bit-identical tables and towers."""
    import socket

    import torch.distributed as dist

    from recommendflow_amd.runtime.dist import DataParallel

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        dp = DataParallel(bucket_bytes=1 << 16)
        S = 16
        hb = synthetic_batch(128, [s % 4 == 0 for s in range(S)], seed=9, id_max=400).to("cuda")
        y = (torch.arange(128, device="cuda") % 2).float()
        models = [_model()[0] for _ in range(2)]
        for _ in range(3):
            models[0].step(hb, y)
            models[1].step(hb, y, dp=dp)
        torch.cuda.synchronize()
        assert torch.equal(models[0].enc.table, models[1].enc.table)
        for a, b in zip(models[0].parameters(), models[1].parameters()):
            assert torch.equal(a, b)
    finally:
        dist.destroy_process_group()


def test_backward_plan_reduce_equals_backward(cuda):
    """rf_fused_hash_embed_bwd_plan + _reduce (the halves the train step splits across streams) give the
    one-call backward's rows and gradient bit for bit."""
    S = 12
    specs = [SlotSpec(f"f{s}", 700, (2022, 2023), ["sum", "avg", "max"][s % 3]) for s in range(S)]
    enc = FusedSparseEncoder(specs, 16, seed=6)
    b = synthetic_batch(200, [s % 3 == 0 for s in range(S)], seed=12, id_max=500).to("cuda")
    out = enc(b)
    dout = torch.randn(out.shape, generator=torch.Generator().manual_seed(2)).cuda()
    g1 = enc.backward(b, dout, out=out)
    plan = enc.backward_plan(b)
    g2 = enc.backward_reduce(plan, dout, out=out)
    n = g1.count()
    assert g2.count() == n
    assert torch.equal(g1.rows[:n], g2.rows[:n])
    assert torch.equal(g1.grad[:n], g2.grad[:n])


def test_overlapped_table_adam_equals_dense(cuda):
    """TrainableDssm.step with the table's dense Adam split (untouched rows on a side stream during the towers,
    the gradient's rows after the backward) against the one-launch dense Adam: three steps, bit-identical
    tables, Adam moments and towers."""
    S = 16
    hb = synthetic_batch(128, [s % 4 == 0 for s in range(S)], seed=21, id_max=400).to("cuda")
    y = (torch.arange(128, device="cuda") % 2).float()
    models = [_model(deferred=False)[0] for _ in range(2)]
    models[1].overlap_table_adam = False
    for _ in range(3):
        for m in models:
            m.step(hb, y)
    torch.cuda.synchronize()
    a, b = models
    assert torch.equal(a.enc.table, b.enc.table)
    assert torch.equal(a.sparse_opt.m, b.sparse_opt.m) and torch.equal(a.sparse_opt.v, b.sparse_opt.v)
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.equal(p, q)


def test_deferred_table_adam_equals_dense(cuda):
    """TrainableDssm's default table Adam (SparseAdam(deferred=True): a row's missed untouched steps are replayed
    when the row is next read) against the split and the one-launch dense Adam, over batches whose row sets differ
    (rows skip one or two steps, then are read again): bit-identical losses at every step, and after materialize()
    bit-identical tables, Adam moments and towers."""
    S = 16
    hbs = [synthetic_batch(128, [s % 4 == 0 for s in range(S)], seed=40 + i, id_max=300 + 200 * i).to("cuda")
           for i in range(3)]
    y = (torch.arange(128, device="cuda") % 2).float()
    models = [_model(deferred=d)[0] for d in (False, False, True)]
    models[1].overlap_table_adam = False
    assert models[2].sparse_opt.deferred and not models[0].sparse_opt.deferred
    losses = [[], [], []]
    for k in (0, 1, 2, 0, 2, 1):
        for i, m in enumerate(models):
            losses[i].append(m.step(hbs[k], y).cpu().numpy().view(np.uint32).item())
    assert losses[0] == losses[1] == losses[2], losses
    last = models[2].sparse_opt.last
    assert int((last < models[2].sparse_opt.iterations).sum()) > 0  # some rows are still behind before materialize
    models[2].materialize()
    torch.cuda.synchronize()
    for a in models[:2]:
        b = models[2]
        assert torch.equal(a.enc.table, b.enc.table)
        assert torch.equal(a.sparse_opt.m, b.sparse_opt.m) and torch.equal(a.sparse_opt.v, b.sparse_opt.v)
        for p, q in zip(a.parameters(), b.parameters()):
            assert torch.equal(p, q)


def test_deferred_adam_eval_forward_reads_current_rows(cuda):
    """After deferred-Adam training steps, the eval-mode forward (which materializes first) returns the dense
    model's scores bit for bit, and state_dict() holds the dense step's table."""
    S = 16
    hbs = [synthetic_batch(128, [s % 4 == 0 for s in range(S)], seed=60 + i, id_max=300 + 250 * i).to("cuda")
           for i in range(2)]
    y = (torch.arange(128, device="cuda") % 2).float()
    dense, defer = _model(deferred=False)[0], _model(deferred=True)[0]
    for k in (0, 1, 0):
        dense.step(hbs[k], y)
        defer.step(hbs[k], y)
    dense.eval()
    defer.eval()
    with torch.no_grad():
        for hb in hbs:
            ud, vd = dense(hb)
            uf, vf = defer(hb)
            assert torch.equal(ud, uf) and torch.equal(vd, vf)
    assert torch.equal(dense.enc.table, defer.enc.table)
    assert int(defer.sparse_opt.last.min()) == defer.sparse_opt.iterations


def test_deferred_adam_checkpoint_round_trip(cuda):
    """state_dict() of a deferred-Adam model carries the fused table, m, v and the step count with every
    row current (the dense model's values bit for bit), and load_state_dict() into a model with different table
    contents resets the deferred bookkeeping, so training continues exactly as the dense model does (no missed step
    is replayed onto the loaded rows)."""
    S = 16
    hbs = [synthetic_batch(128, [s % 4 == 0 for s in range(S)], seed=80 + i, id_max=300 + 250 * i).to("cuda")
           for i in range(2)]
    y = (torch.arange(128, device="cuda") % 2).float()
    dense, defer = _model(deferred=False)[0], _model(deferred=True)[0]
    for k in (0, 1, 0):
        dense.step(hbs[k], y)
        defer.step(hbs[k], y)
    sd = defer.state_dict()
    assert torch.equal(sd["sparse_table"], dense.enc.table)
    assert torch.equal(sd["sparse_m"], dense.sparse_opt.m) and torch.equal(sd["sparse_v"], dense.sparse_opt.v)
    assert int(sd["sparse_iterations"]) == 3
    sd = {k: v.clone() for k, v in sd.items()}
    fresh = _model(deferred=True)[0]
    fresh.step(hbs[1], y)  # one step of its own: rows behind by one, iterations 1
    fresh.load_state_dict(sd)
    assert fresh.sparse_opt.iterations == 3 and int(fresh.sparse_opt.last.min()) == 3
    fresh.dense_opt.m = [m.clone() for m in dense.dense_opt.m]
    fresh.dense_opt.v = [v.clone() for v in dense.dense_opt.v]
    fresh.dense_opt.iterations = dense.dense_opt.iterations
    for k in (1, 0):
        ld = dense.step(hbs[k], y)
        lf = fresh.step(hbs[k], y)
        assert torch.equal(ld, lf)
    assert torch.equal(fresh.embedding_table(), dense.enc.table)


# state_layout() of the tiny model below, written out: a checkpoint written today must still load tomorrow
DSSM_STATE_LAYOUT = [
    ('ad_tower.W.0', (8, 16), 'float32'), ('ad_tower.W.1', (4, 8), 'float32'), ('ad_tower.b.0', (8,), 'float32'),
    ('ad_tower.b.1', (4,), 'float32'), ('ad_tower.beta.0', (16,), 'float32'), ('ad_tower.beta.1', (8,), 'float32'),
    ('ad_tower.gamma.0', (16,), 'float32'), ('ad_tower.gamma.1', (8,), 'float32'),
    ('ad_tower.moving_mean_0', (16,), 'float32'), ('ad_tower.moving_mean_1', (8,), 'float32'),
    ('ad_tower.moving_var_0', (16,), 'float32'), ('ad_tower.moving_var_1', (8,), 'float32'),
    ('sparse_iterations', (), 'int64'), ('sparse_m', (2400, 4), 'float32'), ('sparse_table', (2400, 4), 'float32'),
    ('sparse_v', (2400, 4), 'float32'), ('user_tower.W.0', (8, 16), 'float32'), ('user_tower.W.1', (4, 8), 'float32'),
    ('user_tower.b.0', (8,), 'float32'), ('user_tower.b.1', (4,), 'float32'), ('user_tower.beta.0', (16,), 'float32'),
    ('user_tower.beta.1', (8,), 'float32'), ('user_tower.gamma.0', (16,), 'float32'),
    ('user_tower.gamma.1', (8,), 'float32'), ('user_tower.moving_mean_0', (16,), 'float32'),
    ('user_tower.moving_mean_1', (8,), 'float32'), ('user_tower.moving_var_0', (16,), 'float32'),
    ('user_tower.moving_var_1', (8,), 'float32'),
]


def test_state_dict_layout(cuda):
    """The checkpoint format: every state_dict() key with its shape and dtype (4 slots x 300 bins, D 4, 2 user slots,
    towers 8 -> 4). TrainableDssm carries no dense-optimizer moments and no dropout step counters."""
    specs = [SlotSpec(f"f{s}", 300, (2022, 2023), ["sum", "avg"][s % 2]) for s in range(4)]
    model = TrainableDssm(FusedSparseEncoder(specs, 4, seed=4), 2, units=(8, 4), dropout=0.3, learning_rate=0.01, seed=1)
    assert state_layout(model) == DSSM_STATE_LAYOUT
