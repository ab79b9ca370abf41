"""GPU: TrainableXDeepFM (6 slots, D 8, a 3600-row table, hidden units 32 -> 16, cin_size (8, 4), l2_reg 0.01) against
the float64 restatement (tests/cin_train_ref.py) composed from the model's own parameters and the GPU's own embed
output. Tolerance per tensor: max(4 x err(restatement with CinEmu, float64), 8 x err(float32 restatement, float64),
2^-20): the CIN rounds its MFMA operands to bf16 where CinEmu does, everything else is fp32 as in the other rankers."""
import numpy as np
import pytest
import torch

import cin_train_ref as C
import interact_train_ref as T
from model_helpers import state_layout
from recommendflow_amd.backend.encoder.sparse_encoder import FusedSparseEncoder, SlotSpec
from recommendflow_amd.models.ranking import TrainableXDeepFM
from recommendflow_amd.runtime.batch import synthetic_batch

pytestmark = pytest.mark.gpu

S, D, HIDDEN, CIN_SIZE = 6, 8, (32, 16), (8, 4)


def _model(dropout=0.0, seed=1, enc_seed=4, lr=0.01):
    specs = [SlotSpec(f"f{s}", 600, (2022, 2023), ["sum", "avg"][s % 2]) for s in range(S)]
    enc = FusedSparseEncoder(specs, D, seed=enc_seed)
    return TrainableXDeepFM(enc, cin_size=CIN_SIZE, hidden_units=HIDDEN, dropout=dropout, l2_reg=0.01, learning_rate=lr,
                            seed=seed)


def _batch(B, seed=3):
    return synthetic_batch(B, [s % 2 == 1 for s in range(S)], seed=seed, id_max=400, uniform=True).to("cuda")


def _labels(B):
    return (torch.arange(B, device="cuda") % 2).float()


def _check(name, got, want64, want32, emu):
    err = T.rel_err(got, want64)
    e_emu, e_32 = T.rel_err(emu, want64), T.rel_err(want32, want64)
    bar = max(4.0 * e_emu, 8.0 * e_32, T.FLOOR)
    print(f"{name}: err {err:.3e} bar {bar:.3e} (CinEmu restatement err {e_emu:.3e}, float32 CPU err {e_32:.3e})")
    assert bool(torch.isfinite(got).all()) and err <= bar, (name, err, bar)


def _restated_step(model, x, y, dtype, cin):
    P = T.model_params(model, dtype)
    xr = x.detach().to(dtype).clone().requires_grad_(True)  # a leaf of its own: x.to(float32) would be x itself
    lv = C.xdeepfm_loss(model, P, xr, y.cpu().to(dtype), cin)
    lv.backward()
    return lv.detach(), {n: p.grad for n, p in P.items()}, xr.grad


@pytest.mark.parametrize("B", [64, 63])
def test_training_step_against_float64(cuda, B):
    """dropout = 0: the loss, every dense parameter's gradient and the gradient reaching the embed output."""
    model = _model()
    hb, y = _batch(B), _labels(B)
    x = model.enc(hb).detach().cpu()
    seen = {}
    model.train()
    logits = model(hb, embed_hook=lambda gr: seen.setdefault("g", gr.detach().clone()))
    assert logits.shape == (B,)
    lv = model.loss(y, logits)
    lv.backward()
    torch.cuda.synchronize()
    assert model.enc.grad is not None and model.enc.grad.count() > 0
    l64, g64, dx64 = _restated_step(model, x, y, torch.float64, C.R.cin_einsum)
    l32, g32, dx32 = _restated_step(model, x, y, torch.float32, C.R.cin_einsum)
    lem, gem, dxem = _restated_step(model, x, y, torch.float64, C.cin_emu)
    _check(f"xdeepfm loss B{B}", lv.detach().reshape(1), l64.reshape(1), l32.reshape(1), lem.reshape(1))
    named = dict(model.named_parameters())
    assert set(named) == set(g64)
    assert {"cin.cin_W.CIN_W_0", "cin.cin_W.CIN_W_1", "head.W", "head.b"} <= set(named)
    assert named["cin.cin_W.CIN_W_0"].shape == (1, S * S, 8) and named["cin.cin_W.CIN_W_1"].shape == (1, S * 8, 4)
    assert named["head.W"].shape == (1, 12 + 16)
    for n, p in named.items():
        assert p.grad is not None and p.grad.shape == p.shape, n
        _check(f"xdeepfm grad {n} B{B}", p.grad, g64[n], g32[n], gem[n])
    assert seen["g"].shape == (B, S * 2 * D)
    _check(f"xdeepfm grad embed output B{B}", seen["g"], dx64, dx32, dxem)


def test_eval_forward(cuda):
    model = _model(dropout=0.3)
    hb = _batch(64)
    model.step(hb, _labels(64))  # moving statistics and parameters away from their initial values
    model.eval()
    out = model(hb)
    assert out.shape == (64,) and not out.requires_grad
    assert torch.equal(out, model(hb)), "the eval forward is not deterministic (dropout left on?)"
    x = model.enc(hb).detach().cpu()
    with torch.no_grad():
        P64, P32 = T.model_params(model, torch.float64), T.model_params(model, torch.float32)
        r64 = torch.sigmoid(C.xdeepfm(model, P64, x.double(), training=False))
        r32 = torch.sigmoid(C.xdeepfm(model, P32, x.float(), training=False))
        rem = torch.sigmoid(C.xdeepfm(model, P64, x.double(), training=False, cin=C.cin_emu))
    _check("xdeepfm eval", out, r64, r32, rem)


def _run_steps(n, seed):
    model = _model(dropout=0.3, seed=seed)
    hb, y = _batch(64, seed=8), _labels(64)
    plan = model.enc.backward_plan(hb)
    rows = plan.rows[: int(plan.n_uniq)].long().clone()
    t0 = model.embedding_table().clone()
    losses = [model.step(hb, y).cpu().numpy().view(np.uint32).item() for _ in range(n)]
    return model, losses, rows, t0


def test_thirty_steps(cuda):
    model, bits, rows, t0 = _run_steps(30, 3)
    losses = np.array(bits, np.uint32).view(np.float32)
    print("xdeepfm losses", losses.tolist())
    assert np.isfinite(losses).all()
    assert losses[-1] < losses[0]
    t1 = model.embedding_table()
    assert rows.numel() > 0 and bool((t1[rows] != t0[rows]).any(dim=1).all()), "a touched table row did not move"
    assert model.sparse_opt.iterations == 30 and model.dense_opt.iterations == 30
    _, bits2, _, _ = _run_steps(30, 3)
    assert bits == bits2, "equal seeds gave different runs"


def test_checkpoint_round_trip(cuda):
    hb, y = _batch(64, seed=8), _labels(64)
    a = _model(dropout=0.3, seed=3)
    for _ in range(3):
        a.step(hb, y)
    sd = {k: v.detach().clone() for k, v in a.state_dict().items()}
    assert any(k.startswith("dense_m.") for k in sd) and "sparse_m" in sd
    b = _model(dropout=0.3, seed=3, enc_seed=9)  # another table: everything must come from the checkpoint
    assert not torch.equal(a.enc.table, b.enc.table)
    b.load_state_dict(sd)
    la, lb = a.step(hb, y), b.step(hb, y)
    assert la.cpu().numpy().view(np.uint32).item() == lb.cpu().numpy().view(np.uint32).item()
    assert torch.equal(a.embedding_table(), b.embedding_table())
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.equal(p, q)


def test_step_refuses_data_parallel(cuda):
    with pytest.raises(NotImplementedError):
        _model().step(_batch(8), _labels(8), dp=object())


# state_layout() of the tiny model below, written out: a checkpoint written today must still load tomorrow
STATE_LAYOUT = [
    ('cin.cin_W.CIN_W_0', (1, 16, 8), 'float32'), ('cin.cin_W.CIN_W_1', (1, 32, 4), 'float32'),
    ('dense_iterations', (), 'int64'),
    ('dense_m.0', (8, 32), 'float32'), ('dense_m.1', (4, 8), 'float32'), ('dense_m.10', (1, 16), 'float32'),
    ('dense_m.11', (1,), 'float32'), ('dense_m.2', (8,), 'float32'), ('dense_m.3', (4,), 'float32'),
    ('dense_m.4', (32,), 'float32'), ('dense_m.5', (8,), 'float32'), ('dense_m.6', (32,), 'float32'),
    ('dense_m.7', (8,), 'float32'), ('dense_m.8', (1, 16, 8), 'float32'), ('dense_m.9', (1, 32, 4), 'float32'),
    ('dense_v.0', (8, 32), 'float32'), ('dense_v.1', (4, 8), 'float32'), ('dense_v.10', (1, 16), 'float32'),
    ('dense_v.11', (1,), 'float32'), ('dense_v.2', (8,), 'float32'), ('dense_v.3', (4,), 'float32'),
    ('dense_v.4', (32,), 'float32'), ('dense_v.5', (8,), 'float32'), ('dense_v.6', (32,), 'float32'),
    ('dense_v.7', (8,), 'float32'), ('dense_v.8', (1, 16, 8), 'float32'), ('dense_v.9', (1, 32, 4), 'float32'),
    ('head.W', (1, 16), 'float32'), ('head.b', (1,), 'float32'), ('sparse_iterations', (), 'int64'),
    ('sparse_m', (2400, 4), 'float32'), ('sparse_table', (2400, 4), 'float32'),
    ('sparse_v', (2400, 4), 'float32'), ('tower.W.0', (8, 32), 'float32'), ('tower.W.1', (4, 8), 'float32'),
    ('tower.b.0', (8,), 'float32'), ('tower.b.1', (4,), 'float32'), ('tower.beta.0', (32,), 'float32'),
    ('tower.beta.1', (8,), 'float32'), ('tower.gamma.0', (32,), 'float32'), ('tower.gamma.1', (8,), 'float32'),
    ('tower.moving_mean_0', (32,), 'float32'), ('tower.moving_mean_1', (8,), 'float32'),
    ('tower.moving_var_0', (32,), 'float32'), ('tower.moving_var_1', (8,), 'float32'),
    ('tower_steps', (1,), 'int64'),
]


def test_state_dict_layout(cuda):
    """The checkpoint format: every state_dict() key with its shape and dtype (4 slots x 300 bins, D 4, hidden units
    8 -> 4, cin_size (8, 4)): dense_m / dense_v numbered in list(model.parameters()) order (tower, cin, head)."""
    specs = [SlotSpec(f"f{s}", 300, (2022, 2023), ["sum", "avg"][s % 2]) for s in range(4)]
    enc = FusedSparseEncoder(specs, 4, seed=4)
    model = TrainableXDeepFM(enc, cin_size=(8, 4), hidden_units=(8, 4), dropout=0.3, l2_reg=0.01, learning_rate=0.01,
                             seed=3)
    assert state_layout(model) == STATE_LAYOUT
