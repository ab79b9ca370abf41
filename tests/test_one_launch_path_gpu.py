"""The inference layer and its training twin launch rf_cross_fwd / rf_cin_fwd / rf_tfenc_fwd through the same function:
from the same seed, the inference layer, the training layer in eval() under no_grad and the training layer in train()
with grad enabled give the same bits."""
import pytest
import torch

from recommendflow_amd.backend.layers import network_layers as N

pytestmark = pytest.mark.gpu


def _three(infer, train, call):
    """call(layer) on the inference layer, on the training layer in eval() without grad, and in train() with grad."""
    with torch.no_grad():
        a = call(infer)
        train.eval()
        b = call(train)
    train.train()
    with torch.enable_grad():
        c = call(train)
    assert c.requires_grad
    return a, b, c.detach()


def test_cross(cuda):
    B, dim, layers = 5, 33, 2
    x = torch.randn(B, dim, generator=torch.Generator().manual_seed(1)).to(cuda)
    a, b, c = _three(N.CrossNetwork(layers, seed=3), N.TrainCrossNetwork(layers, seed=3), lambda layer: layer(x))
    assert a.shape == (B, dim) and torch.equal(a, b) and torch.equal(a, c)


def test_cin(cuda):
    B, fields, dim, sizes = 3, 5, 10, [6, 4]  # the smallest two-layer shape of tests/cin_train_ref.py SHAPES
    x = torch.randn(B, fields, dim, generator=torch.Generator().manual_seed(2)).to(cuda)
    a, b, c = _three(N.CIN(sizes, seed=4), N.TrainCIN(sizes, seed=4), lambda layer: layer(x))
    assert a.shape == (B, sum(sizes)) and torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.parametrize("into_view", [False, True], ids=["new", "out_view"])
def test_transformer_encoder(cuda, into_view):
    B, Ln, d, heads, ffn = 2, 3, 16, 1, 16
    x = torch.randn(B, Ln, d, generator=torch.Generator().manual_seed(5)).to(cuda)
    mask = torch.ones(B, Ln, device=cuda)
    mask[0, 1] = 0.0  # one masked query row
    infer = [N.TransformerEncoder(d, num_heads=heads, ffn_hidden_unit=ffn, seed=10 * i + 6) for i in range(2)]
    train = [N.TrainTransformerEncoder(d, num_heads=heads, ffn_hidden_unit=ffn, seed=10 * i + 6) for i in range(2)]
    outs = []
    for blocks, stack, training, grad in ((infer, N.transformer_encoder_stack, False, False),
                                          (train, N.train_transformer_encoder_stack, False, False),
                                          (train, N.train_transformer_encoder_stack, True, True)):
        for blk in blocks:
            blk.train(training)
        wide = torch.full((B, Ln, d + 8), -3.0, device=cuda)
        with torch.set_grad_enabled(grad):
            y = stack(blocks, x, mask, out=wide[:, :, 4: 4 + d] if into_view else None)
        assert y.requires_grad == grad
        if into_view:
            assert y.data_ptr() == wide[:, :, 4: 4 + d].data_ptr() and y.stride() == wide[:, :, 4: 4 + d].stride()
            assert bool((wide[:, :, :4] == -3.0).all()) and bool((wide[:, :, 4 + d:] == -3.0).all())
        outs.append(y.detach())
    assert outs[0].shape == (B, Ln, d) and bool(torch.isfinite(outs[0]).all())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
