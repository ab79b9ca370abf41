"""CPU: the float64 ESIM training oracle (oracle.esim_train_loss, esim_pool_bwd, ln_mlp_train_bwd) against central
finite differences of its own forward. This pins the analytic backward the GPU training path is checked against
(tests/test_esim_train_gpu.py): for every parameter group a random direction v, (f(t + h v) - f(t - h v)) / 2h vs
<grad, v>, rtol 1e-6 in float64. The forward follows esim.py:45-53,69-89, attention_layers.py:33-74, mlp.py:4-15;
parity of the forward itself with the reference is unpinned (TensorFlow is not importable).
ln_mlp_train_fwd / _bwd are pinned the same way on their own for each activation TrainLNMLP accepts (gelu, relu, selu,
none), with every pre-activation kept away from relu's and selu's kink at 0."""
import numpy as np
import pytest

from oracle import oracle as O


def _model(rng, B=6, L=5, d=8, n_dense=4, inu=(8, 12), outu=(16, 8)):
    def layers(k, units):
        out = []
        for u in units:
            out.append({"W": rng.normal(0, 0.4, (u, k)), "b": rng.normal(0, 0.1, u), "gamma": 1 + rng.normal(0, 0.1, k),
                        "beta": rng.normal(0, 0.1, k)})
            k = u
        return out

    q = rng.normal(0, 1.0, (B, L, d))
    a = rng.normal(0, 1.0, (B, L, d))
    dense = rng.normal(0, 1.0, (B, n_dense))
    lin = layers(n_dense, inu)
    lout = layers(inu[-1] + 6 * d, outu)
    Wo = rng.normal(0, 0.4, (2, outu[-1]))
    bo = rng.normal(0, 0.1, 2)
    y = rng.integers(0, 2, B)
    return q, a, dense, y, lin, lout, Wo, bo


def _fd(f, x, v, h=1e-6):
    return (f(x + h * v) - f(x - h * v)) / (2 * h)


@pytest.mark.parametrize("rate", [0.0, 0.3])
def test_esim_train_grads_match_finite_differences(rate):
    rng = np.random.default_rng(7)
    q, a, dense, y, lin, lout, Wo, bo = _model(rng)
    seeds = ([11, 12], 13, [14, 15])
    loss, _, g = O.esim_train_loss(q, a, dense, y, lin, lout, Wo, bo, rate=rate, seeds=seeds, grads=True)

    def L(q_=q, a_=a, lin_=lin, lout_=lout, Wo_=Wo, bo_=bo):
        return O.esim_train_loss(q_, a_, dense, y, lin_, lout_, Wo_, bo_, rate=rate, seeds=seeds)[0]

    checks = []
    v = rng.normal(size=q.shape)
    checks.append(("q", _fd(lambda t: L(q_=t), q, v), (g["q"] * v).sum()))
    v = rng.normal(size=a.shape)
    checks.append(("a", _fd(lambda t: L(a_=t), a, v), (g["a"] * v).sum()))
    v = rng.normal(size=Wo.shape)
    checks.append(("W_out", _fd(lambda t: L(Wo_=t), Wo, v), (g["W_out"] * v).sum()))
    v = rng.normal(size=bo.shape)
    checks.append(("b_out", _fd(lambda t: L(bo_=t), bo, v), (g["b_out"] * v).sum()))
    for name, layers, key in (("input", lin, "lin_"), ("output", lout, "lout_")):
        for li, p in enumerate(layers):
            for k in ("W", "b", "gamma", "beta"):
                v = rng.normal(size=p[k].shape)

                def f(t, li=li, k=k, layers=layers, key=key):
                    ls = [dict(x) for x in layers]
                    ls[li][k] = t
                    return L(**{key: ls})

                checks.append((f"{name}[{li}].{k}", _fd(f, p[k], v), (g[name][li][k] * v).sum()))
    for name, fd, an in checks:
        assert abs(fd - an) <= 1e-6 * max(1.0, abs(fd)) + 1e-9, (name, fd, an)
    assert np.isfinite(loss)


def _ln_mlp_case(act, rate, margin=1e-3):
    """A two-layer LayerNorm MLP whose every pre-activation keeps `margin` from 0: relu and selu are not
    differentiable there (selu's slope jumps from scale alpha to scale), and the finite-difference step moves a
    pre-activation by ~1e-5 at most. Redrawn from consecutive seeds until the margin holds (about 9 draws in 10 do)."""
    for seed in range(100, 140):
        rng = np.random.default_rng(seed)
        M, k = 6, 5
        layers = []
        for u in (8, 7):
            layers.append({"W": rng.normal(0, 0.6, (u, k)), "b": rng.normal(0, 0.3, u), "gamma": 1 + rng.normal(0, 0.1, k),
                           "beta": rng.normal(0, 0.1, k)})
            k = u
        x = rng.normal(0, 1.0, (M, 5))
        R = rng.normal(size=(M, k))
        _, cache = O.ln_mlp_train_fwd(x, layers, rate, [21, 22], act=act)
        if min(np.abs(c["pre"]).min() for c in cache) >= margin:
            return rng, x, layers, R
    raise AssertionError("no draw kept the margin")


@pytest.mark.parametrize("rate", [0.0, 0.3])
@pytest.mark.parametrize("act", ["relu", "selu", "none", "gelu"])
def test_ln_mlp_train_grads_match_finite_differences(act, rate):
    """ln_mlp_train_bwd(act=...) against central differences of ln_mlp_train_fwd(act=...) on f = <h, R>: the input
    and every parameter group, the step and the bar of the gelu pin above."""
    rng, x, layers, R = _ln_mlp_case(act, rate)
    seeds = [21, 22]

    def f(x_=x, layers_=layers):
        return (O.ln_mlp_train_fwd(x_, layers_, rate, seeds, act=act)[0] * R).sum()

    h, cache = O.ln_mlp_train_fwd(x, layers, rate, seeds, act=act)
    assert min(np.abs(c["pre"]).min() for c in cache) >= 1e-3
    if act in ("relu", "selu"):
        assert all((c["pre"] < 0).any() and (c["pre"] > 0).any() for c in cache)  # both branches differentiated
    dx, grads = O.ln_mlp_train_bwd(R, layers, cache, rate, act=act)
    v = rng.normal(size=x.shape)
    checks = [("x", _fd(lambda t: f(x_=t), x, v), (dx * v).sum())]
    for li, p in enumerate(layers):
        for k in ("W", "b", "gamma", "beta"):
            v = rng.normal(size=p[k].shape)

            def fp(t, li=li, k=k):
                ls = [dict(q) for q in layers]
                ls[li][k] = t
                return f(layers_=ls)

            checks.append((f"[{li}].{k}", _fd(fp, p[k], v), (grads[li][k] * v).sum()))
    for name, fd, an in checks:
        assert abs(fd - an) <= 1e-6 * max(1.0, abs(fd)) + 1e-9, (act, name, fd, an)


def test_ln_mlp_train_default_activation_is_gelu():
    """act defaults to gelu: the same bits with and without the argument, so no earlier caller changes."""
    rng, x, layers, R = _ln_mlp_case("gelu", 0.3)
    h0, c0 = O.ln_mlp_train_fwd(x, layers, 0.3, [21, 22])
    h1, c1 = O.ln_mlp_train_fwd(x, layers, 0.3, [21, 22], act="gelu")
    assert np.array_equal(h0, h1) and np.array_equal(h0, np.where(c0[1]["keep"], O.gelu(c0[1]["pre"]) / 0.7, 0.0))
    d0, g0 = O.ln_mlp_train_bwd(R, layers, c0, 0.3)
    d1, g1 = O.ln_mlp_train_bwd(R, layers, c1, 0.3, act="gelu")
    assert np.array_equal(d0, d1) and all(np.array_equal(g0[i][k], g1[i][k]) for i in range(2) for k in g0[i])
    with pytest.raises(ValueError):
        O.ln_mlp_train_fwd(x, layers, 0.0, [21, 22], act="softmax")
