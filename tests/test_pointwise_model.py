"""The numpy model of MF / SVD / WRMF (tests/pointwise_model.py) against torch
autograd of the literal loss graphs (mf.py:47-68, svd.py:50-71, wrmf.py:52-75)
in float64, and its dedup-then-Adagrad against a per-distinct-row loop."""
import numpy as np
import pytest
import torch

import pointwise_cases as C
import pointwise_model as PM


def literal_loss(kind, U, V, K, ui, r, reg, weight):
    """The TF graph, op for op: embedding_lookup, reduce_sum, l2_loss."""
    u = torch.as_tensor(ui[:, 0].astype(np.int64))
    i = torch.as_tensor(ui[:, 1].astype(np.int64))
    ue, ie = U[u], V[i]
    if kind == "svd":
        pred = (torch.matmul(ue, K) * ie).sum(1)
    else:
        pred = (ue * ie).sum(1)
    diff = pred - torch.as_tensor(r.astype(np.float64))
    if kind == "wrmf":
        diff = diff * float(np.float32(np.sqrt(weight)))
    l2 = lambda x: (x * x).sum() / 2
    return l2(diff) + reg * (l2(ue) + l2(ie))


@pytest.mark.parametrize("kind", ["mf", "svd", "wrmf"])
@pytest.mark.parametrize("d", [1, 17, 32])
def test_gradients_match_autograd(kind, d):
    rng = np.random.RandomState(d)
    T = C.cast(C.init_tables(kind, 3, C.EDGE_NU, C.EDGE_NI, d, 0.3), np.float64)
    ui, r = C.edge_batch(rng, C.EDGE_NU, C.EDGE_NI, 63)
    tU = torch.tensor(T["user"], requires_grad=True)
    tV = torch.tensor(T["item"], requires_grad=True)
    tK = torch.tensor(T["kernel"], requires_grad=True) if kind == "svd" else None
    loss = literal_loss(kind, tU, tV, tK, ui, r, C.REG, C.WEIGHT[kind])
    loss.backward()
    lo, (ru, gU), (ri, gV), gK = PM.grads(kind, T["user"], T["item"], T.get("kernel"), ui, r, C.REG, C.WEIGHT[kind])
    assert abs(lo - loss.item()) <= 1e-12 * abs(loss.item())
    for rows, g, t in ((ru, gU, tU), (ri, gV, tV)):
        dense = t.grad.numpy()
        np.testing.assert_allclose(g, dense[rows], rtol=1e-12, atol=1e-15)
        rest = np.setdiff1d(np.arange(dense.shape[0]), rows)
        assert not dense[rest].any()           # IndexedSlices: no other row has a gradient
    if kind == "svd":
        np.testing.assert_allclose(gK, tK.grad.numpy(), rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("kind", ["mf", "svd", "wrmf"])
def test_step_is_one_adagrad_update_per_distinct_row(kind):
    d = 9
    rng = np.random.RandomState(2)
    T0 = C.cast(C.init_tables(kind, 5, C.EDGE_NU, C.EDGE_NI, d, 0.3), np.float64)
    ui, r = C.edge_batch(rng, C.EDGE_NU, C.EDGE_NI, 40)
    T = {n: t.copy() for n, t in T0.items()}
    PM.step(kind, T, ui, r, C.REG, C.LR, C.WEIGHT[kind])
    # the loop: per distinct row, the occurrences' gradient rows added, one update
    tU = torch.tensor(T0["user"], requires_grad=True)
    tV = torch.tensor(T0["item"], requires_grad=True)
    tK = torch.tensor(T0["kernel"], requires_grad=True) if kind == "svd" else None
    literal_loss(kind, tU, tV, tK, ui, r, C.REG, C.WEIGHT[kind]).backward()
    for name, t, col in (("user", tU, 0), ("item", tV, 1)):
        X, A = T0[name].copy(), T0["acc_" + name].copy()
        for row in sorted(set(ui[:, col].tolist())):
            g = t.grad.numpy()[row]
            A[row] = A[row] + g * g
            X[row] = X[row] - C.LR * g / np.sqrt(A[row])
        np.testing.assert_allclose(T[name], X, rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(T["acc_" + name], A, rtol=1e-12, atol=1e-15)
        untouched = np.setdiff1d(np.arange(X.shape[0]), ui[:, col])
        assert np.array_equal(T[name][untouched], T0[name][untouched])
        assert np.array_equal(T["acc_" + name][untouched], T0["acc_" + name][untouched])
    if kind == "svd":
        g = tK.grad.numpy()
        A = T0["acc_kernel"] + g * g
        np.testing.assert_allclose(T["acc_kernel"], A, rtol=1e-12)
        np.testing.assert_allclose(T["kernel"], T0["kernel"] - C.LR * g / np.sqrt(A), rtol=1e-12, atol=1e-15)


def test_predict_clips_to_the_range():
    T = C.cast(C.init_tables("svd", 1, 10, 12, 5, 1.0), np.float64)
    ui = np.stack([np.arange(10), np.arange(10)], 1)
    raw = PM.raw_predict("svd", T["user"], T["item"], T["kernel"], ui)
    p = PM.predict("svd", T["user"], T["item"], T["kernel"], ui, -0.5, 0.5)
    assert (raw < -0.5).any() and (raw > 0.5).any()
    assert np.array_equal(p, np.minimum(np.maximum(raw, -0.5), 0.5))
    want = np.einsum("bk,kn,bn->b", T["user"][:10], T["kernel"], T["item"][:10])
    np.testing.assert_allclose(raw, want, rtol=1e-12)
