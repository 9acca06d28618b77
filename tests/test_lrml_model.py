"""The CPU model of LRML (tests/lrml_model.py) pinned to the reference graph,
and the LRML interface checks that need no GPU.

* ``step`` against torch-CPU autograd of a literal transcription of
  lrml.py:59-80 (float64): the loss and, through the Adagrad accumulators
  AU - 0.1 = g^2 and AV - 0.1 = g^2, the summed gradient of every row, to
  1e-12, on a batch with a hot user, a user in both roles, i = i', a row whose
  negative pair equals its positive pair, and both hinge branches.
* ``predict("reference")`` against a literal transcription of lrml.py:86-104.
* the float32 drift of the model against itself in float64 over the ten
  golden-stream steps: under 0.25 of conftest's default band, which leaves the
  GPU tests 4x for atomic order and the device's expf.
"""
import ctypes

import numpy as np
import pytest
import torch

import lrml_cases as C
import lrml_model as LM
from conftest import ATOL, RTOL
from collaborativefilteringusingtensorflow_amd import _native as N


def _ref_loss(U, V, Key, Mem, pos, neg, margin):
    """lrml.py:59-80, line by line, on torch tensors."""
    pos_user_embed = U[pos[:, 0]]
    pos_item_embed = V[pos[:, 1]]
    neg_user_embed = U[neg[:, 0]]
    neg_item_embed = V[neg[:, 1]]
    useritem_embed = pos_user_embed * pos_item_embed
    attention = torch.softmax(useritem_embed @ Key, dim=-1)
    relation = attention @ Mem
    pos_score = torch.sum((pos_user_embed + relation - pos_item_embed) ** 2, dim=-1)
    neg_score = torch.sum((neg_user_embed + relation - neg_item_embed) ** 2, dim=-1)
    return torch.sum(torch.relu(pos_score + margin - neg_score))


def _ref_predict(U, V, Key, Mem, users):
    """lrml.py:86-104, line by line."""
    tst_user_embed = U[users].unsqueeze(1)                      # (U, 1, K)
    all_item_embed = V.unsqueeze(0)                             # (1, I, K)
    useritem_embed_ = tst_user_embed * all_item_embed           # (U, I, K)
    attention_ = torch.softmax(useritem_embed_.unsqueeze(2) * Key.t(), dim=-1)   # (U, I, N, K)
    relation_ = torch.sum(attention_ * Mem, dim=2)              # (U, I, K)
    return -torch.sum((tst_user_embed + relation_ - all_item_embed) ** 2, dim=-1)


def test_step_matches_autograd_of_the_reference_graph():
    nu, ni, d, M, B = 30, 40, 12, 7, 48
    U0, V0, Key, Mem = (t.astype(np.float64) for t in C.init_tables(5, nu, ni, d, M, 0.3))
    rng = np.random.RandomState(9)
    pos, neg = C.edge_batch(rng, nu, ni, B)
    assert (pos[:, 0] == 3).sum() >= B // 3                     # a hot user
    assert np.intersect1d(pos[:, 0], neg[:, 0]).size > 0        # a user in both roles
    assert (pos[:, 1] == neg[:, 1]).any() and (pos[-1] == neg[-1]).all()
    tU, tV = (torch.tensor(x, requires_grad=True) for x in (U0, V0))
    loss_t = _ref_loss(tU, tV, torch.tensor(Key), torch.tensor(Mem), torch.tensor(pos), torch.tensor(neg), 0.2)
    loss_t.backward()
    U, V = U0.copy(), V0.copy()
    AU, AV = np.full_like(U, 0.1), np.full_like(V, 0.1)
    loss, h = LM.step(U, V, AU, AV, Key, Mem, pos, neg, **C.HP)
    active = float((h > 0).mean())
    assert 0.2 < active < 0.9, active                           # both hinge branches
    assert abs(loss - loss_t.item()) <= 1e-12 * abs(loss_t.item())
    gU, gV = tU.grad.numpy(), tV.grad.numpy()
    assert np.abs(AU - 0.1 - gU * gU).max() <= 1e-12
    assert np.abs(AV - 0.1 - gV * gV).max() <= 1e-12
    # the update and the clip of every row (lrml.py:106-116)
    for X, X0, A, g in ((U, U0, AU, gU), (V, V0, AV, gV)):
        W = X0 - 0.01 * g / np.sqrt(A)
        W = W * 1.0 / np.maximum(np.sqrt((W * W).sum(1, keepdims=True)), 1.0)
        assert np.abs(X - W).max() <= 1e-12
        assert np.sqrt((X * X).sum(1)).max() <= 1.0 + 1e-12


@pytest.mark.parametrize("nu,ni,d,M", [(6, 9, 5, 3), (4, 11, 17, 33), (3, 7, 1, 1)])
def test_predict_reference_matches_literal_transcription(nu, ni, d, M):
    U, V, Key, Mem = (t.astype(np.float64) for t in C.init_tables(nu + d, nu, ni, d, M, 0.7))
    users = np.arange(nu)
    S = LM.predict(U, V, Key, Mem, users, "reference")
    R = _ref_predict(*(torch.tensor(x) for x in (U, V, Key, Mem)), torch.tensor(users)).numpy()
    assert np.abs(S - R).max() <= 1e-12 * np.abs(R).max()
    # not the training attention: the two modes differ
    if M > 1:
        assert np.abs(LM.predict(U, V, Key, Mem, users, "train") - S).max() > 1e-3
    # recommend: train items out, ties to the lower id
    indptr = np.arange(nu + 1, dtype=np.int64)
    indices = (np.arange(nu) % ni).astype(np.int32)
    S2 = np.zeros_like(S)
    rec = LM.recommend(S2, indptr, indices, users, 3)
    for u, row in enumerate(rec):
        assert row == [i for i in range(ni) if i != indices[u]][:3]


@pytest.mark.parametrize("stddev", [0.01, 0.3])
def test_fp32_drift_stays_under_a_quarter_of_the_band(stddev):
    d, M = 50, 20
    pos, neg = C.stream()
    batches = list(zip(pos[:10], neg[:10]))
    tabs = C.init_tables(C.INIT_SEEDS[(d, M, stddev)], C.NU, C.NI, d, M, stddev)
    T64, l64, h64 = C.run_model(tabs, batches, np.float64)
    T32, l32, h32 = C.run_model(tabs, batches, np.float32)
    assert C.min_abs_h(h64) > C.H_MIN
    assert all(np.array_equal(a > 0, b > 0) for a, b in zip(h64, h32))     # no branch flips
    if stddev == 0.3:   # the clip bites and a good part of the rows is inactive
        assert 0.2 < np.mean([np.mean(h <= 0) for h in h64]) < 0.5
        assert np.sqrt((tabs[0].astype(np.float64) ** 2).sum(1)).min() > 1.0
    for name in ("user", "item", "acc_user", "acc_item"):
        r = C.band_ratio(T32[name], T64[name], RTOL, ATOL)
        print("fp32 drift / band, stddev %g, %s: %.4f" % (stddev, name, r))
        assert r <= 0.25, (name, r)
    for a, b in zip(l32, l64):
        assert abs(a - b) <= 0.25e-5 * abs(b)


def test_interface_rejections():
    from collaborativefilteringusingtensorflow_amd.lrml import LRML, LRMLEngine
    with pytest.raises(ValueError):
        LRML(10, 10, predict_mode="x")
    L = N.lib()
    h = ctypes.c_void_p()
    assert L.cf_lrml_create(10, 10, 129, 20, 0.2, 1.0, 0.01, 0.1, 0, ctypes.byref(h)) == -1
    assert b"n_factors must be 1..128" in L.cf_last_error()
    assert L.cf_lrml_create(10, 10, 50, 65, 0.2, 1.0, 0.01, 0.1, 0, ctypes.byref(h)) == -1
    assert b"n_memory must be 1..64" in L.cf_last_error()
    assert N.LRML_MODES == {"reference": 0, "train": 1}
    if N.device_count() > 0:
        return
    with pytest.raises(N.NativeError, match="no HIP device"):
        LRMLEngine(10, 10, 8, 4)
