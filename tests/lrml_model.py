"""CPU model of LRML (src/models/others/models/lrml.py) in plain numpy,
parameterised by dtype: every array keeps the dtype of the tables it is given,
so the same code is the float64 reference and its float32 rendition.

step       one optimizer step (lrml.py:59-80, 106-116): mutates U, V, AU, AV,
           returns (loss, h) with h the per-row hinge argument;
predict    the scores of lrml.py:86-104 ("reference": softmax over the factor
           axis per memory slot) or of the training attention ("train");
recommend  top-k of the scores without the users' train items, ties to the
           lower id.
Pinned to torch autograd of literal transcriptions in tests/test_lrml_model.py.
"""
import numpy as np


def _attend(e, Key, Mem):
    z = e @ Key
    z = z - z.max(axis=1, keepdims=True)
    a = np.exp(z)
    a = a / a.sum(axis=1, keepdims=True)
    return a, a @ Mem


def _clip_rows(X, c):
    # tf.clip_by_norm(X, c, axes=[1]): X * c / max(|row|, c)
    n = np.sqrt((X * X).sum(axis=1, keepdims=True))
    X[...] = X * c / np.maximum(n, c)


def step(U, V, AU, AV, Key, Mem, pos, neg, margin=0.2, clip_norm=1.0, lr=0.01):
    dt = U.dtype.type
    pos, neg = np.asarray(pos, np.int64), np.asarray(neg, np.int64)
    pu, pi, nu, ni = pos[:, 0], pos[:, 1], neg[:, 0], neg[:, 1]
    uu, vi, un, vn = U[pu], V[pi], U[nu], V[ni]
    a, r = _attend(uu * vi, Key, Mem)
    dp = uu + r - vi
    dn = un + r - vn
    h = (dp * dp).sum(axis=1) + dt(margin) - (dn * dn).sum(axis=1)
    act = (h > 0).astype(U.dtype)[:, None]
    loss = float(h[h > 0].astype(np.float64).sum())
    g_r = dt(2) * (dp - dn)
    g_a = g_r @ Mem.T
    g_z = a * (g_a - (a * g_a).sum(axis=1, keepdims=True))
    g_e = g_z @ Key.T
    GU, GV = np.zeros_like(U), np.zeros_like(V)
    np.add.at(GU, pu, act * (dt(2) * dp + g_e * vi))
    np.add.at(GV, pi, act * (-dt(2) * dp + g_e * uu))
    np.add.at(GU, nu, act * (-dt(2) * dn))
    np.add.at(GV, ni, act * (dt(2) * dn))
    for X, A, G in ((U, AU, GU), (V, AV, GV)):   # SparseApplyAdagrad; a zero row is a no-op
        A += G * G
        X -= dt(lr) * G / np.sqrt(A)
        _clip_rows(X, dt(clip_norm))
    return loss, h


def predict(U, V, Key, Mem, users, mode="reference"):
    users = np.asarray(users, np.int64)
    S = np.empty((len(users), V.shape[0]), dtype=U.dtype)
    for c, u in enumerate(users):
        e = U[u][None, :] * V                                  # [I, d]
        if mode == "reference":
            x = e[:, None, :] * Key.T[None, :, :]               # [I, M, d]
            x = x - x.max(axis=2, keepdims=True)
            att = np.exp(x)
            att = att / att.sum(axis=2, keepdims=True)
            rel = (att * Mem[None, :, :]).sum(axis=1)
        elif mode == "train":
            rel = _attend(e, Key, Mem)[1]
        else:
            raise ValueError(mode)
        t = U[u][None, :] + rel - V
        S[c] = -(t * t).sum(axis=1)
    return S


def recommend(S, indptr, indices, users, k):
    out = []
    for c, u in enumerate(np.asarray(users, np.int64)):
        s = np.array(S[c], dtype=np.float64)
        s[indices[indptr[u]:indptr[u + 1]]] = -np.inf
        out.append(np.argsort(-s, kind="stable")[:k].tolist())
    return out
