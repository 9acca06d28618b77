"""CPU model of the pointwise family (src/models/basic/models/mf.py, svd.py,
wrmf.py) in plain numpy, parameterised by dtype: every array keeps the dtype
of the tables it is given, so the same code is the float64 reference and its
float32 rendition.

grads      the loss (mf.py:47-59, svd.py:50-62, wrmf.py:52-66) and its
           gradient as TF1 hands it to the optimizer: the rows of U and V as
           IndexedSlices with duplicate rows summed, K's dense;
step       one optimizer step (tf.train.AdagradOptimizer: sparse on U and V,
           one update per distinct row; dense on K), mutates the tables;
predict    clip_by_value(pred, lo, hi) (mf.py:77-79).
Pinned to torch autograd of the literal loss graphs in
tests/test_pointwise_model.py.
"""
import numpy as np


def _rows(ui):
    ui = np.asarray(ui)
    return ui[:, 0].astype(np.int64), ui[:, 1].astype(np.int64)


def raw_predict(kind, U, V, K, ui):
    u, i = _rows(ui)
    Uu = U[u] @ K if kind == "svd" else U[u]
    return (Uu * V[i]).sum(axis=1)


def predict(kind, U, V, K, ui, lo, hi):
    dt = U.dtype.type
    return np.clip(raw_predict(kind, U, V, K, ui), dt(lo), dt(hi))


def sum_rows(idx, g):
    """Duplicate rows summed: (distinct rows ascending, their summed gradients)."""
    uniq, inv = np.unique(idx, return_inverse=True)
    out = np.zeros((uniq.shape[0], g.shape[1]), dtype=g.dtype)
    np.add.at(out, inv, g)
    return uniq, out


def grads(kind, U, V, K, ui, r, reg, weight=1.0):
    dt = U.dtype.type
    u, i = _rows(ui)
    s = dt(np.float32(np.sqrt(weight)))      # np.sqrt(weight) enters the float32 graph as a constant
    reg = dt(reg)
    Uu, Vi = U[u], V[i]
    P = Uu @ K if kind == "svd" else Uu
    es = ((P * Vi).sum(axis=1) - np.asarray(r).astype(U.dtype)) * s
    loss = dt(0.5) * (es * es).sum() + reg * (dt(0.5) * (Uu * Uu).sum() + dt(0.5) * (Vi * Vi).sum())
    w = (es * s)[:, None]
    gK = None
    if kind == "svd":
        gU = w * (Vi @ K.T) + reg * Uu
        gK = (w * Uu).T @ Vi
    else:
        gU = w * Vi + reg * Uu
    gV = w * P + reg * Vi
    return float(loss), sum_rows(u, gU), sum_rows(i, gV), gK


def adagrad_rows(X, A, rows, g, lr):
    """SparseApplyAdagrad on distinct rows."""
    A[rows] += g * g
    X[rows] -= X.dtype.type(lr) * g / np.sqrt(A[rows])


def step(kind, T, ui, r, reg, lr=0.1, weight=1.0):
    """T: dict user, item, acc_user, acc_item (svd: kernel, acc_kernel)."""
    K = T.get("kernel")
    loss, (ru, gU), (ri, gV), gK = grads(kind, T["user"], T["item"], K, ui, r, reg, weight)
    adagrad_rows(T["user"], T["acc_user"], ru, gU, lr)
    adagrad_rows(T["item"], T["acc_item"], ri, gV, lr)
    if kind == "svd":
        T["acc_kernel"] += gK * gK
        T["kernel"] -= K.dtype.type(lr) * gK / np.sqrt(T["acc_kernel"])
    return loss
