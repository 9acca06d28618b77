"""Host model of the neighbourhood family (csrc/cf_knn.hip) -- test
infrastructure, not part of the product.  A numpy restatement of what
pop.py, usercf.py, itemcf.py and useritemcf.py compute on a binary matrix,
with this project's tie rule:

* similarities: float32, S[a, b] = fl32(fl32(c / den_lo) / den_hi) with c the
  intersection count, den_x = float32(sqrt(nnz_x)), lo = min(a, b), hi =
  max(a, b); the diagonal and every pair without a common member are 0;
* neighbours: a row's topK largest positive similarities by (similarity
  descending, id ascending), padded with (-1, 0);
* predictions: float64 sums of float32 terms, added in table order;
* recommend: top-N of float32(prediction), ties to the lower id, the user's
  train items skipped.

R is a dense 0/1 array [n_users, n_items]; side 0 = users, 1 = items.
"""
import numpy as np

KINDS = ("pop", "user", "item", "useritem")


def similarity(R, side):
    A = np.asarray(R) != 0
    if side == 1:
        A = A.T
    A = A.astype(np.int64)
    c = A @ A.T
    den = np.sqrt(A.sum(1).astype(np.float32))   # float32 sqrt, IEEE
    ids = np.arange(A.shape[0])
    lo, hi = np.minimum.outer(ids, ids), np.maximum.outer(ids, ids)
    with np.errstate(divide="ignore", invalid="ignore"):
        S = (c.astype(np.float32) / den[lo]) / den[hi]
    assert S.dtype == np.float32
    S[c == 0] = 0.0
    S[ids, ids] = 0.0
    return S


def neighbours(S, topK):
    """(ids int32, sims float32) [n, topK] from a dense similarity matrix."""
    n = S.shape[0]
    idx = np.full((n, topK), -1, dtype=np.int32)
    sim = np.zeros((n, topK), dtype=np.float32)
    ids = np.arange(n)
    for r in range(n):
        order = np.lexsort((ids, -S[r].astype(np.float64)))   # similarity descending, then id ascending
        order = order[S[r, order] > 0][:topK]
        idx[r, :order.size] = order
        sim[r, :order.size] = S[r, order]
    return idx, sim


def tables_from_matrix(M, topK):
    """A reference top-K'd matrix (at most topK nonzeros a row) as neighbour
    tables, by the same order rule."""
    assert (np.count_nonzero(M, axis=1) <= topK).all()
    return neighbours(np.asarray(M, dtype=np.float32), topK)


def tied_rows(S, topK):
    """Rows whose K-th and (K+1)-th largest similarities are equal and positive."""
    if S.shape[1] <= topK:
        return np.zeros(S.shape[0], dtype=bool)
    d = -np.sort(-S, axis=1)
    return (d[:, topK - 1] == d[:, topK]) & (d[:, topK - 1] > 0)


def user_terms(kind, theta, sim):
    return np.float32(theta) * sim if kind == "useritem" else sim


def item_terms(kind, theta, sim):
    return np.float32(1. - theta) * sim if kind == "useritem" else sim


def predict(kind, R, users, nb_user=None, nb_item=None, theta=0.0):
    """float64 [len(users), n_items]."""
    R = np.asarray(R) != 0
    out = np.zeros((len(users), R.shape[1]), dtype=np.float64)
    for row, u in enumerate(users):
        pred = out[row]
        if kind == "pop":
            pred += R.sum(0)
            continue
        if kind in ("user", "useritem"):
            idx, sim = nb_user[0][u], user_terms(kind, theta, nb_user[1][u])
            assert sim.dtype == np.float32
            for v, t in zip(idx, sim):
                if v >= 0:
                    pred[R[v]] += np.float64(t)
        if kind in ("item", "useritem"):
            for i in np.nonzero(R[u])[0]:
                idx, sim = nb_item[0][i], item_terms(kind, theta, nb_item[1][i])
                assert sim.dtype == np.float32
                ok = idx >= 0
                pred[idx[ok]] += sim[ok].astype(np.float64)   # a row's ids are distinct
    return out


def recommend(pred, R, users, k, exclude_train=True):
    """(ids int32 [n, k] padded with -1, vals float32 padded with NaN)."""
    R = np.asarray(R) != 0
    n_items = R.shape[1]
    idx = np.full((len(users), k), -1, dtype=np.int32)
    val = np.full((len(users), k), np.nan, dtype=np.float32)
    ids = np.arange(n_items)
    for row, u in enumerate(users):
        s = pred[row].astype(np.float32)
        order = np.lexsort((ids, -s.astype(np.float64)))
        if exclude_train:
            order = order[~R[u, order]]
        order = order[:k]
        idx[row, :order.size] = order
        val[row, :order.size] = s[order]
    return idx, val


def fit(kind, R, topK):
    """(nb_user, nb_item): the tables the kind reads, None for the others."""
    nb_user = neighbours(similarity(R, 0), topK) if kind in ("user", "useritem") else None
    nb_item = neighbours(similarity(R, 1), topK) if kind in ("item", "useritem") else None
    return nb_user, nb_item


def order_free(terms_per_cell):
    """The precondition under which a float64 sum of float32 terms is exact in
    any order: (max exponent - min exponent) + ceil(log2(#terms)) + 24 <= 53
    over the nonzero terms of the cell."""
    t = np.asarray([x for x in terms_per_cell if x != 0], dtype=np.float64)
    if t.size == 0:
        return True
    e = np.frexp(np.abs(t))[1]
    return int(e.max() - e.min()) + int(np.ceil(np.log2(t.size))) + 24 <= 53
