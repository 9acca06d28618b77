"""The neighbourhood fixtures (tests/golden/knn_*.npz, written by
tests/golden/make_knn_golden.py from the reference) and the edge shapes of
tests/test_gpu_knn.py -- test infrastructure."""
import functools
import os

import numpy as np

import knn_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("97x131_k8", "257x300_k32", "130x70_k200")
FULL_CASE = "130x70_k200"   # K exceeds every row's positives: no K-boundary tie exists
REF_MODELS = {"ucf": "user", "icf": "item", "uicf": "useritem"}
METRICS = ['pre', 'recall', 'map', 'mrr', 'ndcg']


def _dense(z, name, n):
    (r, c), v = z[name + "_rc"], z[name + "_v"]
    out = np.zeros((n, n), dtype=np.float32)
    out[r, c] = v
    return out


@functools.lru_cache(maxsize=None)
def load(name):
    """One fixture, read once and shared; callers leave it unchanged."""
    with np.load(os.path.join(GOLDEN, "knn_%s.npz" % name)) as z:
        c = {k: z[k] for k in z.files}
    n_users, n_items = c["R"].shape
    c["topK"], c["topN"], c["theta"] = int(c["topK"]), int(c["topN"]), float(c["theta"])
    c["ucf_topk"] = _dense(c, "ucf_topk", n_users)
    c["icf_topk"] = _dense(c, "icf_topk", n_items)
    c["uicf_user_topk"] = _dense(c, "uicf_user_topk", n_users)
    c["uicf_item_topk"] = _dense(c, "uicf_item_topk", n_items)
    return c


@functools.lru_cache(maxsize=None)
def ref_tables(name, model):
    """The reference's top-K'd matrices of a model as (nb_user, nb_item) tables."""
    c = load(name)
    K = c["topK"]
    if model == "ucf":
        return M.tables_from_matrix(c["ucf_topk"], K), None
    if model == "icf":
        return None, M.tables_from_matrix(c["icf_topk"], K)
    return M.tables_from_matrix(c["uicf_user_topk"], K), M.tables_from_matrix(c["uicf_item_topk"], K)


@functools.lru_cache(maxsize=None)
def model_fit(name):
    """The model's own similarity matrices and neighbour tables of a fixture."""
    c = load(name)
    S = (M.similarity(c["R"], 0), M.similarity(c["R"], 1))
    return S, (M.neighbours(S[0], c["topK"]), M.neighbours(S[1], c["topK"]))


def csr(R):
    R = np.asarray(R) != 0
    indptr = np.concatenate([[0], np.cumsum(R.sum(1))]).astype(np.int64)
    return indptr, np.nonzero(R)[1].astype(np.int32)


def edge_matrix(n_users, n_items, empty_item=False, seed=5):
    """A binary matrix with the rows the kernels can go wrong at: an empty
    user (0), a user holding every item (1), two (2, 5) and three (6, 7, the
    last) identical rows, identical columns, one item (3) held by every
    non-empty user.  ``empty_item``: item 2 is held by nobody instead, user 1
    included."""
    rng = np.random.RandomState(seed + 1000 * n_users + n_items)
    R = rng.random_sample((n_users, n_items)) < 0.3
    if n_users < 9 or n_items < 9:   # 2 x 2: an empty user next to a full one
        R[:] = False
        R[1] = True
        if empty_item:
            R[:, n_items - 1] = False
        return R.astype(np.uint8)
    for c in (63, 64, 127, 128):   # members on both sides of the 64- and 128-wide tile edges
        if c < n_items:
            R[8, c] = True
        if c < n_users:
            R[c, 8] = True
    R[:, 3] = True
    R[5] = R[2]
    R[n_users - 1] = R[6]   # across the whole id range
    R[7] = R[6]
    R[:, 4] = R[:, n_items - 1]
    R[1] = True
    if empty_item:
        R[:, 2] = False
    R[0] = False
    return R.astype(np.uint8)
