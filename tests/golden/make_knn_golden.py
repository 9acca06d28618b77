"""Generate ``knn_*.npz`` from the *reference itself*.

Test infrastructure only, as ``make_golden.py``: it runs where the read-only
reference checkout lives and imports its four memory-based classes
(src/models/basic/models/{pop,usercf,itemcf}.py,
src/models/others/models/useritemcf.py); the tests only read the files.

Per case (a random binary matrix with uneven row and column propensities,
topN = 5, theta = 0.8) the file holds data only:

* ``R`` and a test matrix ``T`` (uint8), ``test_users`` in the reference's order;
* ``sim_user`` / ``sim_item``: the reference's ``__calsim__`` matrices (float32);
* the reference's top-K'd matrices: ``ucf_topk`` (usercf.py:34-39 applied to
  every row: ``argsort[-K:]``, ``sim > 0``), ``icf_topk`` (itemcf.py:29-40),
  ``uicf_user_topk`` / ``uicf_item_topk`` (useritemcf.py:33-39), as
  (row, column, value) triplets;
* ``{ucf,icf,uicf}_pred``: ``__predict__`` of the trained instance (float64);
* ``{pop,ucf,icf,uicf}_lists`` (padded with -1) and ``_scores``;
* ``numpy_version``.

Conditions on a fixture, asserted here (another seed is taken otherwise):
at most 20 % of a side's rows have equal, positive K-th and (K+1)-th largest
similarities; on the case whose K exceeds every row's positives, adjacent
float64 predictions among each test user's first topN + 1 unmasked items
differ by more than one float32 ulp, for all three models.
"""
import os
import sys

import numpy as np
from scipy.sparse import lil_matrix

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
for sub in ("src/metrics", "src/models/basic/models", "src/models/others/models"):
    p = os.path.join(REF, sub)
    if p not in sys.path:
        sys.path.insert(0, p)
sys.path.insert(0, os.path.dirname(HERE))

TOPN, THETA = 5, 0.8
METRICS = ['pre', 'recall', 'map', 'mrr', 'ndcg']
CASES = [("97x131_k8", 97, 131, 8, 24), ("257x300_k32", 257, 300, 32, 40), ("130x70_k200", 130, 70, 200, 40)]
TIE_CAP = 0.20


def draw(n_users, n_items, n_test, seed):
    rng = np.random.RandomState(seed)
    pu = rng.uniform(0.15, 1.0, n_users)
    pi = rng.uniform(0.05, 0.6, n_items) ** 1.5
    full = rng.random_sample((n_users, n_items)) < np.outer(pu, pi)
    full[:, rng.randint(n_items)] |= rng.random_sample(n_users) < 0.7   # one popular item
    T = np.zeros_like(full)
    for u in rng.choice(n_users, n_test, replace=False):
        held = np.nonzero(full[u])[0]
        if held.size >= 4:
            T[u, rng.choice(held, max(1, held.size // 4), replace=False)] = True
    R = full & ~T
    return R.astype(np.uint8), T.astype(np.uint8)


def triplets(M):
    r, c = np.nonzero(M)
    return np.stack([r, c]).astype(np.int32), np.asarray(M[r, c], dtype=np.float32)


def ucf_topk_matrix(S, K):
    out = np.zeros_like(S)
    n = S.shape[0]
    for u in range(n):
        inds = np.argsort(S[u, :])[-K:] if K < n else range(n)   # usercf.py:34-37
        for v in inds:
            if S[u, v] > 0:                                        # usercf.py:39
                out[u, v] = S[u, v]
    return out


def lists_array(lists):
    out = np.full((len(lists), TOPN), -1, dtype=np.int32)
    for r, l in enumerate(lists):
        out[r, :len(l)] = l
    return out


def separated(pred, R, users):
    """Adjacent float64 predictions among each user's first TOPN + 1 unmasked
    items differ by more than one float32 ulp."""
    for row, u in enumerate(users):
        p = np.sort(np.asarray(pred[row])[R[u] == 0])[::-1][:TOPN + 1]
        gap = p[:-1] - p[1:]
        if (gap <= np.spacing(np.abs(p[:-1]).astype(np.float32)).astype(np.float64)).any():
            return False
    return True


def run_case(name, n_users, n_items, K, n_test, seed):
    import knn_model as M
    from pop import PopRank
    from usercf import UserCF
    from itemcf import ItemCF
    from useritemcf import UserItemCF
    R, T = draw(n_users, n_items, n_test, seed)
    trasR, tstsR = lil_matrix(R.astype(np.float32)), lil_matrix(T.astype(np.float32))
    test_users = list(set(np.asarray(tstsR.nonzero()[0])))
    if max(R[u].sum() for u in test_users) > n_items - TOPN - 1:
        return None

    ucf = UserCF(n_users, n_items, K, TOPN, 'cv', METRICS)
    ucf_scores = ucf.train(1, trasR, tstsR)
    sim_user = np.array(ucf._UserCF__simMat, dtype=np.float32)
    sim_item = np.array(ItemCF(n_users, n_items, K).__calsim__(trasR), dtype=np.float32)
    assert ucf._UserCF__simMat.dtype == np.float32
    for side, S in ((0, sim_user), (1, sim_item)):
        if M.tied_rows(S, K).mean() > TIE_CAP:
            return None
    out = {"R": R, "T": T, "test_users": np.asarray(test_users, dtype=np.int32), "topK": np.int64(K),
           "topN": np.int64(TOPN), "theta": np.float64(THETA), "sim_user": sim_user, "sim_item": sim_item,
           "numpy_version": np.array(np.__version__), "seed": np.int64(seed)}
    out["ucf_topk_rc"], out["ucf_topk_v"] = triplets(ucf_topk_matrix(sim_user, K))
    out["ucf_pred"] = np.array(ucf.__predict__(trasR, test_users), dtype=np.float64)
    out["ucf_lists"] = lists_array(ucf._UserCF__recommend(trasR, test_users))
    out["ucf_scores"] = np.asarray(ucf_scores, dtype=np.float64)

    icf = ItemCF(n_users, n_items, K, TOPN, 'cv', METRICS)
    out["icf_scores"] = np.asarray(icf.train(1, trasR, tstsR), dtype=np.float64)
    out["icf_topk_rc"], out["icf_topk_v"] = triplets(icf._ItemCF__simMat)
    out["icf_pred"] = np.array(icf.__predict__(trasR, test_users), dtype=np.float64)
    out["icf_lists"] = lists_array(icf._ItemCF__recommend(trasR, test_users))

    uicf = UserItemCF(n_users, n_items, K, THETA, TOPN, 'cv', METRICS)
    out["uicf_scores"] = np.asarray(uicf.train(1, trasR, tstsR), dtype=np.float64)
    out["uicf_user_topk_rc"], out["uicf_user_topk_v"] = triplets(uicf._UserItemCF__userSimMat)
    out["uicf_item_topk_rc"], out["uicf_item_topk_v"] = triplets(uicf._UserItemCF__itemSimMat)
    out["uicf_pred"] = np.array(uicf.__predict__(trasR, test_users), dtype=np.float64)
    out["uicf_lists"] = lists_array(uicf._UserItemCF__recommend(trasR, test_users))

    pop = PopRank(n_users, n_items, TOPN, 'cv', METRICS)
    out["pop_scores"] = np.asarray(pop.train(1, trasR, tstsR), dtype=np.float64)
    out["pop_lists"] = lists_array(pop._PopRank__recommend(trasR, test_users))

    if K >= max(n_users, n_items):   # the end-to-end case: no near tie may decide a list
        for m in ("ucf", "icf", "uicf"):
            if not separated(out[m + "_pred"], R, test_users):
                return None
    return out


if __name__ == "__main__":
    for name, n_users, n_items, K, n_test in CASES:
        for seed in range(100, 160):
            case = run_case(name, n_users, n_items, K, n_test, seed)
            if case is not None:
                break
        else:
            raise SystemExit("no seed gave a valid fixture for " + name)
        path = os.path.join(HERE, "knn_%s.npz" % name)
        np.savez_compressed(path, **case)
        print(name, "seed", seed, "->", path, os.path.getsize(path), "bytes")
