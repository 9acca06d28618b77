"""UserCF drop-in (src/models/basic/models/usercf.py:11-87): cosine
similarities of the binarised user rows (usercf.py:19-27), the ``topK``
largest positive ones per user (usercf.py:34-39; ties across the K-th place go
to the lower id), pred[u, :] = sum_v S[u, v] R[v, :] (usercf.py:40), top-N
with the train items skipped (usercf.py:44-58), then ranking.evaluateCV /
evaluateLOOV.  ``UserCF.train(fold, trasR, tstsR)`` runs on the native
neighbourhood object (``cf_knn_fit``, ``cf_knn_score_topk``, kind USER)."""
from ._knn import KnnEngine, KnnModel

__all__ = ["UserCF", "KnnEngine"]


class UserCF(KnnModel):
    KIND = "user"

    def __init__(self, n_users, n_items, topK=50, topN=5, split_method='cv', eval_metrics=['rmse', 'mae'],
                 device=0):
        self._init_common(n_users, n_items, topN, split_method, eval_metrics, device)
        self._topK = int(topK)
