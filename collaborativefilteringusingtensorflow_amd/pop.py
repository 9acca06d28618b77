"""PopRank drop-in (src/models/basic/models/pop.py:11-62): items ranked by
train count, ties to the lower id (Python's stable ``sorted(reverse=True)``,
pop.py:22), the user's train items skipped, then ranking.evaluateCV /
evaluateLOOV.  ``PopRank.train(fold, trasR, tstsR)`` runs on the native
neighbourhood object (``cf_knn_score_topk``, kind POP)."""
from ._knn import KnnEngine, KnnModel

__all__ = ["PopRank", "KnnEngine"]


class PopRank(KnnModel):
    KIND = "pop"

    def __init__(self, n_users, n_items, topN=5, split_method='cv', eval_metrics=['rmse', 'mae'], device=0):
        self._init_common(n_users, n_items, topN, split_method, eval_metrics, device)
