"""UserItemCF drop-in (src/models/others/models/useritemcf.py:13-95): the
user-side and the item-side cosine similarities, each row cut to its ``topK``
largest (useritemcf.py:33-39; ties across the K-th place go to the lower id),
pred[u, :] = sum_v theta S_user[u, v] R[v, :] + sum_{i in R_u} (1 - theta)
S_item[i, :] with float32 terms (useritemcf.py:41-51), top-N with the train
items skipped, then ranking.evaluateCV / evaluateLOOV.
``UserItemCF.train(fold, trasR, tstsR)`` runs on the native neighbourhood
object (``cf_knn_fit``, ``cf_knn_score_topk``, kind USERITEM)."""
from ._knn import KnnEngine, KnnModel

__all__ = ["UserItemCF", "KnnEngine"]


class UserItemCF(KnnModel):
    KIND = "useritem"

    def __init__(self, n_users, n_items, topK=50, theta=.5, topN=5, split_method='cv',
                 eval_metrics=['rmse', 'mae'], device=0):
        self._init_common(n_users, n_items, topN, split_method, eval_metrics, device)
        self._topK, self._theta = int(topK), float(theta)
