"""ItemCF drop-in (src/models/basic/models/itemcf.py:11-94): cosine
similarities of the binarised item columns (itemcf.py:19-27), every row cut to
its ``topK`` largest (itemcf.py:29-40; ties across the K-th place go to the
lower id), pred[u, :] = sum of the cut rows of the user's own items
(itemcf.py:42-50), top-N with the train items skipped, then
ranking.evaluateCV / evaluateLOOV.  ``ItemCF.train(fold, trasR, tstsR)`` runs
on the native neighbourhood object (``cf_knn_fit``, ``cf_knn_score_topk``,
kind ITEM)."""
from ._knn import KnnEngine, KnnModel

__all__ = ["ItemCF", "KnnEngine"]


class ItemCF(KnnModel):
    KIND = "item"

    def __init__(self, n_users, n_items, topK=50, topN=5, split_method='cv', eval_metrics=['rmse', 'mae'],
                 device=0):
        self._init_common(n_users, n_items, topN, split_method, eval_metrics, device)
        self._topK = int(topK)
