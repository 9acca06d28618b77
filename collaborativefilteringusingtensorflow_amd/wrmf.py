"""WRMF drop-in (src/models/basic/models/wrmf.py:11-164): MF on binarised
interactions plus sampled negatives (rating 0), every row weighted by
``weight`` -- the loss is the literal l2_loss((pred - r) * sqrt(weight)) of
wrmf.py:59-60 (the per-sign weighting there is commented out), so the factor
is float32(sqrt(weight))^2, not ``weight``.  Evaluated as a ranker: U[test]
V^T, top-k, train items dropped (wrmf.py:98-111), then ranking.evaluateCV /
evaluateLOOV.

``WRMF.train(fold, trasR, tstsR, sampler)`` follows wrmf.py:114-161 on the
native pointwise object (``cf_pw_step``, ``cf_pw_score_topk``).
"""
import sys
import time

import numpy as np

from ._model import parse_device
from ._pointwise import PointwiseEngine, split_batch
from .io_util import to_csr
from .ranking import evaluateCV, evaluateLOOV

__all__ = ["WRMF", "PointwiseEngine"]


class WRMF(object):
    def __init__(self, n_users, n_items, topN=10, split_method='cv',
                 eval_metrics=['pre', 'recall', 'map', 'mrr', 'ndcg'], weight=1, reg=0.02, n_factors=10,
                 batch_size=500, max_iter=50, lr=.1, init_mean=0.0, init_stddev=0.1, device='CPU',
                 seed=None, verbose=True):
        self._n_users, self._n_items, self._topN = int(n_users), int(n_items), int(topN)
        self._split_method, self._eval_metrics = split_method, list(eval_metrics)
        self._weight, self._reg = float(weight), float(reg)
        self._n_factors, self._batch_size = int(n_factors), int(batch_size)
        self._max_iter, self._lr = int(max_iter), float(lr)
        self._train_lr = float(lr)
        self._init_mean, self._init_stddev = float(init_mean), float(init_stddev)
        self._device = parse_device(device)
        self._seed = seed
        self._verbose = verbose
        self._engine = None
        self._init_tables = None

    @property
    def engine(self):
        return self._engine

    def set_initial_tables(self, user=None, item=None):
        t = {n: np.asarray(a, dtype=np.float32) for n, a in (("user", user), ("item", item)) if a is not None}
        self._init_tables = t or None

    def _recommend(self, test_users):
        idx = self._engine.score_topk(np.asarray(test_users, dtype=np.int32), self._topN, exclude_train=True)
        return [[int(x) for x in row if x >= 0] for row in idx]

    def _eval(self, yss_true, yss_pred):
        if self._split_method == 'cv':
            return evaluateCV(yss_true, yss_pred, self._eval_metrics, self._topN)
        if self._split_method == 'loov':
            return evaluateLOOV(yss_true, yss_pred, self._eval_metrics, self._topN)
        return None

    def train(self, fold, trasR, tstsR, sampler):
        t_indptr, t_indices, _ = to_csr(tstsR)
        test_users = list(set(np.asarray(tstsR.nonzero()[0])))
        yss_true = None
        if self._split_method == 'cv':
            yss_true = [set(t_indices[t_indptr[u]:t_indptr[u + 1]].tolist()) for u in test_users]
        elif self._split_method == 'loov':
            yss_true = [int(t_indices[t_indptr[u]]) for u in test_users]
        indptr, indices, _ = to_csr(trasR)
        n_batches = int(indices.shape[0] / self._batch_size)   # wrmf.py:139
        if self._engine is not None:
            self._engine.close()
        self._engine = eng = PointwiseEngine(self._n_users, self._n_items, self._n_factors, kind="wrmf",
                                             weight=self._weight, reg=self._reg, lr=self._train_lr,
                                             device=self._device)
        eng.set_interactions(indptr, indices)
        seed = self._seed if self._seed is not None else 1
        eng.init_params(self._init_mean, self._init_stddev, seed=seed ^ 0x2468ACE)
        if self._init_tables is not None:
            for name, arr in self._init_tables.items():
                eng.set_table(name, arr)
        draw = getattr(sampler, "_draw", None)
        scores = None
        for it in range(self._max_iter):
            t0 = time.time()
            for _ in range(n_batches):
                ui, r = draw() if draw is not None else split_batch(sampler.next_batch())   # wrmf.py:145-147
                eng.step(ui, r, return_loss=False)
            aveloss = eng.take_loss() / max(n_batches, 1)
            scores = self._eval(yss_true, self._recommend(test_users))
            if self._verbose:
                print("fold=%d iter=%2d: " % (fold, it + 1),
                      "TraLoss=%.4f lr=%.4f" % (aveloss, self._lr),
                      '\tTst:' + ' '.join([m + '=%.4f' % s for m, s in zip(self._eval_metrics, scores)]),
                      "\ttimecost=%.1f(s)" % (time.time() - t0))
                sys.stdout.flush()
            self._lr *= .98
        return scores

    def close(self):
        if self._engine is not None:
            self._engine.close()
            self._engine = None
