"""LRML drop-in (src/models/others/models/lrml.py:11-202): latent relational
metric learning, trained on ``sampler_lrml_ranking`` batches of positive and
negative (user, item) pairs.

The arithmetic -- the memory attention a = softmax((U_u o V_i)^T Key), the
relation r = a^T Mem, the hinge on |U_u + r - V_i|^2 + margin -
|U_u' + r - V_i'|^2 (lrml.py:59-80), sparse Adagrad on U and V with TF1's
duplicate-row sum, the clip of every row to ``clip_norm`` (lrml.py:106-116)
and the recommend scores (lrml.py:86-104) -- runs in the native LRML object
(csrc/cf_lrml.hip, ``cf_lrml_*``); this module is the host loop.

``LRML.train(fold, trasR, tstsR, sampler)`` follows lrml.py:150-199:
``5 * int(nnz / batch_size)`` host-fed steps per epoch, the mean pre-update
batch loss, one recommend + evaluate pass and the log line.  The
``lr *= .98`` there is cosmetic: the optimizer was built with the initial lr.

``predict_mode="reference"`` (default) scores as lrml.py:95-100 is written:
the elementwise product with Key^T and a softmax over the *factor* axis per
memory slot -- not the training attention.  ``predict_mode="train"`` scores
with the step's own a and r (optional, not a parity target).
"""
import ctypes
import sys
import time

import numpy as np

from . import _native as N
from ._native import _ptr
from ._model import parse_device
from .io_util import to_csr
from .ranking import evaluateCV, evaluateLOOV

TABLES = {"user": 0, "item": 1, "key": 2, "memory": 3, "acc_user": 4, "acc_item": 5}


class LRMLEngine(N._NativeObject):
    """One HIP device's LRML tables U [n_users, d], V [n_items, d], Key [d, M],
    Mem [M, d] and the Adagrad accumulators of U and V."""

    PREFIX, TABLES = "cf_lrml", TABLES

    def __init__(self, n_users, n_items, n_factors=50, n_memory=20, margin=0.2, clip_norm=1.0,
                 lr=0.01, acc_init=0.1, device=0):
        self.n_users, self.n_items = int(n_users), int(n_items)
        self.d, self.M = int(n_factors), int(n_memory)
        self._create(self.n_users, self.n_items, self.d, self.M, float(margin), float(clip_norm), float(lr),
                     float(acc_init), int(device))

    def _shape(self, name):
        return {"user": (self.n_users, self.d), "item": (self.n_items, self.d),
                "key": (self.d, self.M), "memory": (self.M, self.d),
                "acc_user": (self.n_users, self.d), "acc_item": (self.n_items, self.d)}[name]

    def init_params(self, mean=0.0, stddev=0.01, seed=1):
        N.check(self._L.cf_lrml_init_params(self._h, float(mean), float(stddev),
                                            int(seed) & 0xFFFFFFFFFFFFFFFF), "cf_lrml_init_params")

    def step(self, pos, neg, return_loss=True):
        p = np.ascontiguousarray(pos, dtype=np.int32)
        q = np.ascontiguousarray(neg, dtype=np.int32)
        if p.ndim != 2 or p.shape[1] != 2 or q.shape != p.shape:
            raise ValueError("pos and neg must both be [B, 2]")
        loss = ctypes.c_double(0.0)
        N.check(self._L.cf_lrml_step(self._h, _ptr(p, ctypes.c_int32), _ptr(q, ctypes.c_int32),
                                     p.shape[0], ctypes.byref(loss) if return_loss else None),
                "cf_lrml_step")
        return float(loss.value) if return_loss else None

    def score_topk(self, users, k, exclude_train=True, predict_mode="reference", return_values=False):
        if predict_mode not in N.LRML_MODES:
            raise ValueError("predict_mode must be one of %s" % sorted(N.LRML_MODES))
        return self._score_topk(users, k, exclude_train, return_values, N.LRML_MODES[predict_mode])


class LRML(object):
    def __init__(self, n_users, n_items, topN=5, split_method='cv',
                 eval_metrics=['pre', 'recall', 'mrr', 'ndcg'], n_memory=20, margin=.2, clip_norm=1.0,
                 n_factors=50, batch_size=100, max_iter=50, lr=0.01, init_mean=0.0, init_stddev=0.01,
                 device='CPU', seed=None, verbose=True, predict_mode="reference"):
        if predict_mode not in N.LRML_MODES:
            raise ValueError("predict_mode must be one of %s, got %r" % (sorted(N.LRML_MODES), predict_mode))
        self._n_users, self._n_items, self._topN = int(n_users), int(n_items), int(topN)
        self._split_method, self._eval_metrics = split_method, list(eval_metrics)
        self._n_memory, self._margin, self._clip_norm = int(n_memory), float(margin), float(clip_norm)
        self._n_factors, self._batch_size = int(n_factors), int(batch_size)
        self._max_iter, self._lr = int(max_iter), float(lr)
        self._train_lr = float(lr)
        self._init_mean, self._init_stddev = float(init_mean), float(init_stddev)
        self._device = parse_device(device)
        self._seed = seed
        self._verbose = verbose
        self._predict_mode = predict_mode
        self._engine = None
        self._init_tables = None

    @property
    def engine(self):
        return self._engine

    def set_initial_tables(self, user=None, item=None, key=None, memory=None):
        """Start the next ``train`` from these tables instead of the seeded
        random-normal initializer (the reference's is unseeded)."""
        t = {n: np.asarray(a, dtype=np.float32)
             for n, a in (("user", user), ("item", item), ("key", key), ("memory", memory)) if a is not None}
        self._init_tables = t or None

    def _recommend(self, test_users):
        idx = self._engine.score_topk(np.asarray(test_users, dtype=np.int32), self._topN,
                                      exclude_train=True, predict_mode=self._predict_mode)
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
        n_batches = 5 * int(indices.shape[0] / self._batch_size)   # lrml.py:175
        if self._engine is not None:
            self._engine.close()
        self._engine = eng = LRMLEngine(self._n_users, self._n_items, self._n_factors, self._n_memory,
                                        margin=self._margin, clip_norm=self._clip_norm,
                                        lr=self._train_lr, device=self._device)
        eng.set_interactions(indptr, indices)
        seed = self._seed if self._seed is not None else 1
        eng.init_params(self._init_mean, self._init_stddev, seed=seed ^ 0x1234567)
        if self._init_tables is not None:
            for name, arr in self._init_tables.items():
                eng.set_table(name, arr)
        scores = None
        for it in range(self._max_iter):
            t0 = time.time()
            for _ in range(n_batches):
                pos, neg = sampler.next_batch()   # lrml.py:181-183
                eng.step(pos, neg, return_loss=False)
            aveloss = eng.take_loss() / max(n_batches, 1)
            scores = self._eval(yss_true, self._recommend(test_users))
            if self._verbose:
                print("%s_fold=%d iter=%2d: " % (self._split_method, fold, it + 1),
                      "TraLoss=%.4f lr=%.4f" % (aveloss, self._lr),
                      '\tTst@' + str(self._topN) + ':' + ' '.join(
                          [m + '=%.4f' % s for m, s in zip(self._eval_metrics, scores)]),
                      "\ttimecost=%.1f(s)" % (time.time() - t0))
                sys.stdout.flush()
            self._lr *= .98
        return scores

    def close(self):
        if self._engine is not None:
            self._engine.close()
            self._engine = None
