"""The native neighbourhood object (csrc/cf_knn.hip, ``cf_knn_*``) behind the
PopRank, UserCF, ItemCF and UserItemCF drop-ins, and the ``train`` the four
share (pop.py:46-62, usercf.py:68-87, itemcf.py:76-94, useritemcf.py:77-95)."""
import ctypes

import numpy as np
import scipy.sparse as sp

from . import _native as N
from ._native import _ptr
from ._model import parse_device
from .io_util import to_csr
from .ranking import evaluateCV, evaluateLOOV

KINDS = {"pop": N.CF_KNN_POP, "user": N.CF_KNN_USER, "item": N.CF_KNN_ITEM, "useritem": N.CF_KNN_USERITEM}
SIDES = {"user": 0, "item": 1}


def binary_csr(trasR):
    """The pattern-only CSR of a train matrix whose nonzeros are all 1 (what
    every reference driver passes: ``lil_matrix(matBinarize(...))``)."""
    data = sp.csr_matrix(trasR).data
    if data.size and not np.all((data == 1) | (data == 0)):
        raise ValueError("the neighbourhood models take a binarised trasR (nonzeros all 1); "
                         "weighted ratings are not supported")
    return to_csr(trasR)


class KnnEngine(N._NativeObject):
    """One HIP device's train CSR, its transpose, and the [n_side, topK]
    neighbour tables (ids, float32 similarities) the kind reads."""

    PREFIX = "cf_knn"

    def __init__(self, n_users, n_items, kind="user", topK=50, theta=0.5, device=0):
        if kind not in KINDS:
            raise ValueError("kind must be one of %s" % sorted(KINDS))
        self.n_users, self.n_items, self.topK = int(n_users), int(n_items), int(topK)
        self.kind = kind
        self._create(self.n_users, self.n_items, KINDS[kind], self.topK, float(theta), int(device))

    def _n_side(self, side):
        return self.n_users if SIDES[side] == 0 else self.n_items

    def set_option(self, name, value):
        self._call("set_option", name.encode(), int(value))

    def fit(self):
        self._call("fit")

    def get_neighbours(self, side):
        """(ids int32, sims float32), [n_side, topK] each: descending
        similarity, ties to the lower id, pads (-1, 0)."""
        shape = (self._n_side(side), self.topK)
        idx, sim = np.empty(shape, dtype=np.int32), np.empty(shape, dtype=np.float32)
        self._call("get_neighbours", SIDES[side], _ptr(idx, ctypes.c_int32), _ptr(sim, ctypes.c_float))
        return idx, sim

    def set_neighbours(self, side, idx, sim):
        shape = (self._n_side(side), self.topK)
        i = np.ascontiguousarray(idx, dtype=np.int32)
        s = np.ascontiguousarray(sim, dtype=np.float32)
        if i.shape != shape or s.shape != shape:
            raise ValueError("%s neighbour tables must be %s" % (side, shape))
        self._call("set_neighbours", SIDES[side], _ptr(i, ctypes.c_int32), _ptr(s, ctypes.c_float))

    def similarity(self, side, rows):
        """Dense float32 similarity rows [len(rows), n_side]."""
        r = np.ascontiguousarray(rows, dtype=np.int32)
        out = np.empty((r.shape[0], self._n_side(side)), dtype=np.float32)
        self._call("similarity", SIDES[side], _ptr(r, ctypes.c_int32), r.shape[0], _ptr(out, ctypes.c_float))
        return out

    def predict(self, users):
        """Dense float64 predictions [len(users), n_items]."""
        u = np.ascontiguousarray(users, dtype=np.int32)
        out = np.empty((u.shape[0], self.n_items), dtype=np.float64)
        self._call("predict", _ptr(u, ctypes.c_int32), u.shape[0], _ptr(out, ctypes.c_double))
        return out

    def score_topk(self, users, k, exclude_train=True, return_values=False):
        return self._score_topk(users, k, exclude_train, return_values)


class KnnModel(object):
    """``train(fold, trasR, tstsR)`` and ``close()`` of the four drop-ins; a
    subclass sets ``KIND`` and stores ``_topK`` / ``_theta``."""

    KIND = None
    _topK, _theta = 1, 0.0

    def _init_common(self, n_users, n_items, topN, split_method, eval_metrics, device):
        self._n_users, self._n_items = int(n_users), int(n_items)
        self._topN, self._split_method, self._eval_metrics = int(topN), split_method, list(eval_metrics)
        self._device = parse_device(device)
        self._engine = None

    @property
    def engine(self):
        return self._engine

    def _eval(self, yss_true, yss_pred):
        if self._split_method == 'cv':
            return evaluateCV(yss_true, yss_pred, self._eval_metrics, self._topN)
        if self._split_method == 'loov':
            return evaluateLOOV(yss_true, yss_pred, self._eval_metrics, self._topN)
        return None

    def train(self, fold, trasR, tstsR):
        indptr, indices, _ = binary_csr(trasR)
        t_indptr, t_indices, _ = to_csr(tstsR)
        test_users = list(set(np.asarray(tstsR.nonzero()[0])))
        yss_true = None
        if self._split_method == 'cv':
            yss_true = [set(t_indices[t_indptr[u]:t_indptr[u + 1]].tolist()) for u in test_users]
        elif self._split_method == 'loov':
            yss_true = [int(t_indices[t_indptr[u]]) for u in test_users]
        self.close()
        # no row has more positives than the longer side: a larger topK selects the same neighbours
        topK = min(int(self._topK), max(self._n_users, self._n_items))
        self._engine = eng = KnnEngine(self._n_users, self._n_items, self.KIND, topK, self._theta, self._device)
        eng.set_interactions(indptr, indices)
        eng.fit()
        idx = eng.score_topk(np.asarray(test_users, dtype=np.int32), self._topN, exclude_train=True)
        return self._eval(yss_true, [[int(x) for x in row if x >= 0] for row in idx])

    def close(self):
        if self._engine is not None:
            self._engine.close()
            self._engine = None
