"""The native pointwise object (csrc/cf_pointwise.hip, ``cf_pw_*``) behind the
MF, SVD and WRMF drop-ins, and the host loop the two rating models share."""
import ctypes
import sys
import time

import numpy as np

from . import _native as N
from ._native import _ptr
from ._model import parse_device
from .rating import scores_from_sums

TABLES = {"user": 0, "item": 1, "kernel": 2, "acc_user": 3, "acc_item": 4, "acc_kernel": 5}
KINDS = {"mf": N.CF_PW_MF, "wrmf": N.CF_PW_MF, "svd": N.CF_PW_SVD}


def split_batch(batch):
    """A sampler_rating batch [B, 3] -> (ui int32 [B, 2], r float32 [B])."""
    b = np.asarray(batch)
    if b.ndim != 2 or b.shape[1] != 3:
        raise ValueError("a rating batch is [B, 3] (user, item, rating)")
    return np.ascontiguousarray(b[:, :2], dtype=np.int32), np.ascontiguousarray(b[:, 2], dtype=np.float32)


class PointwiseEngine(N._NativeObject):
    """One HIP device's tables U [n_users, d], V [n_items, d] (``kind="svd"``:
    and the kernel matrix K [d, d]) with their Adagrad accumulators."""

    PREFIX, TABLES = "cf_pw", TABLES

    def __init__(self, n_users, n_items, n_factors=10, kind="mf", weight=1.0, reg=0.02, lr=0.1,
                 acc_init=0.1, device=0):
        if kind not in KINDS:
            raise ValueError("kind must be one of %s" % sorted(KINDS))
        self.n_users, self.n_items, self.d = int(n_users), int(n_items), int(n_factors)
        self.kind = kind
        self._create(self.n_users, self.n_items, self.d, KINDS[kind], float(weight), float(reg), float(lr),
                     float(acc_init), int(device))

    def _shape(self, name):
        return {"user": (self.n_users, self.d), "item": (self.n_items, self.d), "kernel": (self.d, self.d),
                "acc_user": (self.n_users, self.d), "acc_item": (self.n_items, self.d),
                "acc_kernel": (self.d, self.d)}[name]

    def init_params(self, mean=0.0, stddev=0.1, seed=1, truncated=True):
        N.check(self._L.cf_pw_init_params(self._h, float(mean), float(stddev), int(bool(truncated)),
                                          int(seed) & 0xFFFFFFFFFFFFFFFF), "cf_pw_init_params")

    def step(self, ui, r, return_loss=True):
        p = np.ascontiguousarray(ui, dtype=np.int32)
        q = np.ascontiguousarray(r, dtype=np.float32)
        if p.ndim != 2 or p.shape[1] != 2 or q.shape != (p.shape[0],):
            raise ValueError("ui must be [B, 2] and r [B]")
        loss = ctypes.c_double(0.0)
        N.check(self._L.cf_pw_step(self._h, _ptr(p, ctypes.c_int32), _ptr(q, ctypes.c_float), p.shape[0],
                                   ctypes.byref(loss) if return_loss else None), "cf_pw_step")
        return float(loss.value) if return_loss else None

    def eval(self, ui, r, lo, hi, return_pred=True):
        """(pred float32 [n] or None, sum |r - pred|, sum (r - pred)^2)."""
        p = np.ascontiguousarray(ui, dtype=np.int32).reshape(-1, 2)
        q = np.ascontiguousarray(r, dtype=np.float32)
        if q.shape != (p.shape[0],):
            raise ValueError("ui must be [n, 2] and r [n]")
        pred = np.empty(p.shape[0], dtype=np.float32) if return_pred else None
        sums = (ctypes.c_double * 2)(0.0, 0.0)
        N.check(self._L.cf_pw_eval(self._h, _ptr(p, ctypes.c_int32), _ptr(q, ctypes.c_float), p.shape[0],
                                   float(lo), float(hi),
                                   _ptr(pred, ctypes.c_float) if pred is not None else None, sums), "cf_pw_eval")
        return pred, float(sums[0]), float(sums[1])

    def score_topk(self, users, k, exclude_train=True, return_values=False):
        return self._score_topk(users, k, exclude_train, return_values)


class RatingModel(object):
    """The constructor and ``train`` of mf.py:11-116 and svd.py:11-119."""

    KIND = "mf"

    def __init__(self, n_users, n_items, eval_metrics=['rmse', 'mae'], range_of_ratings=(.5, 5), reg=0.02,
                 n_factors=10, batch_size=500, max_iter=50, lr=.1, init_mean=0.0, init_stddev=0.1,
                 device='CPU', seed=None, verbose=True):
        self._n_users, self._n_items, self._eval_metrics = int(n_users), int(n_items), list(eval_metrics)
        self._range_of_ratings, self._reg = tuple(range_of_ratings), float(reg)
        self._n_factors, self._batch_size = int(n_factors), int(batch_size)
        self._max_iter, self._lr = int(max_iter), float(lr)
        self._train_lr = float(lr)   # the optimizer is built once with the initial lr (mf.py:73, 89)
        self._init_mean, self._init_stddev = float(init_mean), float(init_stddev)
        self._device = parse_device(device)
        self._seed = seed
        self._verbose = verbose
        self._engine = None
        self._init_tables = None

    @property
    def engine(self):
        return self._engine

    def set_initial_tables(self, **tables):
        """Start the next ``train`` from these tables (user, item, kernel)
        instead of the seeded truncated-normal initializer."""
        t = {n: np.asarray(a, dtype=np.float32) for n, a in tables.items() if a is not None}
        self._init_tables = t or None

    def _eval(self, tst_tuple):
        tst = np.asarray(tst_tuple)
        lo, hi = self._range_of_ratings
        _, ab, sq = self._engine.eval(tst[:, :2], tst[:, 2], lo, hi, return_pred=False)
        return scores_from_sums(tst.shape[0], ab, sq, self._eval_metrics)

    def train(self, fold, tra_tuple, tst_tuple, sampler):
        n_batches = int(len(tra_tuple) / self._batch_size)   # mf.py:92
        if self._engine is not None:
            self._engine.close()
        self._engine = eng = PointwiseEngine(self._n_users, self._n_items, self._n_factors, kind=self.KIND,
                                             reg=self._reg, lr=self._train_lr, device=self._device)
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
                ui, r = draw() if draw is not None else split_batch(sampler.next_batch())   # mf.py:98-100
                eng.step(ui, r, return_loss=False)
            aveloss = eng.take_loss() / max(n_batches, 1)
            scores = self._eval(tst_tuple)
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
