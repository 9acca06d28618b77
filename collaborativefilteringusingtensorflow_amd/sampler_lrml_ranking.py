"""Drop-in for ``src/samplers/sampler_lrml_ranking.py``: ``next_batch()``
returns ``(pos_useritem_batch, neg_useritem_batch)``, two ``[B,2]`` int64
arrays of (user, item) rows.  Per epoch the nnz pairs are shuffled once and
sliced into ``int(nnz / B)`` batches; each row's negative pair is
``randint(0, n_users, 1)[0]``, ``randint(0, n_items, 1)[0]``, both redrawn
while ``trasR[u, i] > 0`` (sampler_lrml_ranking.py:20-35).

Both classes run that stream on the native MT19937 restatement
(cf_mt_sampler kind 3, csrc/cf_mt_sampler.cpp): no thread, no queue.
``ExactSampler(seed=s)`` is the reference's stream for ``np.random.seed(s)``
set right before its ``Sampler`` is built; ``Sampler`` seeds itself from the
OS when ``seed`` is None, as the reference never seeds.
"""
import ctypes
import os

import numpy as np

from . import _native as N
from ._sampler import MTSampler


class ExactSampler(MTSampler):
    KIND = 3

    def __init__(self, trasR, batch_size=1000, n_workers=1, seed=0):
        super(ExactSampler, self).__init__(trasR, n_neg=1, batch_size=batch_size, gsize=0, seed=seed)
        self.n_workers = n_workers  # accepted for signature parity; the host stream needs no threads

    def _draw(self):
        # kind 3 writes the negative (user, item) pairs [B, 2] into negs
        pos = np.empty((self.batch_size, 2), dtype=np.int32)
        neg = np.empty((self.batch_size, 2), dtype=np.int32)
        P = ctypes.POINTER(ctypes.c_int32)
        N.check(self._L.cf_mt_sampler_next(self._h, pos.ctypes.data_as(P), neg.ctypes.data_as(P), None),
                "cf_mt_sampler_next")
        return pos, neg

    def next_batch(self):
        pos, neg = self._draw()
        return pos.astype(np.int64), neg.astype(np.int64)


class Sampler(ExactSampler):
    def __init__(self, trasR, batch_size=1000, n_workers=1, seed=None):
        if seed is None:
            seed = int.from_bytes(os.urandom(4), "little")
        super(Sampler, self).__init__(trasR, batch_size=batch_size, n_workers=n_workers, seed=seed)
