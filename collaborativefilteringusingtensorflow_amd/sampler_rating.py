"""Drop-in for ``src/samplers/sampler_rating.py``: ``next_batch()`` returns one
float64 ``[B', 3]`` array of (user, item, rating) rows, ``B' = B +
int(B * negRatio)``.

The reference never shuffles the epoch (sampler_rating.py:22-39): batch k is
rows ``[kB, (k+1)B)`` of the tuples in ``trasR.nonzero()`` order, ``int(nnz /
B)`` batches per epoch.  With ``negRatio = 0`` the batch is a view that
``np.random.shuffle`` permutes in place, so the order inside a slice persists
into the next epoch and the trailing ``nnz % B`` tuples are never trained.
With negatives, each is ``randint(0, n_users)``, ``randint(0, n_items)`` with
only the item redrawn while it is a train item of the user; the rows
``[user, item, 0]`` are appended and the whole batch shuffled.

Both classes run that stream on the native MT19937 restatement
(cf_rating_sampler, csrc/cf_mt_sampler.cpp): no thread, no queue.
``ExactSampler(seed=s)`` is the reference's stream for ``np.random.seed(s)``
set right before its ``Sampler`` is built; ``Sampler`` seeds itself from the
OS, as the reference never seeds.
"""
import ctypes
import os

import numpy as np
import scipy.sparse as sp

from . import _native as N


class ExactSampler(object):
    def __init__(self, trasR, negRatio=.0, batch_size=500, n_workers=1, seed=0):
        csr = sp.csr_matrix(trasR, dtype=np.float64)
        csr.sum_duplicates()
        csr.eliminate_zeros()
        csr.sort_indices()
        self.n_users, self.n_items = int(csr.shape[0]), int(csr.shape[1])
        self.batch_size, self.negRatio = int(batch_size), negRatio
        self.n_workers = n_workers  # accepted for signature parity; the host stream needs no threads
        self.n_rows = self.batch_size + int(self.batch_size * negRatio)
        if not 0 <= int(seed) < 2 ** 32:
            raise ValueError("Seed must be between 0 and 2**32 - 1")  # np.random.seed's rule
        self._L = N.lib()
        self._h = ctypes.c_void_p()
        ip = np.ascontiguousarray(csr.indptr, dtype=np.int64)
        ix = np.ascontiguousarray(csr.indices, dtype=np.int32)
        v = np.ascontiguousarray(csr.data, dtype=np.float64)
        N.check(self._L.cf_rating_sampler_create(
            ip.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), ix.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
            v.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), self.n_users, self.n_items, float(negRatio),
            self.batch_size, int(seed), ctypes.byref(self._h)), "cf_rating_sampler_create")

    def _draw(self):
        """(ui int32 [B', 2], r float32 [B']): the engine's own input types."""
        ui = np.empty((self.n_rows, 2), dtype=np.int32)
        r = np.empty(self.n_rows, dtype=np.float32)
        N.check(self._L.cf_rating_sampler_next(self._h, ui.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                               r.ctypes.data_as(ctypes.POINTER(ctypes.c_float))),
                "cf_rating_sampler_next")
        return ui, r

    def next_batch(self):
        ui, r = self._draw()
        out = np.empty((self.n_rows, 3), dtype=np.float64)
        out[:, :2] = ui
        out[:, 2] = r
        return out

    def state(self):
        e, b = ctypes.c_int64(0), ctypes.c_int64(0)
        N.check(self._L.cf_rating_sampler_state(self._h, ctypes.byref(e), ctypes.byref(b)),
                "cf_rating_sampler_state")
        return int(e.value), int(b.value)

    def close(self):
        if self._h:
            self._L.cf_rating_sampler_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Sampler(ExactSampler):
    def __init__(self, trasR, negRatio=.0, batch_size=500, n_workers=1, seed=None):
        if seed is None:
            seed = int.from_bytes(os.urandom(4), "little")
        super(Sampler, self).__init__(trasR, negRatio, batch_size, n_workers, seed=seed)
