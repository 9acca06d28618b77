"""MF drop-in (src/models/basic/models/mf.py:11-116): pred = <U_u, V_i> on
raw ratings, loss 1/2 sum (pred - r)^2 + reg 1/2 (sum |U_u|^2 + sum |V_i|^2)
over the batch rows (mf.py:47-68), sparse Adagrad with TF1's duplicate-row
sum, evaluated as clip_by_value(pred, lo, hi) against the test tuples with
metrics/rating.py (mf.py:77-80).

The arithmetic runs in the native pointwise object (csrc/cf_pointwise.hip,
``cf_pw_*``); ``MF.train(fold, tra_tuple, tst_tuple, sampler)`` is the host
loop of mf.py:83-113: ``int(len(tra_tuple) / batch_size)`` host-fed steps per
epoch, the mean pre-update batch loss, one evaluate pass (``cf_pw_eval``) and
the log line.  The ``lr *= .98`` there is cosmetic: the optimizer was built
with the initial lr.
"""
from ._pointwise import PointwiseEngine, RatingModel  # noqa: F401

__all__ = ["MF", "PointwiseEngine"]


class MF(RatingModel):
    KIND = "mf"
