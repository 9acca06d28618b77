"""SVD drop-in (src/models/basic/models/svd.py:11-119): MF with a trained
dense kernel matrix K [d, d] between the factors, pred = <U_u K, V_i>
(svd.py:65-71).  K is truncated-normal like U and V (svd.py:29-31), is not
regularised (svd.py:50-54) and takes a dense Adagrad update every step
(svd.py:76).  Loss, optimizer, evaluation and ``train`` are mf.py's.

The products U_b K and V_b K^T run on the f32-input MFMA of gfx950 and the
gradient of K on the f64 MFMA with fp64 block partials
(csrc/cf_pointwise.hip).
"""
from ._pointwise import PointwiseEngine, RatingModel  # noqa: F401

__all__ = ["SVD", "PointwiseEngine"]


class SVD(RatingModel):
    KIND = "svd"
