"""Rating metrics: drop-in for ``src/metrics/rating.py`` (MAE, MSE, RMSE and
``evaluate``), with the reference's expression order -- ``1 / n * sum(...)``,
the power as ``np.power(., 2)`` -- so float32 predictions against float64
ratings give the same float64 scores (rating.py:4-29)."""
import numpy as np


def mean_absolute_error(ys_true, ys_pred):
    return 1 / ys_true.shape[0] * np.sum(np.fabs(ys_true - ys_pred))


def mean_squared_error(ys_true, ys_pred):
    return 1 / ys_true.shape[0] * np.sum(np.power(ys_true - ys_pred, 2))


def root_mean_squared_error(ys_true, ys_pred):
    return np.sqrt(1 / ys_true.shape[0] * np.sum(np.power(ys_true - ys_pred, 2)))


_SCORES = {'mae': mean_absolute_error, 'mse': mean_squared_error, 'rmse': root_mean_squared_error}


def evaluate(ys_true, ys_pred, eval_metrics):
    """One score per name; an unknown name scores None (rating.py:27-28)."""
    return [_SCORES[m](ys_true, ys_pred) if m in _SCORES else None for m in eval_metrics]


def scores_from_sums(n, abs_sum, sq_sum, eval_metrics):
    """The same scores from the two fp64 sums of ``cf_pw_eval``."""
    out = []
    for m in eval_metrics:
        if m == 'mae':
            out.append(1 / n * abs_sum)
        elif m == 'mse':
            out.append(1 / n * sq_sum)
        elif m == 'rmse':
            out.append(np.sqrt(1 / n * sq_sum))
        else:
            out.append(None)
    return out
