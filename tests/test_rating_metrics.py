"""The rating.py port against known answers computed by the reference's
src/metrics/rating.py (tests/golden/rating_cases.json)."""
import json
import os

import numpy as np

from conftest import GOLDEN
from collaborativefilteringusingtensorflow_amd import rating as R


def test_rating_cases():
    with open(os.path.join(GOLDEN, "rating_cases.json")) as f:
        cases = json.load(f)
    assert len(cases) >= 4
    for c in cases:
        yt = np.array(c["ys_true"])
        yp = np.array(c["ys_pred"], dtype=c["pred_dtype"])
        got = R.evaluate(yt, yp, c["metrics"])
        for m, g, w in zip(c["metrics"], got, c["scores"]):
            if w is None:
                assert g is None, (c["name"], m)
            else:
                assert abs(g - w) <= 1e-15 * abs(w), (c["name"], m, g, w)


def test_the_demo_case():
    yt, yp = np.array([2.5, 1.5, 0]), np.array([1, 2, 1])
    mae, mse, rmse = R.evaluate(yt, yp, ["mae", "mse", "rmse"])
    assert abs(mae - 1.0) <= 1e-15 and abs(mse - 7 / 6) <= 1e-15 and abs(rmse - np.sqrt(7 / 6)) <= 1e-15
    assert R.mean_absolute_error(yt, yp) == mae and R.root_mean_squared_error(yt, yp) == rmse


def test_scores_from_sums_is_the_same_expression():
    rng = np.random.RandomState(1)
    yt = rng.randint(1, 6, 50).astype(np.float64)
    yp = rng.rand(50).astype(np.float32) * 5
    ab, sq = np.sum(np.fabs(yt - yp)), np.sum(np.power(yt - yp, 2))
    assert R.scores_from_sums(50, ab, sq, ["rmse", "mae", "mse", "x"]) == R.evaluate(yt, yp, ["rmse", "mae", "mse", "x"])
