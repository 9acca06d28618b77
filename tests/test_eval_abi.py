"""The device-metric entry points at the C-ABI boundary, without a GPU: the
header declares them, the metric columns are the ones ranking.py names, and
ranking.scores_from_sums scales each column as evaluateCV / evaluateLOOV do."""
import re

from collaborativefilteringusingtensorflow_amd import _native as N
from collaborativefilteringusingtensorflow_amd import ranking


def _header():
    with open(N.HEADER_PATH) as f:
        return f.read()


def test_header_declares_the_metric_entry_points():
    syms = N.header_symbols()
    for name in ("cf_set_truth", "cf_eval_lists", "cf_evaluate"):
        assert name in syms, name
        assert name in N.SIGNATURES, name
        assert hasattr(N.lib(), name), name
    text = _header()
    assert re.search(r"CF_EVAL_N\s*=\s*7\b", text)
    assert re.search(r"CF_K_METRICS\s*=\s*15\b", text) and re.search(r"CF_K_COUNT\s*=\s*16\b", text)
    assert N.KERNELS["metrics"] == 15


def test_enum_order_is_device_columns():
    text = _header()
    assert ranking.DEVICE_COLUMNS == ("pre", "recall", "ndcg", "map", "mrr", "hr", "arhr")
    for col, name in enumerate(ranking.DEVICE_COLUMNS):
        m = re.search(r"CF_EVAL_%s\s*=\s*(\d+)" % name.upper(), text)
        assert m and int(m.group(1)) == col, name


def test_scores_from_sums_columns_and_scaling():
    row = [3.0, 5.0, 7.0, 11.0, 13.0, 17.0, 19.0]
    n = 4
    cv = ranking.scores_from_sums(row, n, ["pre", "recall", "ndcg", "map", "mrr", "hr", "bogus"], "cv")
    assert cv == [3.0 / 4, 5.0 / 4, 7.0 / 4, 11.0 / 4, 13.0 / 4, None, None]    # means; hr is not a CV metric
    lo = ranking.scores_from_sums(row, n, ["hr", "arhr", "pre", "bogus"], "loov")
    assert lo == [17.0, 19.0, None, None]                                        # sums, as hr_k_score returns
    assert ranking.scores_from_sums(row, n, ["pre", "hr"], "other") == [None, None]
    # the same None pattern as the host functions give
    assert [s is None for s in cv] == [s is None for s in ranking.evaluateCV(
        [{1}], [[1]], ["pre", "recall", "ndcg", "map", "mrr", "hr", "bogus"], 1)]
    assert [s is None for s in lo] == [s is None for s in ranking.evaluateLOOV(
        [1], [[1]], ["hr", "arhr", "pre", "bogus"], 1)]
