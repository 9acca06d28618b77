"""Deterministic mode on the positive-sorted path (round 3).

With "deterministic" 1 and pos_sort active, a step runs the fast path's own
launches (draw with its atomic ranks, psort, grad_sort_kernel, the pos_sort
apply) and takes every sum of gradient rows in 64-bit fixed point: integer
adds are associative, so the sums do not depend on the order the atomic
ranks gave the occurrences or on which pairs share a gradient block.  The
positive partials are int64 rows (past the first 8 of an item: int64
atomics), duplicated users past their slot cap add with int64 atomics,
negatives' and users' slot rows are converted as they are summed, and the
per-pair losses add as integers.  Two runs from the same
state must be BITWISE identical (TF1's CPU UnsortedSegmentSum behind
AdagradOptimizer is deterministic, bprmf.py:83-88), and the result must match
the float64 oracle: every host-fed step from the engine's own pre-step tables
within the a-priori fp32 bound of oracle/fp32_bound.py (which covers the
2^-32 fixed-point terms), and the trajectory within 1e-6 + 1e-5 |ref| plus
the same bound carried over the steps (a Zipf-head item sums ~1,000 rows).
"""
import numpy as np
import pytest

from conftest import LocalStepCheck
from conftest import assert_close as _assert_close

pytestmark = pytest.mark.gpu

TABLES = ("user", "item", "acc_user", "acc_item")
HP = {"bpr": dict(reg=0.02), "amf": dict(reg=0.05, reg_adv=1.0)}


def assert_close(got, ref, name, rtol=1e-5, atol=1e-6, bound=None, max_excluded=0.0):
    """Elementwise |got - ref| <= atol + rtol |ref| (+ the carried a-priori
    fp32 bound where given; non-finite bounds only up to ``max_excluded``)."""
    return _assert_close(got, ref, name, rtol=rtol, atol=atol, bound=bound, max_excluded=max_excluded)


def _host_fed(e, B, n, ni, reg=0.02):
    """n host-fed steps on device-drawn batches: each step checked locally
    (conftest.LocalStepCheck, every element), the trajectory against the
    float64 oracle within the strict band plus the carried a-priori bound --
    finite on all but a few Zipf-head item elements after 3-4 steps (a CPU
    replay of these shapes: 0 of 128,000 at B = 8192 x 4, 4 of 256,000 at
    B = 32768 x 3), so at most 1 % may go unchecked (asserted)."""
    from oracle import fp32_bound as FB
    T = {t: e.get_table(t).astype(np.float64) for t in TABLES}
    E = FB.zero_bounds(T["user"], T["item"], acc_exact=True)
    local = LocalStepCheck(reg)
    hot = hot_user = 0
    for _ in range(n):
        pairs, negs, _ = e.sample(B)
        hot = max(hot, int(np.bincount(pairs[:, 1], minlength=ni).max()))
        hot_user = max(hot_user, int(np.bincount(pairs[:, 0]).max()))
        local.before(e)
        lg = e.step(pairs, negs)
        local.after(e, pairs, negs, lg)
        lo = FB.bpr_step_bounded(T["user"], T["item"], T["acc_user"], T["acc_item"], E, pairs, negs, reg)
        assert abs(lg - lo) <= 1e-5 * abs(lo), (lg, lo)
    for t in TABLES:
        assert_close(e.get_table(t), T[t], t, bound=E[t], max_excluded=0.01)
    return hot, hot_user


@pytest.fixture(scope="module")
def skewed_graph():
    from collaborativefilteringusingtensorflow_amd.engine import synth_graph
    return synth_graph(40_000, 4_000, 30.0, 0.8, 20261017, n_threads=8)


def _engine(model, graph, d, W, det, seed=17, slot_max=0):
    from collaborativefilteringusingtensorflow_amd.engine import Engine
    ip, ix = graph
    e = Engine(model, len(ip) - 1, 4_000, d, n_neg=W, seed=seed, **HP[model])
    e.set_option("deterministic", 1 if det else 0)
    e.set_option("pos_sort", 1)
    if slot_max:   # users past this many occurrences take the (int64) atomics
        e.set_option("slot_max_user", slot_max)
    e.set_interactions(ip, ix)
    e.init_params(0.0, 0.1, truncated=True, seed=3)
    if model == "amf":
        e.begin_phase(1)
    return e


def _run(model, graph, d, W, B, steps, det, slot_max=0):
    e = _engine(model, graph, d, W, det, slot_max=slot_max)
    _, path = e.step_path(B)
    assert path["pos_sort"] and path["deterministic"] == bool(det), path
    e.profile(True)
    loss = e.train_steps(B, steps)
    e.profile(False)
    assert e.profile_read("psort")[1] == steps
    out = {t: e.get_table(t) for t in TABLES}
    e.close()
    return loss, out


@pytest.mark.parametrize("model,d,W,slot_max", [("bpr", 64, 1, 0), ("bpr", 64, 1, 2), ("bpr", 32, 5, 0),
                                                  ("amf", 32, 5, 0)],
                         ids=["bpr-w1", "bpr-w1-user-atomics", "bpr-w5", "amf-adv-w5"])
def test_det_pos_sort_two_runs_bitwise_identical(skewed_graph, model, d, W, slot_max):
    a = _run(model, skewed_graph, d, W, 16384, 6, det=True, slot_max=slot_max)
    b = _run(model, skewed_graph, d, W, 16384, 6, det=True, slot_max=slot_max)
    assert a[0] == b[0]
    for t in TABLES:
        assert np.array_equal(a[1][t], b[1][t]), t
    # the fast pos_sort path trains the same model up to fp32 summation order
    c = _run(model, skewed_graph, d, W, 16384, 6, det=False, slot_max=slot_max)
    assert abs(c[0] - a[0]) <= 1e-5 * abs(a[0])
    for t in TABLES:
        assert_close(c[1][t], a[1][t].astype(np.float64), t, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("W,slot_max", [(1, 0), (5, 0), (1, 2)], ids=["w1", "w5", "w1-user-atomics"])
def test_det_pos_sort_matches_oracle(skewed_graph, W, slot_max):
    """Host-fed deterministic pos_sort steps on device-drawn batches whose Zipf
    head spans many 16-pair gradient blocks, against the float64 oracle
    (slot_max 2: users seen more than twice add their rows with int64 atomics)."""
    e = _engine("bpr", skewed_graph, 32, W, det=True, seed=23, slot_max=slot_max)
    e.profile(True)
    hot, hot_user = _host_fed(e, 8192, 4, 4_000)
    e.profile(False)
    assert e.profile_read("psort")[1] == 4
    assert hot >= 16 * 8   # a positive run past the 8 partial rows: int64 atomics (GV64)
    if slot_max:
        assert hot_user > slot_max, hot_user
    e.close()


def test_fast_pos_sort_hot_partials_match_oracle(skewed_graph):
    """The fast path with a Zipf-head item whose run spans dozens of
    gradient blocks: its first capP (8) partials in their compact rows
    (slotP[block + item]), the rest on float atomics; host-fed steps against
    the float64 oracle."""
    e = _engine("bpr", skewed_graph, 64, 1, det=False, seed=29)
    hot, _ = _host_fed(e, 32768, 3, 4_000)
    assert hot >= 16 * 32   # one run over >= 32 blocks, far past the 8 partial rows
    e.close()


@pytest.mark.parametrize("how", ["huge", "inf"])
def test_det_fixed_point_range_guard(skewed_graph, how):
    """A diverged item table (rows of 1e25, or inf) makes every duplicated
    item's gradient term leave the fixed-point range: the deterministic call
    fails with CF_ENUMERIC instead of leaving wrapped integers in the table
    (the fast path carries the inf / NaN into the tables, as TF1's fp32 path
    would).  The flag is cleared by the failing call: the engine steps again
    once the tables are valid."""
    from collaborativefilteringusingtensorflow_amd import _native as N
    e = _engine("bpr", skewed_graph, 32, 1, det=True, seed=31)
    V = e.get_table("item")
    bad = V.copy()
    bad[: 200] = 1e25 if how == "huge" else np.inf
    e.set_table("item", bad)
    pairs, negs, _ = e.sample(8192)
    with pytest.raises(N.NativeError, match="at step 0 .*CF_ENUMERIC"):
        e.step(pairs, negs)
    e.set_table("item", V)
    e.set_table("acc_item", np.full_like(V, 0.1))
    with pytest.raises(N.NativeError, match="at step 0 .*CF_ENUMERIC"):   # the call's first step
        e.set_table("item", bad)
        e.train_steps(8192, 2)
    e.set_table("item", V)
    e.set_table("acc_item", np.full_like(V, 0.1))
    e.init_params(0.0, 0.1, truncated=True, seed=3)
    loss = e.train_steps(8192, 2)          # valid again: no stale flag
    assert np.isfinite(loss)
    # the fast path takes the same state without an error and shows the divergence
    f = _engine("bpr", skewed_graph, 32, 1, det=False, seed=31)
    f.set_table("item", bad)
    f.step(pairs, negs)
    assert not np.isfinite(f.get_table("item")[:200]).all() or how == "huge"
    e.close()
    f.close()


@pytest.mark.parametrize("B,W", [(1 << 17, 1), (16384, 5)])
def test_user_runs_equal_atomic_ranks(skewed_graph, B, W):
    """Sorted batches take each user's rank and count from the batch's runs
    of consecutive pairs (StepArgs::user_runs) -- one non-returning atomic add
    of the run's length per run, a returning one only for the wave's first and
    last runs, which may continue in the neighbouring waves -- instead of one
    returning count atomic per pair.  The ranks are a different
    permutation, so in deterministic mode (order-free fixed-point sums) the
    training must be BITWISE the same with user_runs on and off; at
    B = 2^17 on 40K users a batch has ~3.3 pairs per user, so many runs cross
    the 16-pair wave boundaries.  The fast path trains the same model up to
    fp32 summation order."""
    out = {}
    for det in (1, 0):
        for ur in (0, 1):
            e = _engine("bpr", skewed_graph, 32, W, det=bool(det), seed=43)
            e.set_option("user_runs", ur)
            e.set_option("sorted_batches", 1)
            assert e.step_path(B)[1]["sorted_batches"]
            loss = e.train_steps(B, 5)
            out[det, ur] = (loss, {t: e.get_table(t) for t in TABLES})
            e.close()
    (l0, T0), (l1, T1) = out[1, 0], out[1, 1]
    assert l0 == l1
    for t in TABLES:
        assert np.array_equal(T0[t], T1[t]), t
    (l0, T0), (l1, T1) = out[0, 0], out[0, 1]
    assert abs(l1 - l0) <= 1e-5 * abs(l0)
    for t in TABLES:
        assert_close(T1[t], T0[t].astype(np.float64), t, rtol=1e-4, atol=1e-6)
