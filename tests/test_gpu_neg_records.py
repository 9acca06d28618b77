"""Negatives drawn in the epoch-order pass (cf_set_option "neg_records").

Where the option applies, the counting scatter writes each record as
(u, i, j, 0) with j the negative the step's row-scan draw would take at that
slot, and the step's draw only loads and counts the record.  The batches are
the same bit for bit, so every comparison is ``np.array_equal`` on ids (or on
the tables of deterministic-mode training runs): ``neg_records`` 0 against 1,
and both against the host model (tests/sampler_model.py).

Sections:
  1. ml-100k fold 1, two whole epochs and the start of a third;
  2. rejection down to 1 / 64 and rows longer than a 2,048-pair tile;
  3. every launch that hosts a draw, in training;
  4. state jumps, a second graph, a new B;
  5. the configurations that keep the row-scan draw.
"""
import numpy as np
import pytest

import sampler_model as SM
from conftest import assert_close
from oracle import cf_oracle as O

pytestmark = pytest.mark.gpu


def engine(ip, ix, ni, model="bpr", W=1, G=1, seed=1, d=4, **opts):
    from collaborativefilteringusingtensorflow_amd.engine import Engine
    e = Engine(model, len(ip) - 1, ni, d, n_neg=W, gsize=G, seed=seed)
    for k, v in opts.items():
        e.set_option(k, v)
    e.set_interactions(ip, ix)
    return e


def same(got, ref, what):
    assert np.array_equal(got[0], ref[0]), ("pairs", what)
    assert np.array_equal(got[1], ref[1]), ("negatives", what)
    assert (got[2] is None) == (ref[2] is None), what
    if ref[2] is not None:
        assert np.array_equal(got[2], ref[2]), ("groups", what)


def flag(e, B):
    return e.step_path(B)[1]["neg_records"]


def pair_of(ip, ix, ni, B, **kw):
    """(row-scan engine, record engine) on one graph; the second takes the new path."""
    off = engine(ip, ix, ni, sorted_batches=1, neg_records=0, **kw)
    on = engine(ip, ix, ni, sorted_batches=1, neg_records=1, **kw)
    assert not flag(off, B) and flag(on, B)
    return off, on


def fold(fold1):
    return fold1["train_indptr"], fold1["train_indices"], int(fold1["n_items"])


# ---------------------------------------------------------------------------
# 1. the same batches as the row-scan draw, and as the model
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("B", [100, 997, 4096])
def test_batches_equal_row_scan_and_model(fold1, B):
    ip, ix, ni = fold(fold1)
    per = len(ix) // B
    off, on = pair_of(ip, ix, ni, B, seed=B)
    m = SM.Model(ip, ix, ni, 1, 0, B, sorted=True)
    ref = m.sample_many(B, 2 * per + 1)
    for b, r in enumerate(ref):
        got = on.sample(B)
        same(got, r, ("model", B, b))
        same(got, off.sample(B), ("row scan", B, b))
    assert on.sampler_state() == off.sampler_state() == m.state() == (2, 1)
    assert flag(on, B)
    off.close()
    on.close()


# ---------------------------------------------------------------------------
# 2. rejection and tile edges
# ---------------------------------------------------------------------------
def rejecting_graph():
    """200 users x 64 items, row lengths cycling 1, 2, 31, 62, 63: a 63-id row
    accepts one candidate in 64.  6,360 pairs, four tiles."""
    rng = np.random.RandomState(11)
    lens = [(1, 2, 31, 62, 63)[u % 5] for u in range(200)]
    rows = [np.sort(rng.choice(64, size=n, replace=False)) for n in lens]
    ip, ix = SM.csr_from_rows(rows)
    assert len(ix) == 40 * 159
    return ip, ix, 64


def long_row_graph():
    """8 users x 8,192 items, rows of 3,000 to 5,000 ids: every row crosses
    one or two edges of the 2,048-pair tiles."""
    rng = np.random.RandomState(12)
    rows = [np.sort(rng.choice(8192, size=rng.randint(3000, 5001), replace=False)) for _ in range(8)]
    ip, ix = SM.csr_from_rows(rows)
    return ip, ix, 8192


@pytest.mark.parametrize("graph,B", [("rejecting", 64), ("rejecting", 257), ("long-rows", 257)])
def test_rejection_and_tile_edges(graph, B):
    ip, ix, ni = rejecting_graph() if graph == "rejecting" else long_row_graph()
    per = len(ix) // B
    off, on = pair_of(ip, ix, ni, B, seed=3)
    for b in range(per + 2):
        got, ref = on.sample(B), off.sample(B)
        same(got, ref, (graph, B, b))
        for (u, _i), j in zip(got[0], got[1][:, 0]):
            assert j not in ix[ip[u]:ip[u + 1]]
    off.close()
    on.close()


# ---------------------------------------------------------------------------
# 3. every launch that hosts a draw
# ---------------------------------------------------------------------------
HOSTS = {"stepwise": {"pipeline": 0}, "apply": {"pipeline": 1}, "grad": {"pipeline": 2}, "both": {"pipeline": 3},
         "side-stream": {"pipeline": 0, "prep_stream": 1}}
TABLES = ("user", "item", "acc_user", "acc_item")


def trainer(fold1, opts, neg_records, det, d=16):
    from collaborativefilteringusingtensorflow_amd.engine import Engine
    ip, ix, ni = fold(fold1)
    e = Engine("bpr", len(ip) - 1, ni, d, n_neg=1, reg=0.05, seed=21)
    for k, v in opts.items():
        e.set_option(k, v)
    e.set_option("sorted_batches", 1)
    e.set_option("neg_records", neg_records)
    if det:
        e.set_option("deterministic", 1)
    e.set_interactions(ip, ix)
    return e


@pytest.mark.parametrize("pos_sort", [0, 1])
@pytest.mark.parametrize("host", list(HOSTS))
def test_training_equal_in_every_host_launch(fold1, host, pos_sort):
    """Deterministic sums are order-free, so equal batches give bitwise equal
    tables after two epochs and a step; then one step of the default mode
    against the float64 oracle."""
    B = 4096
    opts = dict(HOSTS[host], item_slots=0, pos_sort=pos_sort)
    per = len(fold1["train_indices"]) // B
    got = []
    for nr in (0, 1):
        e = trainer(fold1, opts, nr, det=True)
        e.init_params(0.0, 0.1, seed=5)
        path = e.step_path(B)[1]
        # (the draw inside the gradient launch, pipeline 2, runs without the positive sort)
        sort = bool(pos_sort) and opts["pipeline"] != 2
        assert path["neg_records"] == bool(nr) and path["pos_sort"] == sort, path
        e.train_steps(B, 2 * per + 1)
        assert e.sampler_state() == (2, 1)
        got.append({t: e.get_table(t) for t in TABLES})
        e.close()
    for t in TABLES:
        assert np.array_equal(got[0][t], got[1][t]), (t, host, pos_sort)
    # the default mode: the first step, on the batch the row-scan draw returns
    rng = np.random.RandomState(4)
    U = O.init_table(rng, (int(fold1["n_users"]), 16))
    V = O.init_table(rng, (int(fold1["n_items"]), 16))
    peek = trainer(fold1, opts, 0, det=False)
    pairs, negs, _ = peek.sample(B)
    peek.close()
    e = trainer(fold1, opts, 1, det=False)
    e.set_table("user", U)
    e.set_table("item", V)
    assert e.step_path(B)[1]["neg_records"]
    loss = e.train_steps(B, 1)
    U64, V64 = U.astype(np.float64), V.astype(np.float64)
    AU, AV = np.full_like(U64, 0.1), np.full_like(V64, 0.1)
    lo = O.bpr_step(U64, V64, AU, AV, pairs, negs, 0.05)
    assert abs(loss - lo) <= 1e-5 * abs(lo) + 1e-6, (loss, lo)
    for t, o in zip(TABLES, (U64, V64, AU, AV)):
        assert_close(e.get_table(t), o, (t, host, pos_sort))
    e.close()


# ---------------------------------------------------------------------------
# 4. state changes
# ---------------------------------------------------------------------------
def test_state_changes(fold1):
    ip, ix, ni = fold(fold1)
    B = 997
    off, on = pair_of(ip, ix, ni, B, seed=8)
    m = SM.Model(ip, ix, ni, 1, 0, 8, sorted=True)

    def draw(n, B, what, model=m):
        for b in range(n):
            got = on.sample(B)
            same(got, off.sample(B), (what, b))
            if model is not None:
                same(got, model.sample(B), (what, b, "model"))
        assert on.sampler_state() == off.sampler_state()

    draw(3, B, "start")
    for e in (off, on):
        e.set_sampler_state(6, 11)      # a later epoch, mid-epoch: neither cached order is its
    m.set_state(6, 11)
    draw(3, B, "after the jump")
    draw(3, 500, "B changed mid-epoch")
    assert m.state() == on.sampler_state() == (7, 3)
    nu2 = 400                           # a second, smaller graph: the other users lose their rows
    ip2 = np.concatenate([ip[:nu2 + 1], np.full(len(ip) - 1 - nu2, ip[nu2])]).astype(np.int64)
    ix2 = ix[:ip[nu2]]
    for e in (off, on):
        e.set_interactions(ip2, ix2)
    assert flag(on, 500) and not flag(off, 500)
    m2 = SM.Model(ip2, ix2, ni, 1, 0, 8, sorted=True)
    m2.set_state(*on.sampler_state())
    draw(len(ix2) // 500 + 2, 500, "second graph", m2)
    off.close()
    on.close()


# ---------------------------------------------------------------------------
# 5. fallbacks
# ---------------------------------------------------------------------------
FALLBACKS = {
    "W5": dict(W=5),
    "gbpr": dict(model="gbpr", G=2),
    "set-probe": dict(neg_check=1),
    "index-form": dict(sorted_batches=3),
    "radix-sort": dict(epoch_sort=1),
    "user-runs": dict(user_runs=1),
    "spec-neg": dict(item_slots=0, pos_sort=1, spec_neg=1),
}


@pytest.mark.parametrize("case", list(FALLBACKS))
def test_fallbacks_keep_the_row_scan_draw(fold1, case):
    ip, ix, ni = fold(fold1)
    B = 997
    kw = dict(sorted_batches=1)
    kw.update(FALLBACKS[case])
    off = engine(ip, ix, ni, seed=13, neg_records=0, **kw)
    on = engine(ip, ix, ni, seed=13, neg_records=1, **kw)
    assert not flag(on, B) and not flag(off, B)
    for b in range(3):
        same(on.sample(B), off.sample(B), (case, b))
    off.close()
    on.close()


def test_flag_set_when_every_condition_holds(fold1):
    ip, ix, ni = fold(fold1)
    e = engine(ip, ix, ni, sorted_batches=1)          # neg_records: the default
    auto = flag(e, 997)
    e.set_option("neg_records", 1)
    assert flag(e, 997)
    assert len(ix) // 40 + 1 > 1024
    assert not flag(e, 40)                            # 1,107 bins: past the counting sort
    e.set_option("neg_records", 0)
    assert not flag(e, 997)
    e.set_option("neg_records", 2)
    assert flag(e, 997) == auto
    e.close()
