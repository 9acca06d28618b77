"""The device sampler against its exact host model (tests/sampler_model.py).

Every draw is a pure function of integers, so every comparison
here is ``np.array_equal`` on int arrays: pairs, negatives, group users and the
sampler position.  The model has only the FORWARD epoch bijection; the
device's inverse (64-bit in the radix keys, 32-bit in the counting scatter),
the counting scatter itself and the radix sort all answer to
``sorted(permute(s) for s in batch)``.

Sections (the shapes are the ones at which the code changes path):
  a. bijection widths 1..22 bits, unsorted batches;
  b. the epoch order: sorted_batches {1, 3} x epoch_sort {0, 1}; tile, bin and
     chunk edges of the counting scatter; the handover to the radix sort;
  c. negatives over row geometry and rejection rate, row scan and set probe;
  d. GBPR group users over column geometry;
  e. the batch / epoch / B-change state machine;
  f. the draws inside cf_train_steps, against a twin fed the model's batches.
"""
import numpy as np
import pytest

import sampler_model as SM

pytestmark = pytest.mark.gpu

BIG_EPOCH = 10 ** 6
N_BIG = 64 * 32 * 2048 + 1      # 4,194,305 pairs: the chunk scan's wave loop goes round twice
NI_BIG = 61                     # prime: a row's items (start + k step) mod 61 are distinct


# ---------------------------------------------------------------------------
# graphs
# ---------------------------------------------------------------------------
_big = {}


def big_graph():
    """4,194,305 pairs in rows of 0..39 items out of 61 (so a W = 1 draw
    rejects up to 64 % of its candidates); users 0 and 1 have empty rows."""
    if not _big:
        rng = np.random.RandomState(7)
        lens = rng.randint(0, 40, size=N_BIG // 19 + 1000)
        lens[:2] = 0
        lens[2:8] = [1, 39, 2, 3, 1, 17]
        ip = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        assert ip[-1] >= N_BIG
        u = np.repeat(np.arange(len(lens)), lens)
        k = np.arange(ip[-1]) - ip[u]
        start, step = rng.randint(0, NI_BIG, size=len(lens)), rng.randint(1, NI_BIG, size=len(lens))
        it = (start[u] + k * step[u]) % NI_BIG
        o = np.lexsort((it, u))            # each row ascending
        _big["ip"], _big["ix"] = ip, it[o].astype(np.int32)
    return _big["ip"], _big["ix"]


_trims = {}


def trimmed(nnz):
    """The first nnz pairs of the big graph (the last row cut short), followed
    by two users without a row; its model (shared, see Model.fresh)."""
    if nnz not in _trims:
        ip, ix = big_graph()
        nu = int(np.searchsorted(ip, nnz, side="left"))    # ip[nu] >= nnz > ip[nu - 1]
        tip = np.concatenate([ip[:nu], [nnz, nnz, nnz]]).astype(np.int64)
        tix = ix[:nnz]
        if len(_trims) > 6:                # keep the cache small: the big arrays are views anyway
            _trims.pop(next(iter(_trims)))
        _trims[nnz] = (tip, tix, SM.Model(tip, tix, NI_BIG, 1, 0, 0))
    return _trims[nnz]


GEOM_LENS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513,
             1000, 38]          # + 38: 3,589 pairs = 37 x 97, so a whole epoch at B = 97 holds every pair
_geom = {}


def geom_graph(n_items):
    """Rows of the lengths above in a shuffled order, empty rows between, at
    the start and at the end; items 0 and n_items - 1 are in every other row
    (of length >= 2) and in none of the rest."""
    if n_items not in _geom:
        rng = np.random.RandomState(n_items)
        lens = list(GEOM_LENS)
        rng.shuffle(lens)
        rows = [[]]
        for n, L in enumerate(lens):
            ends = n % 2 == 0 and L >= 2
            mid = rng.choice(np.arange(1, n_items - 1), size=L - 2 if ends else L, replace=False)
            rows.append(np.concatenate([mid, [0, n_items - 1]]) if ends else mid)
            if n % 5 == 3:
                rows.append([])
        rows.append([])
        ip, ix = SM.csr_from_rows(rows)
        assert ip[-1] == sum(GEOM_LENS) == 37 * 97
        _geom[n_items] = (ip, ix, n_items, SM.Model(ip, ix, n_items, 1, 1, 0))
    return _geom[n_items]


def dense_toy():
    """The 30 x 40 toy of test_gpu_sampler.py::test_pos_set_draw_equals_row_scan:
    users own 5..38 of 40 items, so most candidates are rejected."""
    if "toy" not in _geom:
        rng = np.random.RandomState(5)
        rows = [np.sort(rng.choice(40, size=rng.randint(5, 39), replace=False)) for _ in range(30)]
        ip, ix = SM.csr_from_rows(rows)
        _geom["toy"] = (ip, ix, 40, SM.Model(ip, ix, 40, 1, 1, 0))
    return _geom["toy"]


def two_item_graph():
    """n_items = 2: every user has one of the two items (or no row), so the
    only negative is the other one."""
    if "two" not in _geom:
        rng = np.random.RandomState(2)
        rows = [[] if u % 7 == 0 else [int(rng.randint(0, 2))] for u in range(260)]
        ip, ix = SM.csr_from_rows(rows)
        _geom["two"] = (ip, ix, 2, SM.Model(ip, ix, 2, 1, 1, 0))
    return _geom["two"]


def transposed(g):
    """R.T of a graph: users <-> items."""
    ip, ix, ni, _ = g
    nu = len(ip) - 1
    u = np.repeat(np.arange(nu), np.diff(ip))
    o = np.argsort(ix, kind="stable")
    tip = np.concatenate([[0], np.cumsum(np.bincount(ix, minlength=ni))]).astype(np.int64)
    tix = u[o].astype(np.int32)
    return tip, tix, nu, SM.Model(tip, tix, nu, 1, 1, 0)


# ---------------------------------------------------------------------------
# engines and the comparison
# ---------------------------------------------------------------------------
def engine(ip, ix, ni, W=1, G=0, seed=1, d=4, **opts):
    from collaborativefilteringusingtensorflow_amd.engine import Engine
    e = Engine("gbpr" if G else "bpr", len(ip) - 1, ni, d, n_neg=W, gsize=max(G, 1), seed=seed)
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


def draw_and_compare(e, m, B, n, what):
    """n batches of B from the engine and from the model: equal, position included."""
    ref = m.sample_many(B, n)
    for b in range(n):
        same(e.sample(B), ref[b], (what, "draw %d of %d at B = %d" % (b, n, B), m.state()))
    assert e.sampler_state() == m.state(), what


def jump(e, m, epoch, batch):
    e.set_sampler_state(epoch, batch)
    m.set_state(epoch, batch)


def whole_epoch_script(e, m, B, what):
    """Every batch of epoch 0, the first of epoch 1, then the last whole batch
    of a large epoch and the first of the one after."""
    per = m.nnz // B
    draw_and_compare(e, m, B, per + 1, what)
    assert m.state() == (1, 1)
    jump(e, m, BIG_EPOCH, per - 1)
    draw_and_compare(e, m, B, 2, (what, "epoch 10^6"))
    assert m.state() == (BIG_EPOCH + 1, 1)


def edges_script(e, m, B, what, middle=False):
    """The first two batches, (two in the middle,) the last whole batch of the
    epoch and the first of the next; the same end of a large epoch."""
    per = m.nnz // B
    draw_and_compare(e, m, B, min(2, per), what)
    if middle and per > 6:
        jump(e, m, 0, per // 2)
        draw_and_compare(e, m, B, 2, (what, "middle"))
    jump(e, m, 0, per - 1)
    draw_and_compare(e, m, B, 2, (what, "epoch end"))
    assert m.state() == (1, 1)
    jump(e, m, BIG_EPOCH, per - 1)
    draw_and_compare(e, m, B, 2, (what, "epoch 10^6"))


ORDERS = [dict(sorted_batches=0)] + [dict(sorted_batches=sb, epoch_sort=es) for sb in (1, 3) for es in (0, 1)]
SORTED_ORDERS = ORDERS[1:]


def order_id(o):
    return "unsorted" if not o["sorted_batches"] else "sb%d-es%d" % (o["sorted_batches"], o["epoch_sort"])


# ---------------------------------------------------------------------------
# a + b: bijection widths, unsorted and in every form of the epoch order
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS, ids=order_id)
@pytest.mark.parametrize("k", [0] + list(range(3, 13)))
def test_widths_small_whole_epochs(k, order):
    """nnz = 1..5 (k = 0) and 2^k - 1, 2^k, 2^k + 1 for k = 3..12: bijections of
    1 to 13 bits.  Every batch of epoch 0, the first of epoch 1 and an epoch
    boundary at epoch 10^6, at a B with three batches per epoch (and a
    leftover, or none) and at B = nnz."""
    for nnz in ([1, 2, 3, 4, 5] if k == 0 else [(1 << k) - 1, 1 << k, (1 << k) + 1]):
        ip, ix, model = trimmed(nnz)
        for B in sorted({max(1, nnz // 3), nnz}):
            seed = 1000 * k + nnz + B
            e = engine(ip, ix, NI_BIG, seed=seed, **order)
            m = model.fresh(seed=seed, sorted=order["sorted_batches"] != 0)
            whole_epoch_script(e, m, B, (nnz, B, order))
            e.close()


@pytest.mark.parametrize("order", ORDERS, ids=order_id)
@pytest.mark.parametrize("k", range(13, 22))
def test_widths_large_epoch_edges(k, order):
    """2^k - 1, 2^k, 2^k + 1 for k = 13..21 (13 to 22 bits): the first two
    batches, the last whole batch of the epoch and the first of the next, at
    epochs 0 / 1 and 10^6 / 10^6 + 1, with B <= 4,096 (several batches per
    epoch; up to 513 bins of the counting scatter)."""
    for nnz, B in (((1 << k) - 1, 4096), (1 << k, 4096 if k > 13 else 2048), ((1 << k) + 1, 3001)):
        ip, ix, model = trimmed(nnz)
        seed = 77 * k + B
        e = engine(ip, ix, NI_BIG, seed=seed, **order)
        m = model.fresh(seed=seed, sorted=order["sorted_batches"] != 0)
        edges_script(e, m, B, (nnz, B, order))
        e.close()


@pytest.mark.parametrize("order", SORTED_ORDERS, ids=order_id)
@pytest.mark.parametrize("nnz", [2047, 2048, 2049, 4096, 4097, 65536, 65537])
def test_epoch_order_tile_edges(nnz, order):
    """Tiles of 2,048 pairs: a partial last tile of 2,047 and of 1 pair (the
    copy-out's duplicate store), whole tiles, and 65,537 pairs = 32 tiles + 1
    = one chunk + 1 tile of the column scan.  Whole epochs of five batches
    with a leftover, and of four without where 4 divides nnz."""
    ip, ix, model = trimmed(nnz)
    for B in sorted({nnz // 5, nnz // 4}):
        e = engine(ip, ix, NI_BIG, seed=nnz + B, **order)
        m = model.fresh(seed=nnz + B, sorted=True)
        whole_epoch_script(e, m, B, (nnz, B, order))
        e.close()


# n_bins = nnz // B + 1 -> (B, [nnz with nnz % B == 0, nnz with nnz % B != 0]); 20K..70K pairs
def _bin_cases():
    out = []
    for nb in (2, 3, 254, 255, 256, 511, 512, 767, 768, 1022, 1023, 1024):
        B = 45000 // nb
        out.append((nb + 1, B, nb * B))
        out.append((nb + 1, B, nb * B + min(B - 1, 17)))
    out.append((2, 30011, 30011))             # B = nnz: one batch, the leftover bin empty
    out.append((2, 20000, 30011))             # nnz / 2 < B < nnz: one batch and a leftover
    return out


@pytest.mark.parametrize("order", SORTED_ORDERS, ids=order_id)
@pytest.mark.parametrize("n_bins,B,nnz", _bin_cases())
def test_epoch_order_bin_edges(n_bins, B, nnz, order):
    """The counting scatter's bins: 1..4 consecutive bins per thread (256 / 257,
    512 / 513, 768 / 769 bins), the sentinel's own code at a power-of-two bin
    count (4, 256, 512, 1,024), the empty leftover bin (nnz % B == 0), one
    batch per epoch, and the handover to the radix sort: 1,024 bins is the
    last counting case, 1,025 the first radix one under epoch_sort 0."""
    assert nnz // B + 1 == n_bins and 20000 <= nnz <= 70000
    ip, ix, model = trimmed(nnz)
    e = engine(ip, ix, NI_BIG, seed=n_bins + nnz, **order)
    m = model.fresh(seed=n_bins + nnz, sorted=True)
    edges_script(e, m, B, (n_bins, B, nnz, order), middle=True)
    e.close()


@pytest.mark.parametrize("order", SORTED_ORDERS, ids=order_id)
def test_epoch_order_batch_size_one(order):
    """B = 1 on 1,000 pairs (bin_of_slot's B == 1 branch, 1,001 bins): a whole
    epoch and the start of the next."""
    ip, ix, model = trimmed(1000)
    e = engine(ip, ix, NI_BIG, seed=5, **order)
    m = model.fresh(seed=5, sorted=True)
    whole_epoch_script(e, m, 1, order)
    e.close()


@pytest.mark.parametrize("order", SORTED_ORDERS, ids=order_id)
@pytest.mark.parametrize("B", [1 << 16, 5000])
def test_epoch_order_large(B, order):
    """4,194,305 pairs = 64 x 32 tiles + 1 pair: 65 chunks, so the chunk scan's
    wave loop goes round twice (65 and 839 bins).  First, middle and last whole
    batch and the next epoch's first; the model permutes only those slots."""
    ip, ix, model = trimmed(N_BIG)
    e = engine(ip, ix, NI_BIG, seed=B, **order)
    m = model.fresh(seed=B, sorted=True)
    per = N_BIG // B
    draw_and_compare(e, m, B, 1, (B, order, "first"))
    jump(e, m, 0, per // 2)
    draw_and_compare(e, m, B, 1, (B, order, "middle"))
    jump(e, m, 0, per - 1)
    draw_and_compare(e, m, B, 2, (B, order, "epoch end"))
    assert m.state() == (1, 1)
    e.close()


# ---------------------------------------------------------------------------
# c: negatives over row geometry and rejection rate
# ---------------------------------------------------------------------------
NEG_WS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 16, 17, SM.K_MAX_NEG]
NEG_GRAPHS = {"geom-1003": lambda: geom_graph(1003), "geom-100000": lambda: geom_graph(100000),
              "dense-toy": dense_toy, "two-items": two_item_graph}


@pytest.mark.parametrize("W", NEG_WS)
@pytest.mark.parametrize("graph", list(NEG_GRAPHS))
def test_negatives_over_row_geometry(graph, W):
    """Rows of 1..1,000 ids around every multiple of the scan's 64 ids per
    iteration (4-lane groups at W = 1, 8-lane groups otherwise), C = PGL / nw
    first-scan candidates per negative for every nw, several w0 rounds (W >
    8), and the redraw loop: at n_items = 1,003 the 1,000-row rejects 99.7 %
    of its candidates (~334 attempts per negative), at 100,000 almost none.
    Row scan and set probe, sorted and unsorted batches, a whole epoch at
    B = 97 (every pair of the geometry graph; every user)."""
    ip, ix, ni, model = NEG_GRAPHS[graph]()
    B = 97 if len(ix) >= 97 else 30
    per = len(ix) // B
    for srt in (0, 1):
        m = model.fresh(n_neg=W, gsize=0, seed=W, sorted=bool(srt))
        ref = m.sample_many(B, per + 1)
        users = np.unique(np.concatenate([r[0][:, 0] for r in ref]))
        if len(ix) % B == 0:
            assert np.array_equal(users, np.nonzero(np.diff(ip))[0])   # every user with a row
        for check in (0, 1):
            e = engine(ip, ix, ni, W=W, seed=W, sorted_batches=srt, neg_check=check)
            for b in range(per + 1):
                same(e.sample(B), ref[b], (graph, W, "sorted %d neg_check %d batch %d" % (srt, check, b)))
            assert e.sampler_state() == m.state()
            e.close()


# ---------------------------------------------------------------------------
# d: GBPR group users
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 5])
@pytest.mark.parametrize("G", [1, 2, 3, 7, 8, 9, SM.K_MAX_GROUP])
def test_gbpr_groups_over_column_geometry(G, W):
    """The geometry graph transposed: items whose columns hold 1, 2, .. 64, 65,
    .. 1,000 users.  Member k strides by the group's lanes when G exceeds them
    (G = 7 / 9 at W = 1's four lanes and W = 5's eight, 16 = kMaxGroup);
    members repeat and include u itself, exactly as the model's."""
    ip, ix, ni, model = transposed(geom_graph(1003))
    B = 97
    per = len(ix) // B
    hit_self = repeats = 0
    for srt in (0, 1):
        m = model.fresh(n_neg=W, gsize=G, seed=100 * G + W, sorted=bool(srt))
        e = engine(ip, ix, ni, W=W, G=G, seed=100 * G + W, sorted_batches=srt)
        ref = m.sample_many(B, per + 1)
        for b in range(per + 1):
            same(e.sample(B), ref[b], (G, W, srt, b))
            hit_self += int((ref[b][2] == ref[b][0][:, :1]).sum())
            repeats += int((np.diff(np.sort(ref[b][2], axis=1), axis=1) == 0).sum())
        assert e.sampler_state() == m.state()
        e.close()
    assert hit_self > 0 and (G == 1 or repeats > 0)


# ---------------------------------------------------------------------------
# e: the state machine
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("order", [ORDERS[0], ORDERS[1]], ids=order_id)
def test_state_machine_follows_model(order):
    from collaborativefilteringusingtensorflow_amd import _native as N
    nnz = 1000
    ip, ix, model = trimmed(nnz)
    srt = order["sorted_batches"] != 0
    B = 96
    per = nnz // B                      # 10 batches and a leftover of 40 pairs
    e = engine(ip, ix, NI_BIG, W=2, seed=9, **order)
    m = model.fresh(n_neg=2, seed=9, sorted=srt)
    assert e.sampler_state() == m.state() == (0, 0)
    draw_and_compare(e, m, B, per, "epoch 0")
    assert m.state() == (0, per)        # the rollover is taken at the next draw
    draw_and_compare(e, m, B, 2, "rollover")
    assert m.state() == (1, 2)
    draw_and_compare(e, m, 50, 3, "B change in mid-epoch")        # -> epoch 2, batch 0
    assert m.state() == (2, 3)
    draw_and_compare(e, m, B, 2, "and the change back")           # -> epoch 3, batch 0
    assert m.state() == (3, 2)
    jump(e, m, 3, 0)
    draw_and_compare(e, m, 50, 1, "B change at batch 0 stays in the epoch")
    assert m.state() == (3, 1)
    jump(e, m, 11, 4)
    draw_and_compare(e, m, 50, 2, "set_sampler_state after draws")
    jump(e, m, 12, nnz // 50)
    draw_and_compare(e, m, 50, 1, "set_sampler_state past the last batch")
    assert m.state() == (13, 1)
    draw_and_compare(e, m, nnz, 3, "B == nnz")                    # one batch per epoch
    assert m.state() == (16, 1)
    st = e.sampler_state()
    with pytest.raises(N.NativeError, match="batch size exceeds"):
        e.sample(nnz + 1)
    with pytest.raises(ValueError):
        m.sample(nnz + 1)
    assert e.sampler_state() == st == m.state()
    with pytest.raises(N.NativeError, match="negative sampler state"):
        e.set_sampler_state(-1, 0)
    e.close()
    # on a fresh engine the position is kept whatever the first B is
    e = engine(ip, ix, NI_BIG, W=2, seed=9, **order)
    m = model.fresh(n_neg=2, seed=9, sorted=srt)
    jump(e, m, 5, 7)
    draw_and_compare(e, m, B, 4, "set_sampler_state on a fresh engine")
    assert m.state() == (6, 1)
    e.close()


# ---------------------------------------------------------------------------
# f: the draws inside cf_train_steps
# ---------------------------------------------------------------------------
F_OPTS = {
    "default": {},
    "stepwise": {"pipeline": 0},
    "draw-in-grad": {"pipeline": 2},
    "side-stream": {"prep_stream": 1, "pipeline": 0},
    "unsorted": {"sorted_batches": 0},
    "sorted": {"sorted_batches": 1},
    "sorted-index": {"sorted_batches": 3},
    "set-probe": {"neg_check": 1},
    # the speculative first-candidate counts, as test_gpu_pos_sort.py::test_spec_neg_* set them
    "spec-neg": {"item_slots": 0, "pos_sort": 1, "spec_neg": 1},
}
F_SHAPES = {"bpr-W1": ("bpr", 1, 1), "bpr-W5": ("bpr", 5, 1), "bpr-W12": ("bpr", 12, 1), "gbpr-G3-W2": ("gbpr", 2, 3)}
F_TABLES = {"bpr": ("user", "item", "acc_user", "acc_item"),
            "gbpr": ("user", "item", "bias", "acc_user", "acc_item", "acc_bias")}


def _f_cases():
    """Options x shapes x B, trimmed to the pairs that reach distinct kernels:
    every option set with every shape at B = 257 (the positive sort behind
    spec-neg runs at W = 1 and 5 only); the three launch forms that host a
    draw (apply + draw, its own launch, the gradient launch) also at B = 33
    and 1,000 with every shape (W = 12 at B = 33 in the apply launch only);
    B = 1 with the 4-lane draw in the apply and in the gradient launch (the
    draw in a launch of its own is what cf_sample runs at B = 1 in sections
    a, b and e).  Where sorted_batches is not set, auto sorts at B = 1 and 33 (16 or
    more batches per epoch) and not at B = 257 and 1,000."""
    out = []
    for o in F_OPTS:
        for s in F_SHAPES:
            if o == "spec-neg" and s not in ("bpr-W1", "bpr-W5"):
                continue
            out.append((o, s, 257))
    for o in ("default", "stepwise", "draw-in-grad"):
        for s in F_SHAPES:
            out.append((o, s, 1000))
            if s != "bpr-W12" or o == "default":   # 112 steps whose 1,000-id row redraws ~334 times per negative
                out.append((o, s, 33))
    # B = 1 needs a whole epoch of 3,589 single-pair steps between its two boundaries
    out += [("default", "bpr-W1", 1), ("draw-in-grad", "bpr-W1", 1)]
    return out


_f_ref = {}


def _f_reference(model, shape, B, srt, start, K):
    """The model's K batches from ``start``, its end state and the batch after
    (the option sets of one shape, B and order share them: same seed, same stream)."""
    key = (shape, B, srt, start, K)
    if key not in _f_ref:
        _, W, G = F_SHAPES[shape]
        m = model.fresh(n_neg=W, gsize=G if shape.startswith("gbpr") else 0, seed=31, sorted=srt)
        m.set_state(*start)
        batches = m.sample_many(B, K)
        _f_ref[key] = (batches, m.state(), m.sample(B))
    return _f_ref[key]


@pytest.mark.parametrize("opts,shape,B", _f_cases())
def test_train_steps_draws_follow_model(opts, shape, B):
    """cf_train_steps draws inside apply_prep_kernel (pipeline 1), in a launch
    of its own (pipeline 0, on the engine or the side stream) or inside the
    gradient launch (pipeline 2).  Engine A trains K device-drawn steps in
    deterministic mode across two epoch boundaries; its twin, from the same
    init_params, is fed the MODEL's batches one cf_step at a time.
    Deterministic sums are order-free, so equal batches give
    bitwise equal tables, and a batch that differs in one id does not."""
    from collaborativefilteringusingtensorflow_amd.engine import Engine
    model_name, W, G = F_SHAPES[shape]
    ip, ix, ni, model = geom_graph(1003)
    nu = len(ip) - 1
    kw = dict(reg=0.05, rho=0.4) if model_name == "gbpr" else dict(reg=0.05)
    pair = []
    for _ in range(2):
        e = Engine(model_name, nu, ni, 8, n_neg=W, gsize=G, seed=31, **kw)
        for k, v in F_OPTS[opts].items():
            e.set_option(k, v)
        e.set_option("deterministic", 1)
        e.set_interactions(ip, ix)
        e.init_params(0.0, 0.1, seed=5)
        pair.append(e)
    a, twin = pair
    per = len(ix) // B
    if per > 20:      # start two batches before the end of epoch 0
        a.set_sampler_state(0, per - 2)
        K = 2 + per + 2
    else:
        K = 2 * per + 2
    # without the option, batches are sorted from 16 batches per epoch (auto)
    srt = bool(F_OPTS[opts].get("sorted_batches", per >= 16))
    assert a.step_path(B)[1]["sorted_batches"] == srt
    batches, end, after = _f_reference(model, shape, B, srt, a.sampler_state(), K)
    a.train_steps(B, K)
    for pairs, negs, groups in batches:
        twin.step(pairs, negs, groups, return_loss=False)
    assert end[0] >= 2
    assert a.sampler_state() == end
    assert a.step_path(B)[1]["sorted_batches"] == srt
    for t in F_TABLES[model_name]:
        assert np.array_equal(a.get_table(t), twin.get_table(t)), (t, opts, shape, B)
    # and the stream goes on from there
    same(a.sample(B), after, "after train_steps")
    a.close()
    twin.close()
