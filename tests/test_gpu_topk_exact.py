"""The recommend step on tables whose scores are EXACT in float32: no
tolerance anywhere in this file.

tests/test_gpu_topk.py feeds random tables, where float32 rounding is visible
and a near-tie rule is needed.  Here every table entry is a small integer (or
a one-hot row times a chosen column), every partial sum is an integer below
2^24 (or a single float32 number), so the score is the same float32 number
whatever the summation order, the fused kernels' expanded CML form included.
The float64 oracle's list is then the only correct answer, and each call is
checked three ways:

* ``idx`` equals the oracle's list (descending, ties to the lower id);
* ``val`` equals float32(S[r, idx]) bit for bit;
* positions past the user's remaining items hold idx -1 and a NaN value.

The sign of a zero is the one thing left open: CML at distance 0 is -0.0 in
the direct form (score_kernel, the oracle) and +0.0 in the fused kernels'
2 u.v - |v|^2 - |u|^2, and either is the row's maximum, so its order cannot
be observed; the values are compared after adding +0.0 to both sides.

Family A1 (test_a1_*): small-integer tables with massive ties at the factor
counts, item counts, user counts and k where the kernels change path, with
train rows and item masks that stress the exclusion cursor.

Family A2 (test_a2_*): one-hot user rows, so that column c of the item table
IS the score profile of user class c: scores ascending in the item id (every
tile passes the prefilter, every tile compacts, the threshold rises every
tile), sawteeth that put chosen entry counts into the compactions, ulp steps
around the threshold float, the whole list in the last partial tile.  The
same profiles run through the materialised path's radix select.

Every case runs on the four fused kernels (cf_set_option fused_variant).
"""
import functools

import numpy as np
import pytest

from oracle import cf_oracle as O

pytestmark = pytest.mark.gpu

_FV = [0]
F32 = np.float32
MODELS = ("bpr", "gbpr", "cml", "amf")
FUSED, MATERIALISED, AUTO = 2, 1, 0      # cf_set_option("topk_path")


@pytest.fixture(autouse=True, params=[0, 1, 2, 3], ids=["fused-seq", "fused-pipe", "fused-ws", "fused-u128"])
def fused_variant(request):
    _FV[0] = request.param
    yield request.param
    _FV[0] = 0


# ----------------------------------------------------------------------------
# helpers
# ----------------------------------------------------------------------------
def csr(rows):
    indptr = np.zeros(len(rows) + 1, np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    indices = np.concatenate([np.asarray(r, np.int64) for r in rows]).astype(np.int32)
    return indptr, indices


def make_engine(model, U, V, b, rows):
    """An engine holding exactly these tables and train rows (sorted ids per user)."""
    from collaborativefilteringusingtensorflow_amd.engine import Engine
    e = Engine(model, U.shape[0], V.shape[0], U.shape[1], n_neg=1, gsize=1, seed=1)
    e.set_option("fused_variant", _FV[0])
    e.set_interactions(*csr(rows))
    e.set_table("user", U)
    e.set_table("item", V)
    if b is not None:
        e.set_table("bias", b)
    return e


def exact_scores(model, U, V, b, users):
    """The oracle's float64 scores; they must be float32 numbers."""
    assert U.dtype == F32 and V.dtype == F32
    S = O.predict(model, U.astype(np.float64), V.astype(np.float64),
                  None if b is None else b.astype(np.float64), users)
    assert np.array_equal(S.astype(F32).astype(np.float64), S), "the table's scores are not exact in float32"
    return S


def reference(S, excluded, k):
    """(idx [n, k], val [n, k]) the call must return: cf_oracle.recommend over
    each row's excluded ids, padded with -1 / NaN."""
    n = S.shape[0]
    indptr, indices = csr(excluded)
    lists = O.recommend(S, indptr, indices, np.arange(n), k)
    idx = np.full((n, k), -1, np.int32)
    val = np.full((n, k), np.nan, F32)
    for r, row in enumerate(lists):
        idx[r, :len(row)] = row
        val[r, :len(row)] = S[r, row]
    return idx, val


def assert_exact(out, ref, what):
    idx, val = out
    ridx, rval = ref
    assert idx.shape == ridx.shape and val.shape == rval.shape, what
    if not np.array_equal(idx, ridx):
        r = int(np.nonzero((idx != ridx).any(axis=1))[0][0])
        p = int(np.nonzero(idx[r] != ridx[r])[0][0])
        raise AssertionError("%s: %d rows differ from the oracle's list; row %d first at position %d: "
                             "got %s, oracle %s" % (what, int((idx != ridx).any(axis=1).sum()), r, p,
                                                   idx[r, p:p + 6].tolist(), ridx[r, p:p + 6].tolist()))
    pad = ridx < 0
    assert np.isnan(val[pad]).all(), (what, "a padded position holds a value")
    got = (val[~pad] + F32(0)).view(np.uint32)       # + 0.0: the sign of a zero is not compared
    want = (rval[~pad] + F32(0)).view(np.uint32)
    if not np.array_equal(got, want):
        q = int(np.nonzero(got != want)[0][0])
        raise AssertionError("%s: %d values differ in their bits from float32(S[r, idx]); first: got %r, oracle %r"
                             % (what, int((got != want).sum()), val[~pad][q], rval[~pad][q]))


def excluded_rows(rows, users, exclude_train, mask, n_items):
    flagged = np.nonzero(mask)[0] if mask is not None else np.zeros(0, np.int64)
    out = []
    for u in users:
        tr = np.asarray(rows[u], np.int64) if exclude_train else np.zeros(0, np.int64)
        out.append(np.union1d(tr, flagged))
    return out


def run_case(e, S, rows, users, k, path, exclude_train=True, mask=None, what=""):
    """One cf_score_topk_ex call against the oracle, exactly."""
    e.set_option("topk_path", path)
    out = e.score_topk(users, k, exclude_train=exclude_train, return_values=True, item_mask=mask)
    ref = reference(S, excluded_rows(rows, users, exclude_train, mask, S.shape[1]), k)
    assert_exact(out, ref, "%s variant %d path %d k %d train %d mask %d"
                 % (what, _FV[0], path, k, exclude_train, mask is not None))
    return out, ref


def int_tables(rng, model, nu, ni, d):
    """Entries in {-3..3}, GBPR's bias in {-5..5}: every product, partial sum
    and squared distance is an integer far below 2^24."""
    U = rng.randint(-3, 4, (nu, d)).astype(F32)
    V = rng.randint(-3, 4, (ni, d)).astype(F32)
    b = rng.randint(-5, 6, ni).astype(F32) if model == "gbpr" else None
    return U, V, b


def random_rows(rng, nu, ni):
    """Train rows of mixed density: empty, sparse, half, nearly full."""
    dens = (0.0, 0.05, 0.5, 0.9)
    rows = [np.nonzero(rng.rand(ni) < dens[u % 4])[0] for u in range(nu)]
    if sum(len(r) for r in rows) == 0:
        rows[0] = np.array([0])
    return rows


def fused_paths(d, k):
    """The paths a (d, k) case runs on: the fused kernel where it exists,
    and the materialised kernels."""
    return (FUSED, MATERIALISED) if d <= 128 and k <= 128 else (AUTO, MATERIALISED)


# ----------------------------------------------------------------------------
# A1: small-integer tables
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 4, 5, 8, 12, 63, 64, 65, 127, 128])
def test_a1_factor_dims(d):
    """d & 3 picks the vector or the scalar tile staging, Dp = (d + 7) & ~7
    the padded operand width; every model, narrow and wide lists."""
    for m, model in enumerate(MODELS):
        rng = np.random.RandomState(1000 + 10 * d + m)
        nu, ni = 70, 150
        U, V, b = int_tables(rng, model, nu, ni, d)
        rows = random_rows(rng, nu, ni)
        users = np.arange(nu, dtype=np.int32)
        S = exact_scores(model, U, V, b, users)
        e = make_engine(model, U, V, b, rows)
        for k in (7, 40):
            for path in (FUSED, MATERIALISED):
                run_case(e, S, rows, users, k, path, what="%s d %d" % (model, d))
        e.close()


@pytest.mark.parametrize("d", [129, 256])
def test_a1_factor_dims_past_the_fused_kernels(d):
    """n_factors > 128: topk_path 0 quietly takes the materialised kernels
    (a score launch is recorded), topk_path 2 is CF_EINVAL."""
    from collaborativefilteringusingtensorflow_amd._native import NativeError
    for m, model in enumerate(MODELS):
        rng = np.random.RandomState(2000 + 10 * d + m)
        nu, ni = 66, 150
        U, V, b = int_tables(rng, model, nu, ni, d)
        rows = random_rows(rng, nu, ni)
        users = np.arange(nu, dtype=np.int32)
        S = exact_scores(model, U, V, b, users)
        e = make_engine(model, U, V, b, rows)
        for k in (7, 40):
            e.profile_reset()
            e.profile(True)
            run_case(e, S, rows, users, k, AUTO, what="%s d %d" % (model, d))
            e.profile(False)
            assert e.profile_read("score")[1] >= 1
            run_case(e, S, rows, users, k, MATERIALISED, what="%s d %d" % (model, d))
        e.set_option("topk_path", FUSED)
        with pytest.raises(NativeError, match="CF_EINVAL"):
            e.score_topk(users, 7)
        e.close()


def test_a1_one_item_is_rejected():
    """cf_create takes n_items >= 2: a one-item catalogue never reaches a kernel."""
    from collaborativefilteringusingtensorflow_amd._native import NativeError
    from collaborativefilteringusingtensorflow_amd.engine import Engine
    with pytest.raises(NativeError, match="n_items out of range"):
        Engine("bpr", 4, 1, 4)


@pytest.mark.parametrize("ni", [2, 63, 64, 65, 127, 128, 129, 613])
def test_a1_item_counts(ni):
    """One tile, one item short of it, one past it, two tiles and their
    neighbours, ten tiles with a partial last one; k up to one past ni."""
    for m, model in enumerate(("bpr", "gbpr", "cml")):
        rng = np.random.RandomState(3000 + 10 * ni + m)
        nu, d = 66, 12
        U, V, b = int_tables(rng, model, nu, ni, d)
        rows = random_rows(rng, nu, ni)
        users = np.arange(nu, dtype=np.int32)
        S = exact_scores(model, U, V, b, users)
        e = make_engine(model, U, V, b, rows)
        for k in sorted({1, min(28, ni + 1), min(29, ni + 1), min(128, ni + 1), ni + 1}):
            for path in fused_paths(d, k):
                run_case(e, S, rows, users, k, path, what="%s ni %d" % (model, ni))
                if k > 28:
                    run_case(e, S, rows, users, k, path, exclude_train=False, what="%s ni %d" % (model, ni))
        e.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129])
def test_a1_users_per_call(n):
    """User counts around the 64-user block and the 128-user block of
    fused_variant 3; the ids repeat and are not sorted."""
    for m, model in enumerate(MODELS):
        rng = np.random.RandomState(4000 + 10 * n + m)
        nu, ni, d = 40, 200, 16
        U, V, b = int_tables(rng, model, nu, ni, d)
        rows = random_rows(rng, nu, ni)
        users = rng.randint(0, nu, n).astype(np.int32)
        if n > 2:
            users[-1] = users[0]              # a repeat across the call's first and last block
        S = exact_scores(model, U, V, b, users)
        e = make_engine(model, U, V, b, rows)
        for k in (10, 50):
            for path in (FUSED, MATERIALISED):
                run_case(e, S, rows, users, k, path, what="%s n %d" % (model, n))
        e.close()


@pytest.mark.parametrize("k", [1, 27, 28, 29, 64, 65, 127, 128, 129, 600])
def test_a1_list_widths(k):
    """k <= 28 the narrow lists, 29..128 the wide ones, above that the
    materialised kernels; which one ran is read from the profile."""
    for m, model in enumerate(("bpr", "gbpr", "cml")):
        rng = np.random.RandomState(5000 + 10 * k + m)
        nu, ni, d = 66, 613, 24
        U, V, b = int_tables(rng, model, nu, ni, d)
        rows = random_rows(rng, nu, ni)
        users = np.arange(nu, dtype=np.int32)
        S = exact_scores(model, U, V, b, users)
        e = make_engine(model, U, V, b, rows)
        e.profile_reset()
        e.profile(True)
        run_case(e, S, rows, users, k, AUTO, what="%s k %d" % (model, k))
        e.profile(False)
        assert e.profile_read("topk")[1] >= 1
        if k <= 128:
            assert e.profile_read("score")[1] == 0     # fused: no score matrix written
        else:
            assert e.profile_read("score")[1] >= 1
        run_case(e, S, rows, users, k, MATERIALISED, what="%s k %d" % (model, k))
        run_case(e, S, rows, users, k, AUTO, exclude_train=False, what="%s k %d" % (model, k))
        e.close()


@pytest.mark.parametrize("left", [20, 100, 200])
def test_a1_k_around_the_items_left(left):
    """k one below, equal to and one above the number of items a user has
    left (narrow lists, wide lists, materialised); one user has every item in
    its train row and gets nothing but padding."""
    ni, d, nu = 300, 8, 70
    for m, model in enumerate(("bpr", "gbpr", "cml")):
        rng = np.random.RandomState(6000 + 10 * left + m)
        U, V, b = int_tables(rng, model, nu, ni, d)
        rows = random_rows(rng, nu, ni)
        for u in range(0, nu, 5):             # in every block of every variant
            kind = (u // 5) % 4
            if kind == 0:
                rows[u] = np.sort(rng.permutation(ni)[:ni - left])      # `left` items left
            elif kind == 1:
                rows[u] = np.arange(ni)                                 # none left
            elif kind == 2:
                rows[u] = np.delete(np.arange(ni), ni - 1)              # the last item alone
            else:
                rows[u] = np.zeros(0, np.int64)                         # all left
        users = np.arange(nu, dtype=np.int32)
        S = exact_scores(model, U, V, b, users)
        e = make_engine(model, U, V, b, rows)
        for k in (left - 1, left, left + 1):
            for path in fused_paths(d, k):
                (idx, val), _ = run_case(e, S, rows, users, k, path, what="%s left %d" % (model, left))
                assert (idx[5] == -1).all() and np.isnan(val[5]).all()
                assert (idx[0] >= 0).sum() == min(k, left)
                assert idx[10, 0] == ni - 1 and (idx[10, 1:] == -1).all()
        e.close()


def cursor_rows(ni):
    """Train rows that stress the exclusion cursor (ni = 64 T + r, T >= 5)."""
    tiles = [np.arange(t * 64, min(ni, t * 64 + 64)) for t in range((ni + 63) // 64)]
    return [
        np.zeros(0, np.int64),                 # empty
        np.arange(64, 128),                    # exactly one whole tile
        np.arange(40, 64),                     # ends at item 63
        np.arange(50, 65),                     # ends at item 64
        np.arange(ni - 41, ni),                # ends at the last item
        np.concatenate(tiles[0::2]),           # every second tile whole
        np.concatenate(tiles[1::2]),           # the other tiles whole
        np.array([0]),
        np.array([ni - 1]),
        np.array([63, 64, 127, 128, ni - 1]),  # tile edges only
        np.arange(ni),                         # everything
    ]


@pytest.mark.parametrize("mode", ["train", "mask", "both"])
def test_a1_train_rows_and_item_masks(mode):
    """The rows of cursor_rows as train rows (exclude_train alone), as item
    masks alone (cf_score_topk with a mask: ids through recommend(), ids and
    values through the _ex form), and both overlapping; the mask's last word
    is partial."""
    ni, d, nu = 64 * 5 + 21, 8, 140
    pats = cursor_rows(ni)
    for m, model in enumerate(("bpr", "gbpr", "cml")):
        rng = np.random.RandomState(7000 + m)
        U, V, b = int_tables(rng, model, nu, ni, d)
        rows = [pats[u % len(pats)] for u in range(nu)]
        users = np.arange(nu, dtype=np.int32)
        S = exact_scores(model, U, V, b, users)
        e = make_engine(model, U, V, b, rows)
        masks = [None]
        if mode != "train":
            masks = []
            for p in (1, 4, 5, 6, 9):
                mk = np.zeros(ni, np.uint8)
                mk[pats[p]] = 1
                masks.append(mk)
            masks.append((rng.rand(ni) < 0.3).astype(np.uint8))
        for mk in masks:
            for k in (10, 40):
                for path in (FUSED, MATERIALISED):
                    what = "%s %s" % (model, mode)
                    _, ref = run_case(e, S, rows, users, k, path, exclude_train=(mode != "mask"), mask=mk, what=what)
                    if mode == "mask":
                        assert np.array_equal(e.recommend(users, k, mask=mk), ref[0]), (what, path, k)
                    if mode == "train":
                        assert np.array_equal(e.recommend(users, k), ref[0]), (what, path, k)
        e.close()


# ----------------------------------------------------------------------------
# A2: chosen arrival orders
# ----------------------------------------------------------------------------
SAW_M = (1, 29, 36, 37, 63)      # scores per tile above everything seen so far
A2_D = 24                        # one score profile per column (d & 3 == 0: the prefetched tile path)
A2_REPLICAS = 8                  # users per profile, spread over the blocks of a call


def profiles(ni, r, ulp):
    """[ni, A2_D] float32: column c is the score profile of user class c.
    Lists of k entries compact when they hold more than 28 (narrow) or 128
    (wide) entries, down to k: a sawtooth with m new maxima per tile gives the
    narrow k = 28 lists compactions of 28 + m entries (29, 64, 65, 91, and 92 =
    CAP for the ascending profile), the wide k = 128 lists 128 + m (129, 191,
    192 = CAP), the wide k = 100 lists 100 + 29 = 129."""
    rng = np.random.RandomState(900 + ni)
    j = np.arange(ni)
    t, w = j // 64, j % 64
    T = (ni + 63) // 64
    p1, p2 = rng.permutation(ni), rng.permutation(ni)
    cols = [
        j,                                   # 0 ascending: every score passes, every tile compacts
        -j,                                  # 1 descending: nothing after the list is full
        (T - t) * 64 + w,                    # 2 ascending inside a tile, tiles descending
        t * 64 + (63 - w),                   # 3 descending inside a tile, tiles ascending
    ]
    for m in SAW_M:                          # 4..8 m maxima per tile at scattered lanes, the rest below all before
        rank = (w * 7) % 64                  # a permutation of the tile's 64 lanes
        cols.append(np.where(rank < m, t * 64 + rank + 1, -(j + 1)))
    cols += [
        np.full(ni, 2),                      # 9 everything ties
        j // 7,                              # 10 tie groups straddle the tile edges
        -(j // 7),                           # 11
        p1,                                  # 12 a random permutation
        j - ni // 2,                         # 13 mixed signs and an exact 0.0
    ]
    if ulp:                                  # 14, 15 one-ulp steps: every key shares its high bits
        cols += [1.0 + p2 * 2.0 ** -23, -(1.0 + p2 * 2.0 ** -23)]
    else:                                    # (GBPR: 1 + p 2^-23 + b is not a float32 number)
        cols += [p2 // 3, -(p2 // 3)]
    last = r if r else 3                     # 16 all equal but the last items, which are the top
    cols.append(np.where(j >= ni - last, 10 + j - (ni - last), 1))
    cols += [
        (w * 37) % 64,                       # 17 the same 64 values in every tile: ties across tiles
        -(j % 2),                            # 18 alternating
        -p1,                                 # 19
    ]
    if ulp:
        cols += [
            1.0 + j * 2.0 ** -23,                     # 20 every score one ulp above the best so far
            -(1.0 + j * 2.0 ** -23),                  # 21 and one ulp below the worst
            1.0 + (j % 2) * 2.0 ** -23,               # 22 two adjacent floats: the threshold float ties
            -(1.0 + ((w * 37) % 64) * 2.0 ** -23),    # 23 64 adjacent floats, repeated in every tile
        ]
    else:
        cols += [j // 2, -(j // 2), j % 3, -((w * 37) % 64)]
    V = np.stack([np.asarray(c, np.float64) for c in cols], axis=1)
    assert V.shape == (ni, A2_D) and np.abs(V).max() < 2.0 ** 12
    assert np.array_equal(V.astype(F32).astype(np.float64), V)
    return V.astype(F32)


@functools.lru_cache(maxsize=None)
def a2_case(model, r):
    """Tables, train rows and float64 scores of one A2 engine (shared by the
    four kernels' runs of a case)."""
    ni = 64 * 9 + r
    nu = A2_D * A2_REPLICAS
    V = profiles(ni, r, ulp=(model != "gbpr"))
    U = np.zeros((nu, A2_D), F32)
    U[np.arange(nu), np.arange(nu) % A2_D] = 1.0
    # an integer bias with the opposite trend to the ascending profile: j - 2 (j // 3)
    # rises by one over every three items, and the bias decides the order inside them
    b = (-2.0 * (np.arange(ni) // 3)).astype(F32) if model == "gbpr" else None
    users = np.arange(nu, dtype=np.int32)
    S = exact_scores(model, U, V, b, users)
    rows = []
    for u in range(nu):                      # replica q of class c loses part of its current top
        q = u // A2_D
        top = np.argsort(-S[u], kind="stable")
        if q % 4 == 0:
            row = np.zeros(0, np.int64)
        elif q % 4 == 1:
            row = top[0:128:3]               # ascending profile: every third item of the last two tiles
        elif q % 4 == 2:
            row = top[:40]                   # the whole current top
        else:
            row = top[1:200:2]
        rows.append(np.sort(row))
    return U, V, b, rows, users, S


@functools.lru_cache(maxsize=None)
def a2_reference(model, r, k, exclude_train):
    _, _, _, rows, users, S = a2_case(model, r)
    return reference(S, excluded_rows(rows, users, exclude_train, None, S.shape[1]), k)


@pytest.mark.parametrize("lists", ["narrow", "wide"])
@pytest.mark.parametrize("r", [0, 1, 37])
def test_a2_arrival_orders(r, lists):
    """n_items = 64 * 9 + r; k = 1, 28 on the narrow lists, 29, 100, 128 on
    the wide ones; the fused kernels and the radix select; with and without
    train rows that remove part of each user's top."""
    for model in ("bpr", "gbpr"):
        U, V, b, rows, users, _ = a2_case(model, r)
        e = make_engine(model, U, V, b, rows)
        for k in ((1, 28) if lists == "narrow" else (29, 100, 128)):
            for path in (FUSED, MATERIALISED):
                for excl in (False, True):
                    e.set_option("topk_path", path)
                    out = e.score_topk(users, k, exclude_train=excl, return_values=True)
                    assert_exact(out, a2_reference(model, r, k, excl),
                                 "%s r %d variant %d path %d k %d train %d" % (model, r, _FV[0], path, k, excl))
        e.close()


@functools.lru_cache(maxsize=None)
def a2_cml_case(r, arrival):
    """d = 2, U[u] = (a_u, 0), V[j] = (x_j, 0): the score -(a_u - x_j)^2 is an
    integer below 2^24 in the direct and in the expanded form.  a = 0: the
    order of x reversed; a = n - 1: the order of x; a = n / 2: every score has
    a two-sided tie."""
    ni = 64 * 9 + r
    nu = 72
    rng = np.random.RandomState(950 + r)
    x = {"permutation": rng.permutation(ni), "ascending": np.arange(ni), "descending": np.arange(ni)[::-1]}[arrival]
    V = np.zeros((ni, 2), F32)
    V[:, 0] = x
    a = np.array([0, ni - 1, ni // 2, ni // 2 + 1, 1, ni - 2, ni // 3, 5 * ni // 7], np.float64)
    U = np.zeros((nu, 2), F32)
    U[:, 0] = a[np.arange(nu) % len(a)]
    users = np.arange(nu, dtype=np.int32)
    S = exact_scores("cml", U, V, None, users)
    rows = []
    for u in range(nu):
        top = np.argsort(-S[u], kind="stable")
        q = u // len(a)
        rows.append(np.sort([np.zeros(0, np.int64), top[0:128:3], top[:40]][q % 3]))
    return U, V, rows, users, S


@pytest.mark.parametrize("r", [0, 1, 37])
def test_a2_cml_arrival_orders(r):
    for arrival in ("permutation", "ascending", "descending"):
        U, V, rows, users, S = a2_cml_case(r, arrival)
        e = make_engine("cml", U, V, None, rows)
        for k in (1, 28, 29, 100, 128):
            for path in (FUSED, MATERIALISED):
                for excl in (False, True):
                    run_case(e, S, rows, users, k, path, exclude_train=excl, what="cml %s r %d" % (arrival, r))
        e.close()
