"""PopRank, UserCF, ItemCF and UserItemCF on the native neighbourhood object
(csrc/cf_knn.hip) against the host model (tests/knn_model.py, pinned to the
reference's own output in tests/test_knn_model.py).

Everything is compared in bits: the similarities are two IEEE divisions of an
integer count, the predictions are float64 sums of float32 terms whose order
the kernels fix (the fixtures additionally satisfy the precondition under
which any order gives the same float64, asserted in test_knn_model.py), and
the tie rule -- lower id first -- is this project's on both sides.

Fixture cases (tests/golden/knn_*.npz): similarity bits, neighbour tables on
every row (tied rows included), predictions from the reference's own cut
matrices against the reference's float64 vectors, the top-k values against
float32(prediction), the ids through oracle/topk_check.check_lists with a
bound of half a float32 ulp per score and at most 5 % mismatched positions
(outright equality with the reference's lists where K exceeds every row's
positives), and the drop-ins' scores to 1e-12 there.

Edge shapes (knn_cases.edge_matrix): 2x2, 63x65, 64x64, 65x63, 257x300 with
the LDS tiles at their default, 64 and 128 wide -- one tile, two tiles, a
partial last tile, members on both sides of a tile edge -- an empty user, a
user holding every item, identical rows and columns, an item every user
holds; topK in {1, 8, n - 1, n, n + 5} for n of both sides; recommend k in
{1, 5, n_items}; users repeated and unsorted; exclude_train on and off.  The
empty item has a matrix of its own (test_empty_item): a user cannot hold every
item while one item is held by nobody.

Measured on an MI355X: every comparison is of bits and none differed; the
fixture lists had 2 of 115 positions (UserCF, 97x131, K = 8) inside the
half-ulp near-tie width and none elsewhere.
"""
import ctypes
import functools

import numpy as np
import pytest
from scipy.sparse import lil_matrix

import knn_cases as C
import knn_model as M
from oracle.topk_check import check_lists

from collaborativefilteringusingtensorflow_amd import _native as N
from collaborativefilteringusingtensorflow_amd._knn import KnnEngine

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def engine(R, kind, topK, theta=0.0, tile=0):
    e = KnnEngine(R.shape[0], R.shape[1], kind, topK, theta)
    e.set_option("tile_cols", tile)
    e.set_option("tile_items", tile)
    e.set_interactions(*C.csr(R))
    return e


def assert_tables(got, want, what):
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(bits(got[1]), bits(want[1])), what


def oracle_lists(pred, R, users, k):
    """Top-k of the float64 predictions, ties to the lower id, train items skipped."""
    R = np.asarray(R) != 0
    ids = np.arange(R.shape[1])
    out = []
    for row, u in enumerate(users):
        order = np.lexsort((ids, -pred[row]))
        out.append([int(i) for i in order[~R[u, order]][:k]])
    return out


@pytest.mark.parametrize("name", C.CASES)
def test_fixture_similarity_and_neighbours(name):
    c = C.load(name)
    S, nb = C.model_fit(name)
    e = engine(c["R"], "useritem", c["topK"], c["theta"])
    try:
        for side, key in ((0, "user"), (1, "item")):
            got = e.similarity(key, np.arange(S[side].shape[0]))
            assert np.array_equal(bits(got), bits(S[side])), key
        e.fit()
        for side, key in ((0, "user"), (1, "item")):
            assert_tables(e.get_neighbours(key), nb[side], key)
    finally:
        e.close()


@pytest.mark.parametrize("model", sorted(C.REF_MODELS))
@pytest.mark.parametrize("name", C.CASES)
def test_fixture_predictions_and_lists(name, model):
    c = C.load(name)
    kind, users, k = C.REF_MODELS[model], c["test_users"], c["topN"]
    nb_user, nb_item = C.ref_tables(name, model)
    ref = c[model + "_pred"]
    e = engine(c["R"], kind, c["topK"], c["theta"])
    try:
        if nb_user is not None:
            e.set_neighbours("user", *nb_user)
        if nb_item is not None:
            e.set_neighbours("item", *nb_item)
        pred = e.predict(users)
        assert np.array_equal(pred.view(np.uint64), ref.view(np.uint64))
        idx, val = e.score_topk(users, k, exclude_train=True, return_values=True)
    finally:
        e.close()
    filled = idx >= 0
    rows = np.nonzero(filled)[0]
    assert np.array_equal(bits(val[filled]), bits(ref[rows, idx[filled]].astype(np.float32)))
    assert np.isnan(val[~filled]).all()
    half_ulp = 0.5 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    excluded = [np.nonzero(c["R"][u])[0] for u in users]
    bad, total = check_lists(idx, ref, oracle_lists(ref, c["R"], users, k), np.inf, bound=half_ulp,
                             excluded=excluded)
    print(name, model, "mismatched positions %d of %d" % (bad, total))
    assert bad <= 0.05 * total
    if name == C.FULL_CASE:
        assert np.array_equal(idx, c[model + "_lists"])


@pytest.mark.parametrize("name", C.CASES)
def test_fixture_poprank(name):
    c = C.load(name)
    e = engine(c["R"], "pop", 1)
    try:
        e.fit()
        idx = e.score_topk(c["test_users"], c["topN"])
    finally:
        e.close()
    assert np.array_equal(idx, c["pop_lists"])


def test_dropins_reproduce_reference_scores():
    from collaborativefilteringusingtensorflow_amd.itemcf import ItemCF
    from collaborativefilteringusingtensorflow_amd.pop import PopRank
    from collaborativefilteringusingtensorflow_amd.usercf import UserCF
    from collaborativefilteringusingtensorflow_amd.useritemcf import UserItemCF
    c = C.load(C.FULL_CASE)
    nu, ni = c["R"].shape
    tra, tst = lil_matrix(c["R"].astype(np.float32)), lil_matrix(c["T"].astype(np.float32))
    K, topN = c["topK"], c["topN"]
    models = {"pop": PopRank(nu, ni, topN, 'cv', C.METRICS),
              "ucf": UserCF(nu, ni, K, topN, 'cv', C.METRICS),
              "icf": ItemCF(nu, ni, K, topN, 'cv', C.METRICS),
              "uicf": UserItemCF(nu, ni, K, c["theta"], topN, 'cv', C.METRICS)}
    for name, m in models.items():
        scores = m.train(1, tra, tst)
        m.close()
        m.close()   # twice: the second is a no-op
        assert np.allclose(scores, c[name + "_scores"], rtol=0, atol=1e-12), name


def test_dropin_refuses_weighted_ratings_and_bad_tables():
    from collaborativefilteringusingtensorflow_amd.usercf import UserCF
    c = C.load(C.FULL_CASE)
    nu, ni = c["R"].shape
    m = UserCF(nu, ni, 8, 5, 'cv', C.METRICS)
    with pytest.raises(ValueError, match="binarised"):
        m.train(1, lil_matrix(c["R"].astype(np.float32) * 2.0), lil_matrix(c["T"].astype(np.float32)))
    m.close()
    e = engine(c["R"], "user", 4)
    try:
        L = N.lib()
        assert L.cf_knn_set_interactions(e._h, None, None, 0) == -1 and b"null CSR" in L.cf_last_error()
        with pytest.raises(N.NativeError, match="cf_knn_fit"):
            e.predict([0])   # CF_ESTATE: no table yet
        with pytest.raises(N.NativeError, match="keeps no neighbour table"):
            e.get_neighbours("item")
        idx = np.full((nu, 4), -1, dtype=np.int32)
        sim = np.zeros((nu, 4), dtype=np.float32)
        idx[3, :2] = (nu, 1)
        with pytest.raises(N.NativeError, match="out of range"):
            e.set_neighbours("user", idx, sim)
        idx[3, :2] = (1, 1)
        with pytest.raises(N.NativeError, match="repeated"):
            e.set_neighbours("user", idx, sim)
        idx[3, :2] = (1, -1)
        e.set_neighbours("user", idx, sim)
        assert not e.predict([3, 0]).any()   # zero weights: zero predictions
        for name in ("tile_cols", "tile_items"):
            with pytest.raises(N.NativeError, match=name):
                e.set_option(name, 1 << 20)
        with pytest.raises(N.NativeError, match="unknown option"):
            e.set_option("tile", 64)
    finally:
        e.close()


# ---- edge shapes ---------------------------------------------------------------

SHAPES = [(2, 2), (63, 65), (64, 64), (65, 63), (257, 300)]
TILES = [0, 64, 128]


@functools.lru_cache(maxsize=None)
def edge(shape):
    R = C.edge_matrix(*shape)
    return R, (M.similarity(R, 0), M.similarity(R, 1))


@functools.lru_cache(maxsize=None)
def edge_neighbours(shape, side, topK):
    return M.neighbours(edge(shape)[1][side], topK)


def edge_users(n_users):
    u = [n_users - 1, 0, 1, 5, 2, 5, 7, 6, n_users - 1]   # repeated and unsorted
    return np.asarray([x for x in u if x < n_users], dtype=np.int32)


def edge_topks(shape):
    ks = {1, 8}
    for n in shape:
        ks |= {n - 1, n, n + 5}
    return sorted(k for k in ks if k >= 1)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_edge_shapes(shape, tile):
    R, S = edge(shape)
    n_users, n_items = shape
    users = edge_users(n_users)
    theta = 0.8
    e = engine(R, "pop", 1, tile=tile)
    try:
        for side, key in ((0, "user"), (1, "item")):   # any kind serves similarity rows
            rows = np.arange(S[side].shape[0])[::-1]
            got = e.similarity(key, rows)
            assert np.isfinite(got).all()
            assert np.array_equal(bits(got), bits(S[side][rows])), key
        pred = M.predict("pop", R, users)
        assert np.array_equal(e.predict(users), pred)
        for k in (1, 5, n_items):
            for ex in (True, False):
                idx, val = e.score_topk(users, k, exclude_train=ex, return_values=True)
                want = M.recommend(pred, R, users, k, ex)
                assert np.array_equal(idx, want[0]) and np.array_equal(bits(val), bits(want[1])), ("pop", k, ex)
    finally:
        e.close()
    for topK in edge_topks(shape):
        nb = (edge_neighbours(shape, 0, topK), edge_neighbours(shape, 1, topK))
        for kind in ("user", "item", "useritem"):
            nb_user = nb[0] if kind != "item" else None
            nb_item = nb[1] if kind != "user" else None
            e = engine(R, kind, topK, theta, tile)
            try:
                e.fit()
                if nb_user is not None:
                    assert_tables(e.get_neighbours("user"), nb_user, (kind, topK, "user"))
                if nb_item is not None:
                    assert_tables(e.get_neighbours("item"), nb_item, (kind, topK, "item"))
                pred = M.predict(kind, R, users, nb_user, nb_item, theta)
                got = e.predict(users)
                assert np.isfinite(got).all()
                assert np.array_equal(got.view(np.uint64), pred.view(np.uint64)), (kind, topK)
                assert not got[users == 0].any()   # the empty user (2 x 2: every item is empty too)
                for k in (1, 5, n_items):
                    for ex in (True, False):
                        idx, val = e.score_topk(users, k, exclude_train=ex, return_values=True)
                        want = M.recommend(pred, R, users, k, ex)
                        assert np.array_equal(idx, want[0]), (kind, topK, k, ex)
                        assert np.array_equal(bits(val), bits(want[1])), (kind, topK, k, ex)
                        if ex:   # the user holding every item: nothing left, all pads
                            assert (idx[users == 1] == -1).all() and np.isnan(val[users == 1]).all()
            finally:
                e.close()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_empty_item(shape):
    """An item nobody holds (den = 0): similarity 0 to everything, no neighbours, prediction 0, no NaN;
    it is all that is left to recommend to the user who holds every other item."""
    R = C.edge_matrix(*shape, empty_item=True)
    n_users, n_items = shape
    j = int(np.nonzero(R.sum(0) == 0)[0][0])
    users = edge_users(n_users)
    S = (M.similarity(R, 0), M.similarity(R, 1))
    nb = (M.neighbours(S[0], 8), M.neighbours(S[1], 8))
    e = engine(R, "useritem", 8, 0.8, tile=64)
    try:
        got = e.similarity("item", np.arange(n_items))
        assert np.isfinite(got).all() and not got[j].any() and not got[:, j].any()
        assert np.array_equal(bits(got), bits(S[1]))
        e.fit()
        assert_tables(e.get_neighbours("user"), nb[0], "user")
        assert_tables(e.get_neighbours("item"), nb[1], "item")
        assert (e.get_neighbours("item")[0][j] == -1).all()
        pred = M.predict("useritem", R, users, nb[0], nb[1], 0.8)
        got = e.predict(users)
        assert np.array_equal(got.view(np.uint64), pred.view(np.uint64)) and not got[:, j].any()
        idx, val = e.score_topk(users, n_items, exclude_train=True, return_values=True)
        want = M.recommend(pred, R, users, n_items, True)
        assert np.array_equal(idx, want[0]) and np.array_equal(bits(val), bits(want[1]))
        assert (idx[users == 1, 0] == j).all() and (idx[users == 1, 1:] == -1).all()
    finally:
        e.close()


def test_identical_rows_and_ties():
    """Identical rows lead each other's lists; among equal similarities the lower id leads.
    Their similarity is fl32(fl32(n / den) / den) with den = fl32(sqrt(n)): 1.0 up to one
    rounding of each division (0.9999999 at n = 23, 1.0 at n = 22), the bits the reference has."""
    shape = (65, 63)
    R, S = edge(shape)
    e = engine(R, "user", 8, tile=64)
    try:
        e.fit()
        idx, sim = e.get_neighbours("user")
    finally:
        e.close()
    for a, b in ((2, 5), (6, 7), (6, 64), (7, 64)):
        assert abs(float(S[0][a, b]) - 1.0) <= 2.0 ** -23 and S[0][a, b] == S[0][a].max()
    assert S[0][6, 7] == S[0][6, 64] == S[0][7, 64]
    assert idx[2, 0] == 5 and bits(sim[2, 0]) == bits(S[0][2, 5]) and idx[5, 0] == 2
    assert list(idx[6, :2]) == [7, 64] and list(idx[7, :2]) == [6, 64] and list(idx[64, :2]) == [6, 7]
    assert (idx[0] == -1).all() and not sim[0].any()   # the empty user has no neighbours


def test_two_runs_return_identical_bytes():
    shape = (257, 300)
    R, _ = edge(shape)
    users = edge_users(shape[0])
    e = engine(R, "useritem", 32, 0.8, tile=128)
    try:
        runs = []
        for _ in range(2):
            e.fit()
            out = [a.tobytes() for side in ("user", "item") for a in e.get_neighbours(side)]
            for _ in range(2):
                idx, val = e.score_topk(users, 5, exclude_train=True, return_values=True)
                out += [idx.tobytes(), val.tobytes(), e.predict(users).tobytes()]
            assert out[4:7] == out[7:10]
            runs.append(out)
        assert runs[0] == runs[1]
    finally:
        e.close()
