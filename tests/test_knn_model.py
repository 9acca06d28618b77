"""The host model of the neighbourhood family (tests/knn_model.py) against the
reference's own output (tests/golden/knn_*.npz, written by
tests/golden/make_knn_golden.py from pop.py, usercf.py, itemcf.py and
useritemcf.py on the CPU), and the ``cf_knn_*`` ABI without a device.

The fixture pins the float32 term rule of UserItemCF under the numpy that
wrote it (``numpy_version`` in the file, NEP 50): t1 = fl32(fl32(theta) S_user),
t2 = fl32(fl32(1. - theta) S_item) -- test_predictions_from_reference_lists
holds exactly only under that rule."""
import ctypes

import numpy as np
import pytest

import knn_cases as C
import knn_model as M
from collaborativefilteringusingtensorflow_amd import _native as N
from collaborativefilteringusingtensorflow_amd.ranking import evaluateCV


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("name", C.CASES)
def test_similarity_bits(name):
    c = C.load(name)
    S, _ = C.model_fit(name)
    assert np.array_equal(bits(S[0]), bits(c["sim_user"]))
    assert np.array_equal(bits(S[1]), bits(c["sim_item"]))
    for s in S:
        assert np.array_equal(bits(s), bits(s.T)) and not s.diagonal().any()


@pytest.mark.parametrize("name", C.CASES)
def test_neighbours_on_untied_rows(name):
    c = C.load(name)
    K = c["topK"]
    S, nb = C.model_fit(name)
    # the reference's cut rows per side; UserItemCF's equal UserCF's / ItemCF's where no tie decides
    for side, cut in ((0, ("ucf_topk", "uicf_user_topk")), (1, ("icf_topk", "uicf_item_topk"))):
        tied = M.tied_rows(S[side], K)
        print(name, "side", side, "tied rows: %.1f %%" % (100.0 * tied.mean()))
        assert tied.mean() <= 0.20, "fixture condition: at most 20 % of a side's rows tied"
        idx, sim = nb[side]
        n = S[side].shape[0]
        mine = np.zeros((n, n), dtype=np.float32)
        rows = np.repeat(np.arange(n), K)[idx.ravel() >= 0]
        mine[rows, idx.ravel()[idx.ravel() >= 0]] = sim.ravel()[idx.ravel() >= 0]
        for key in cut:
            assert np.array_equal(bits(mine[~tied]), bits(c[key][~tied])), key
        if name == C.FULL_CASE:
            assert not tied.any()


def user_term_stats(c, kind, nb_user, nb_item, u):
    """Every float32 term the user's prediction adds, and the most terms one cell can take."""
    R = c["R"] != 0
    terms, count = [], 0
    if nb_user is not None:
        t = M.user_terms(kind, c["theta"], nb_user[1][u])[nb_user[0][u] >= 0]
        terms.append(t)
        count += t.size
    if nb_item is not None:
        for i in np.nonzero(R[u])[0]:
            terms.append(M.item_terms(kind, c["theta"], nb_item[1][i])[nb_item[0][i] >= 0])
        count += int(R[u].sum())
    return np.concatenate(terms) if terms else np.zeros(0, np.float32), count


@pytest.mark.parametrize("model", sorted(C.REF_MODELS))
@pytest.mark.parametrize("name", C.CASES)
def test_predictions_from_reference_lists(name, model):
    c = C.load(name)
    kind = C.REF_MODELS[model]
    nb_user, nb_item = C.ref_tables(name, model)
    users = c["test_users"]
    for u in users:   # the precondition that makes every sum exact in any order
        t, count = user_term_stats(c, kind, nb_user, nb_item, u)
        t = t[t != 0].astype(np.float64)
        if t.size:
            e = np.frexp(t)[1]
            assert int(e.max() - e.min()) + int(np.ceil(np.log2(max(count, 1)))) + 24 <= 53, (name, model, u)
    pred = M.predict(kind, c["R"], users, nb_user, nb_item, c["theta"])
    assert pred.dtype == np.float64
    assert np.array_equal(pred.view(np.uint64), c[model + "_pred"].view(np.uint64))


def scores_of(c, lists):
    T = c["T"] != 0
    truth = [set(np.nonzero(T[u])[0].tolist()) for u in c["test_users"]]
    return evaluateCV(truth, [[int(x) for x in row if x >= 0] for row in lists], C.METRICS, c["topN"])


@pytest.mark.parametrize("model", sorted(C.REF_MODELS))
def test_end_to_end_lists_and_scores(model):
    c = C.load(C.FULL_CASE)
    kind = C.REF_MODELS[model]
    nb_user, nb_item = M.fit(kind, c["R"], c["topK"])
    pred = M.predict(kind, c["R"], c["test_users"], nb_user, nb_item, c["theta"])
    idx, _ = M.recommend(pred, c["R"], c["test_users"], c["topN"])
    assert np.array_equal(idx, c[model + "_lists"])
    assert np.allclose(scores_of(c, idx), c[model + "_scores"], rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", C.CASES)
def test_poprank_lists_and_scores(name):
    c = C.load(name)
    pred = M.predict("pop", c["R"], c["test_users"])
    idx, _ = M.recommend(pred, c["R"], c["test_users"], c["topN"])
    assert np.array_equal(idx, c["pop_lists"])
    assert np.allclose(scores_of(c, idx), c["pop_scores"], rtol=0, atol=1e-12)


def test_abi_without_a_device():
    L = N.lib()
    h = ctypes.c_void_p()

    def create(kind=N.CF_KNN_USER, topK=8, theta=0.5, n_users=10, n_items=12):
        return L.cf_knn_create(n_users, n_items, kind, topK, theta, 0, ctypes.byref(h))

    for bad in (dict(kind=-1), dict(kind=4), dict(topK=0), dict(topK=4097), dict(theta=-0.01), dict(theta=1.01),
                dict(theta=float("nan")), dict(n_users=0), dict(n_items=0)):
        assert create(**bad) == -1, bad   # CF_EINVAL, before any device is looked for
    assert b"topK" in (create(topK=0), L.cf_last_error())[1]
    assert b"theta" in (create(theta=2.0), L.cf_last_error())[1]
    assert L.cf_knn_set_interactions(None, None, None, 0) == -1
    assert b"null CSR" in L.cf_last_error()
    # the neighbour-table check of cf_knn_set_neighbours, which needs no object
    idx = np.array([[1, 2, -1], [0, 2, -1], [0, 1, -1]], dtype=np.int32)
    sim = np.array([[.5, .25, 0], [.5, .25, 0], [.25, .25, 0]], dtype=np.float32)

    def check(i, s):
        return L.cf_knn_check_neighbours(3, 3, N._ptr(i, ctypes.c_int32), N._ptr(s, ctypes.c_float))

    assert check(idx, sim) == 0
    for r, n, v, what in ((0, 1, 3, b"out of range"), (1, 2, -2, b"out of range"), (2, 2, 0, b"repeated")):
        broken = idx.copy()
        broken[r, n] = v
        assert check(broken, sim) == -1 and what in L.cf_last_error(), (r, n, v)
    assert L.cf_knn_set_neighbours(None, 0, N._ptr(idx, ctypes.c_int32), N._ptr(sim, ctypes.c_float)) == -1
    if N.device_count() > 0:
        return
    assert create() == -2   # CF_EHIP: no CPU fallback
    assert b"no HIP device" in L.cf_last_error()
    from collaborativefilteringusingtensorflow_amd.usercf import UserCF
    from scipy.sparse import lil_matrix
    R = lil_matrix(np.eye(4, 5, dtype=np.float32))
    with pytest.raises(N.NativeError, match="no HIP device"):
        UserCF(4, 5, topK=2, eval_metrics=C.METRICS).train(1, R, R)


def test_dropins_refuse_weighted_ratings():
    from collaborativefilteringusingtensorflow_amd.itemcf import ItemCF
    from scipy.sparse import lil_matrix
    R = lil_matrix(np.eye(4, 5, dtype=np.float32) * 3.0)
    with pytest.raises(ValueError, match="binarised"):
        ItemCF(4, 5, topK=2, eval_metrics=C.METRICS).train(1, R, lil_matrix(np.eye(4, 5, dtype=np.float32)))
