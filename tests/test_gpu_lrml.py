"""LRML (src/models/others/models/lrml.py) on the native LRML object
(csrc/cf_lrml.hip) against the float64 CPU model (tests/lrml_model.py, pinned
to autograd of the literal TF graph in tests/test_lrml_model.py).

Tolerances: the per-step loss within 1e-5 relative; U, V and their Adagrad
accumulators inside conftest's default band |gpu - model| <= 1e-6 + 1e-5
|model| on every element after the steps.  The model run in float32 stays
under 0.11 of that band at every shape used here (0.05 on the golden stream,
tests/test_lrml_model.py; 0.105 at the worst edge shape, B = 257, d = 128),
and the init seeds are picked so that the float64 model's min |h| exceeds
1e-4 -- asserted below -- so no row can take the other hinge branch in fp32.
Batches: the reference's own sampler_lrml_ranking stream
(tests/golden/lrml_stream.npz) and synthetic edge batches (hot user, users in
both roles, i = i', neg = pos).
"""
import numpy as np
import pytest
import scipy.sparse as sp

import lrml_cases as C
import lrml_model as LM
from conftest import assert_close

pytestmark = pytest.mark.gpu
TABLES4 = ("user", "item", "acc_user", "acc_item")


def make(tabs, nu, ni, **kw):
    from collaborativefilteringusingtensorflow_amd.lrml import LRMLEngine
    U, V, Key, Mem = tabs
    e = LRMLEngine(nu, ni, U.shape[1], Key.shape[1], **kw)
    for name, t in zip(("user", "item", "key", "memory"), tabs):
        e.set_table(name, t)
    return e


def run_parity(tabs, batches, nu, ni, what):
    T, losses, hs = C.run_model(tabs, batches, np.float64)
    assert C.min_abs_h(hs) > C.H_MIN, (what, C.min_abs_h(hs))
    e = make(tabs, nu, ni)
    worst = 0.0
    for s, (pos, neg) in enumerate(batches):
        lg = e.step(pos, neg)
        print("%s step %d: loss gpu %.9g model %.9g" % (what, s, lg, losses[s]))
        assert abs(lg - losses[s]) <= 1e-5 * abs(losses[s]), (what, s, lg, losses[s])
    for name in TABLES4:
        worst = max(worst, assert_close(e.get_table(name), T[name], "%s %s" % (what, name)))
    for name in ("key", "memory"):   # never trained (lrml.py:114)
        assert np.array_equal(e.get_table(name), tabs[2 if name == "key" else 3])
    print("%s: worst |d| / band %.3f, active %.3f" % (what, worst, np.mean([np.mean(h > 0) for h in hs])))
    return e, T, hs


@pytest.mark.parametrize("stddev", [0.01, 0.3])
@pytest.mark.parametrize("d,M", [(50, 20), (100, 20), (20, 1), (128, 64)])
def test_lrml_step_parity_on_the_reference_stream(d, M, stddev):
    pos, neg = C.stream()
    batches = list(zip(pos[:10], neg[:10]))
    tabs = C.init_tables(C.INIT_SEEDS[(d, M, stddev)], C.NU, C.NI, d, M, stddev)
    e, _, hs = run_parity(tabs, batches, C.NU, C.NI, "d=%d M=%d sd=%g" % (d, M, stddev))
    if stddev == 0.3:
        assert 0.2 < np.mean([np.mean(h <= 0) for h in hs]) < 0.6   # both hinge branches
    e.close()


@pytest.mark.parametrize("d", [1, 17, 33, 128])
@pytest.mark.parametrize("B", [1, 63, 257])
def test_lrml_edge_shapes(B, d):
    tabs, batches = C.edge_case(B, d)
    nu, ni = C.EDGE_NU, C.EDGE_NI
    # rows no batch after the first touches: bit-identical after the first step's clip
    e = make(tabs, nu, ni)
    e.step(*batches[0])
    first = {n: e.get_table(n) for n in TABLES4}
    for pos, neg in batches[1:]:
        e.step(pos, neg)
    later_u = np.unique(np.concatenate([np.r_[p[:, 0], n[:, 0]] for p, n in batches[1:]]))
    later_i = np.unique(np.concatenate([np.r_[p[:, 1], n[:, 1]] for p, n in batches[1:]]))
    for name, touched, rows in (("user", later_u, nu), ("item", later_i, ni),
                                ("acc_user", later_u, nu), ("acc_item", later_i, ni)):
        keep = np.setdiff1d(np.arange(rows), touched)
        assert np.array_equal(e.get_table(name)[keep], first[name][keep]), name
    e.close()
    e, _, _ = run_parity(tabs, batches, nu, ni, "edge B=%d d=%d" % (B, d))
    e.close()


def test_lrml_full_clip_once_then_fixed_points():
    nu, ni, d, M = 50, 80, 17, 5
    tabs = C.init_tables(3, nu, ni, d, M, 0.05)
    for t, r0 in ((tabs[0], 40), (tabs[1], 60)):   # rows of norm 3 that no batch touches
        t[r0:] *= 3.0 / np.sqrt((t[r0:].astype(np.float64) ** 2).sum(1, keepdims=True)).astype(np.float32)
    rng = np.random.RandomState(1)
    batches = [(np.stack([rng.randint(0, 10, 20), rng.randint(0, 10, 20)], 1),
                np.stack([rng.randint(0, 10, 20), rng.randint(0, 10, 20)], 1)) for _ in range(2)]
    T, _, _ = C.run_model(tabs, batches[:1], np.float64)
    e = make(tabs, nu, ni)
    e.step(*batches[0])
    one = {n: e.get_table(n) for n in ("user", "item")}
    for name, r0 in (("user", 40), ("item", 60)):
        nrm = np.sqrt((one[name][r0:].astype(np.float64) ** 2).sum(1))
        assert nrm.max() <= 1.0 + 1e-6 and nrm.min() >= 1.0 - 1e-6, (name, nrm.min(), nrm.max())
        assert_close(one[name], T[name], "clip " + name)
    e.step(*batches[1])
    for name, r0 in (("user", 40), ("item", 60)):
        assert np.array_equal(e.get_table(name)[r0:], one[name][r0:]), name
    # set_table arms the full pass again
    e.set_table("item", tabs[1])
    e.step(*batches[1])
    nrm = np.sqrt((e.get_table("item")[60:].astype(np.float64) ** 2).sum(1))
    assert nrm.max() <= 1.0 + 1e-6
    e.close()


def test_lrml_take_loss_sums_the_steps():
    pos, neg = C.stream()
    tabs = C.init_tables(1, C.NU, C.NI, 20, 5, 0.3)
    e = make(tabs, C.NU, C.NI)
    tot = 0.0
    for s in range(5):
        tot += e.step(pos[s], neg[s])
    e.step(pos[5], neg[5], return_loss=False)
    _, losses, _ = C.run_model(tabs, list(zip(pos[:6], neg[:6])), np.float64)
    got = e.take_loss()
    assert abs(got - tot - losses[5]) <= 1e-5 * abs(got)
    assert abs(got - sum(losses)) <= 1e-5 * sum(losses)
    assert e.take_loss() == 0.0
    e.close()


def check_topk(idx, val, S, indptr, indices, users, k, what):
    """Tie-aware, no mismatch budget: ids outside the train row, distinct,
    each with a float64 score >= the float64 k-th best minus the value
    tolerance, and every item beating the k-th best by more than it present."""
    for c, u in enumerate(users):
        s = S[c].copy()
        train = indices[indptr[u]:indptr[u + 1]]
        s[train] = -np.inf
        kth = np.sort(s)[::-1][k - 1]
        tol = 1e-4 * abs(kth)
        ids = idx[c].astype(np.int64)
        assert ids.min() >= 0 and len(set(ids.tolist())) == k, (what, u)
        assert not np.isin(ids, train).any(), (what, u)
        assert (s[ids] >= kth - tol).all(), (what, u, s[ids].min(), kth)
        must = np.nonzero(s > kth + tol)[0]
        assert np.isin(must, ids).all(), (what, u)
        np.testing.assert_allclose(val[c], S[c][ids], rtol=1e-4, atol=0, err_msg="%s user %d" % (what, u))
        assert (np.diff(val[c]) <= 0).all(), (what, u)


@pytest.fixture(scope="module")
def fold_scores(fold1):
    """Tables after ten model steps on the golden stream, and the float64
    scores of every fifth user in both predict modes (computed once)."""
    pos, neg = C.stream()
    tabs = C.init_tables(C.INIT_SEEDS[(50, 20, 0.3)], C.NU, C.NI, 50, 20, 0.3)
    T, _, _ = C.run_model(tabs, list(zip(pos[:10], neg[:10])), np.float64)
    t32 = [T[n].astype(np.float32) for n in ("user", "item", "key", "memory")]
    users = np.arange(0, C.NU, 5, dtype=np.int32)
    t64 = [t.astype(np.float64) for t in t32]
    S = {m: LM.predict(*t64, users, m) for m in ("reference", "train")}
    return t32, users, S


@pytest.mark.parametrize("mode", ["reference", "train"])
def test_lrml_recommend_fold1(fold1, fold_scores, mode):
    t32, users, S = fold_scores
    ip, ix = fold1["train_indptr"], fold1["train_indices"]
    e = make(t32, C.NU, C.NI)
    e.set_interactions(ip, ix)
    for k in (10, 200):
        idx, val = e.score_topk(users, k, predict_mode=mode, return_values=True)
        check_topk(idx, val, S[mode], ip, ix, users, k, "%s k=%d" % (mode, k))
    e.close()


@pytest.mark.parametrize("mode", ["reference", "train"])
def test_lrml_recommend_key_block_tail(mode):
    nu, ni, d, M = 20, 65, 17, 33          # n_items = 64 + 1: the tail of one key block
    tabs = C.init_tables(11, nu, ni, d, M, 0.5)
    rng = np.random.RandomState(2)
    rows = [np.sort(rng.choice(ni, rng.randint(0, 9), replace=False)) for _ in range(nu)]
    rows[0] = np.array([0, 64])            # the first and the last item excluded
    ip = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    ix = np.concatenate(rows).astype(np.int32)
    users = np.arange(nu, dtype=np.int32)
    S = LM.predict(*(t.astype(np.float64) for t in tabs), users, mode)
    e = make(tabs, nu, ni)
    from collaborativefilteringusingtensorflow_amd import _native as N
    with pytest.raises(N.NativeError, match="exclude_train"):
        e.score_topk(users, 5, exclude_train=True)
    e.set_interactions(ip, ix)
    idx, val = e.score_topk(users, 10, predict_mode=mode, return_values=True)
    check_topk(idx, val, S, ip, ix, users, 10, "tail " + mode)
    idx, val = e.score_topk(users, 10, exclude_train=False, predict_mode=mode, return_values=True)
    check_topk(idx, val, S, np.zeros(nu + 1, np.int64), ix[:0], users, 10, "tail no-exclude " + mode)
    e.close()


def test_lrml_rejects_bad_csr():
    from collaborativefilteringusingtensorflow_amd import _native as N
    from test_gpu_ensemble import BAD_CSR
    e = make(C.init_tables(1, 3, 4, 1, 1, 0.1), 3, 4)
    for indptr, indices in BAD_CSR:
        with pytest.raises(N.NativeError, match="CF_EINVAL"):
            e.set_interactions(indptr, indices)
    with pytest.raises(N.NativeError, match="exclude_train"):   # none of them was installed
        e.score_topk(np.array([0]), 2, exclude_train=True)
    e.close()


def test_lrml_rejects_bad_ids():
    from collaborativefilteringusingtensorflow_amd import _native as N
    tabs = C.init_tables(1, 10, 20, 8, 4, 0.1)
    e = make(tabs, 10, 20)
    before = {n: e.get_table(n) for n in TABLES4}
    good = np.array([[0, 1], [2, 3]])
    for pos, neg in ((np.array([[0, 1], [10, 3]]), good), (good, np.array([[0, 20], [2, 3]])),
                     (np.array([[0, -1], [2, 3]]), good), (good, np.array([[-1, 0], [2, 3]]))):
        with pytest.raises(N.NativeError, match="out of range"):
            e.step(pos, neg)
    for n in TABLES4:
        assert np.array_equal(e.get_table(n), before[n]), n
    with pytest.raises(N.NativeError, match="out of range"):
        e.score_topk(np.array([10]), 5, exclude_train=False)
    with pytest.raises(ValueError):
        e.score_topk(np.array([0]), 5, exclude_train=False, predict_mode="x")
    e.step(good, good)   # and a good batch still runs
    e.close()


def _matrices(f):
    tra = sp.csr_matrix((np.ones(len(f["train_indices"])), f["train_indices"], f["train_indptr"]),
                        shape=(943, 1682))
    tst = sp.csr_matrix((np.ones(len(f["test_indices"])), f["test_indices"], f["test_indptr"]),
                        shape=(943, 1682))
    return tra, tst


def test_lrml_train_loop(fold1):
    """LRML.train on ml-100k fold 1 with the exact reference stream, one
    epoch (five sampler epochs of steps): finite scores, precision far above random (the
    Ensemble test's bar; the numpy model reaches pre@10 = 0.103, loss 9.98)."""
    from collaborativefilteringusingtensorflow_amd.lrml import LRML
    from collaborativefilteringusingtensorflow_amd.sampler_lrml_ranking import ExactSampler
    tra, tst = _matrices(fold1)
    sampler = ExactSampler(tra, batch_size=100, seed=0)
    m = LRML(943, 1682, 10, 'cv', ['pre', 'recall', 'map', 'mrr', 'ndcg'], n_factors=20, max_iter=1,
             device=0, seed=3)
    scores = m.train(1, tra, tst, sampler)
    assert np.all(np.isfinite(scores))
    assert scores[0] > 0.05, scores
    assert sampler.state() == (5, 0)       # 5 * int(nnz / B) batches: five sampler epochs
    m.close()
    sampler.close()


def test_lrml_driver_worker_end_to_end(fold1, tmp_path):
    """The testlrml-structured driver: text folds -> loadSparseR ->
    matBinarize -> Sampler -> LRML.train -> scores (testlrml.py:32-55)."""
    from collaborativefilteringusingtensorflow_amd.drivers import testlrml
    for tag in ("train", "test"):
        ip, ix = fold1[tag + "_indptr"], fold1[tag + "_indices"]
        name = "ratings__1_%s.txt" % ("tra" if tag == "train" else "tst")
        with open(tmp_path / name, "w") as f:
            for u in range(943):
                for it in ix[ip[u]:ip[u + 1]]:
                    f.write("%d\t%d\t4.0\n" % (u, it))
    old = testlrml.max_iter
    testlrml.max_iter = 1
    try:
        scores = testlrml.worker(0, 943, 1682, str(tmp_path) + "/")
    finally:
        testlrml.max_iter = old
    assert len(scores) == 5 and np.all(np.isfinite(scores)) and scores[0] > 0.05, scores
