"""MF, SVD and WRMF (src/models/basic/models/mf.py, svd.py, wrmf.py) on the
native pointwise object (csrc/cf_pointwise.hip) against the float64 CPU model
(tests/pointwise_model.py, pinned to autograd of the literal TF graphs in
tests/test_pointwise_model.py).  There is no hinge: no row is ever excluded.

Parity is judged twice per case.

* Step-local (as conftest.LocalStepCheck): before each step the engine's own
  float32 tables are read, the float64 model runs one step from exactly those
  tables, and every element of U, V, AU, AV (SVD: K, AK) must lie inside
  conftest's default band ATOL + RTOL |model|, the loss within 1e-5 relative,
  rows the batch does not touch bit-identical.  A hot row's float32 sum of
  n <= 257 terms rounds at about sqrt(n) 2^-24, well inside 1e-5.
* End of trajectory: the float32 run of the same numpy model leaves the
  default band around the float64 run on hot-user shapes (measured on the CPU,
  worst |d| / band: up to 4.13 at the edge shapes (SVD, B = 257, d = 128; 1.46 at B = 63; MF stays under 0.66), up to 1.82 on the golden
  streams (SVD at d = 100; under 0.38 at the three driver shapes)), so each case computes that ratio on the CPU -- float32 model against
  float64 model, never against the GPU -- and holds the GPU to
  max(1, 2 x ratio) default bands (the factor 2: CML_TRAJ and ENS_HOT in
  conftest keep the float32 oracle under 0.5 of their bands).

Measured on an MI355X, worst |d| / band (step-local; end, allowed): golden
streams MF d = 100 0.145; 0.164 (1.00), MF d = 20 0.111; 0.122 (1.00), SVD
d = 32 0.115; 0.777 (1.00), SVD d = 100 0.353; 1.725 (3.63), WRMF 0.109; 0.123
(1.00); edge shapes MF at most 0.235; 0.399 (B = 257, d = 33: 1.31), SVD at
most 0.924 (B = 257, d = 128); 1.801 (8.26) and 1.668 (B = 63, d = 128: 2.91);
d = 64 with B = 8,208, 8,192, 100 on one object MF 0.072; 0.103 (1.00), SVD
0.139; 0.236 (1.30).

Batches: the reference's own sampler_rating streams
(tests/golden/rating_stream.npz: about two users per hundred rows at negRatio
0, half uniform negatives at negRatio 1) and synthetic edge batches (one user
in a third of the rows, one batch a single user throughout, an item repeated
under different users, an exact duplicate row) at B in {1, 63, 257} and d in
{1, 17, 33, 128}: the 16-lane slot counts, the MFMA tile edges in d and B, a
tile boundary inside a user run, K at its LDS maximum.

Train loops, one epoch on fold 1 from ExactSampler(seed=0) and init seed 11,
scored on the committed tenth of the test tuples;
the float64 model over the same stream gives MF (d 100, B 1000) rmse 2.7145,
SVD (d 32, B 100) rmse 2.0098, WRMF (d 100, B 100 + 100) pre@10 0.0397.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import pointwise_cases as C
import pointwise_model as PM
from conftest import ATOL, RTOL, assert_close

pytestmark = pytest.mark.gpu


def make(kind, T, nu, ni, **kw):
    from collaborativefilteringusingtensorflow_amd._pointwise import PointwiseEngine
    e = PointwiseEngine(nu, ni, T["user"].shape[1], kind=kind, weight=C.WEIGHT[kind], reg=C.REG, lr=C.LR, **kw)
    for name in C.tables_names(kind):
        e.set_table(name, T[name])
    return e


def run_parity(kind, T0, batches, nu, ni, what):
    names = C.tables_names(kind)
    limit = max(1.0, 2.0 * C.fp32_ratio(kind, T0, batches))
    T64, _ = C.run_model(kind, T0, batches, np.float64)
    e = make(kind, T0, nu, ni)
    worst_local = 0.0
    for s, (ui, r) in enumerate(batches):
        L = {n: e.get_table(n) for n in names}
        M = C.cast(L, np.float64)
        lo = PM.step(kind, M, ui, r, C.REG, C.LR, C.WEIGHT[kind])
        lg = e.step(ui, r)
        assert abs(lg - lo) <= 1e-5 * abs(lo), (what, s, lg, lo)
        for n in names:
            got = e.get_table(n)
            worst_local = max(worst_local, assert_close(got, M[n], "%s step %d local %s" % (what, s, n)))
            if "kernel" not in n:
                keep = np.setdiff1d(np.arange(got.shape[0]), ui[:, 0 if "user" in n else 1])
                assert np.array_equal(got[keep], L[n][keep]), (what, s, n)
    end = {n: e.get_table(n) for n in names}
    e.close()
    worst_end = max(C.band_ratio(end[n], T64[n]) for n in names)
    print("%s: worst |d| / band local %.3f, end %.3f (allowed %.2f)" % (what, worst_local, worst_end, limit))
    for n in names:
        assert_close(end[n], T64[n], "%s end %s" % (what, n), rtol=limit * RTOL, atol=limit * ATOL)


@pytest.mark.parametrize("kind,d", [("mf", 100), ("mf", 20), ("svd", 32), ("svd", 100), ("wrmf", 100)])
def test_step_parity_on_the_reference_stream(kind, d):
    ui, r = C.stream(kind)
    T0 = C.init_tables(kind, 7, C.NU, C.NI, d)
    run_parity(kind, T0, list(zip(ui[:10], r[:10])), C.NU, C.NI, "%s d=%d" % (kind, d))


@pytest.mark.parametrize("d", [1, 17, 33, 128])
@pytest.mark.parametrize("B", [1, 63, 257])
@pytest.mark.parametrize("kind", ["mf", "svd"])
def test_edge_shapes(kind, B, d):
    T0, batches = C.edge_case(kind, B, d)
    run_parity(kind, T0, batches, C.EDGE_NU, C.EDGE_NI, "edge %s B=%d d=%d" % (kind, B, d))


@pytest.mark.parametrize("kind", ["mf", "svd"])
def test_batch_size_changes_on_a_live_object(kind):
    """d = 64 fills every slot at four slots per lane (and SVD's Dp = 64, four
    dK tiles per wave).  B = 8,208 is 513 tiles: an SVD block takes two tiles
    and 257 blocks run; B = 8,192 on the same object is 512 blocks of one tile,
    more than the larger batch launched; then a small batch."""
    rng = np.random.RandomState(8)
    T0 = C.init_tables(kind, 5, C.NU, C.NI, 64)
    batches = [(np.stack([rng.randint(0, C.NU, B), rng.randint(0, C.NI, B)], 1).astype(np.int32),
                rng.randint(1, 6, B).astype(np.float32)) for B in (8208, 8192, 100)]
    run_parity(kind, T0, batches, C.NU, C.NI, "%s d=64 B=8208,8192,100" % kind)


def test_svd_two_runs_give_the_same_bits():
    d, B = 33, 300
    rng = np.random.RandomState(4)
    T0 = C.init_tables("svd", 2, C.NU, C.NI, d)
    distinct = [(np.stack([rng.permutation(C.NU)[:B], rng.permutation(C.NI)[:B]], 1).astype(np.int32),
                 rng.randint(1, 6, B).astype(np.float32)) for _ in range(4)]
    ui, r = C.stream("svd")
    for batches in (distinct, list(zip(ui[:4], r[:4]))):     # no duplicated rows; the reference's hot users
        out = []
        for _ in range(2):
            e = make("svd", T0, C.NU, C.NI)
            for b in batches:
                e.step(*b, return_loss=False)
            out.append({n: e.get_table(n) for n in C.tables_names("svd")})
            e.close()
        for n in C.tables_names("svd"):
            assert np.array_equal(out[0][n], out[1][n]), n
        assert not np.array_equal(out[0]["kernel"], T0["kernel"])


@pytest.fixture(scope="module")
def trained():
    """Tables after ten float64 model steps on the golden streams (computed once)."""
    out = {}
    for kind, d in (("mf", 20), ("svd", 32), ("wrmf", 100)):
        ui, r = C.stream(kind)
        T, _ = C.run_model(kind, C.init_tables(kind, 9, C.NU, C.NI, d), list(zip(ui[:10], r[:10])), np.float64)
        out[kind] = C.cast(T, np.float32)
    return out


@pytest.mark.parametrize("kind", ["mf", "svd"])
def test_eval_on_the_test_tuples(trained, kind):
    from collaborativefilteringusingtensorflow_amd import rating as R
    T = trained[kind]
    ui, r = C.tst_tuples()
    assert 1900 <= len(r) <= 2100
    e = make(kind, T, C.NU, C.NI)
    T64 = C.cast(T, np.float64)
    raw = PM.raw_predict(kind, T64["user"], T64["item"], T64.get("kernel"), ui)
    # (1, 5) and (.5, 5): the drivers' ranges, at rtol 1e-5.  Two more: (-10, 10) clips nothing and
    # the last hits both bounds; their unclipped predictions cancel to ~1e-5, so these also get the
    # float32 bound of a dot product of m rounded terms, (m + 1) 2^-24 sum |terms| (m = d, SVD d^2)
    aU, aV = np.abs(T64["user"][ui[:, 0]]), np.abs(T64["item"][ui[:, 1]])
    mag = ((aU @ np.abs(T64["kernel"]) if kind == "svd" else aU) * aV).sum(1)
    m = T["user"].shape[1] ** (2 if kind == "svd" else 1)
    for lo, hi in ((1, 5), (.5, 5), (-10, 10), (float(np.quantile(raw, .3)), float(np.quantile(raw, .7)))):
        atol = 0 if lo > 0 else (m + 1) * 2.0 ** -24 * mag
        for n in (len(r), 0, 1, 17, 1601):
            pred, ab, sq = e.eval(ui[:n], r[:n], lo, hi)
            if n == 0:
                assert ab == 0.0 and sq == 0.0 and pred.shape == (0,)
                continue
            want = np.clip(raw[:n], np.float32(lo), np.float32(hi))
            assert (np.abs(pred - want) <= 1e-5 * np.abs(want) + (atol if lo > 0 else atol[:n])).all(), (lo, hi, n)
            margin = 1e-5 * np.abs(raw[:n]) + (atol if lo > 0 else atol[:n])
            assert (pred[raw[:n] < np.float32(lo) - margin] == np.float32(lo)).all()
            assert (pred[raw[:n] > np.float32(hi) + margin] == np.float32(hi)).all()
            assert pred.min() >= np.float32(lo) and pred.max() <= np.float32(hi)
            mae, mse = R.evaluate(r[:n].astype(np.float64), pred, ["mae", "mse"])
            tol = n * 2.0 ** -53
            assert abs(1 / n * ab - mae) <= tol * mae, (lo, hi, n, ab, mae)
            assert abs(1 / n * sq - mse) <= tol * mse, (lo, hi, n, sq, mse)
            _, ab2, sq2 = e.eval(ui[:n], r[:n], lo, hi, return_pred=False)
            assert (ab2, sq2) == (ab, sq)
    lo, hi = float(np.quantile(raw, .3)), float(np.quantile(raw, .7))
    pred, _, _ = e.eval(ui, r, lo, hi)
    assert (pred == np.float32(lo)).sum() > 100 and (pred == np.float32(hi)).sum() > 100
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


def test_wrmf_recommend_fold1(fold1, trained):
    from collaborativefilteringusingtensorflow_amd import _native as N
    T = trained["wrmf"]
    ip, ix = fold1["train_indptr"], fold1["train_indices"]
    users = np.arange(0, C.NU, 5, dtype=np.int32)
    S = T["user"].astype(np.float64)[users] @ T["item"].astype(np.float64).T
    e = make("wrmf", T, C.NU, C.NI)
    with pytest.raises(N.NativeError, match="exclude_train"):
        e.score_topk(users, 5, exclude_train=True)
    e.set_interactions(ip, ix)
    for k in (10, 200):
        idx, val = e.score_topk(users, k, return_values=True)
        check_topk(idx, val, S, ip, ix, users, k, "wrmf k=%d" % k)
    with pytest.raises(N.NativeError, match="out of range"):
        e.score_topk(np.array([C.NU]), 5, exclude_train=False)
    e.close()
    e = make("svd", trained["svd"], C.NU, C.NI)
    with pytest.raises(N.NativeError, match="CF_EINVAL"):
        e.score_topk(users, 10, exclude_train=False)
    e.close()


def test_pointwise_rejects_bad_csr():
    from collaborativefilteringusingtensorflow_amd import _native as N
    from test_gpu_ensemble import BAD_CSR
    e = make("mf", C.init_tables("mf", 1, 3, 4, 1), 3, 4)
    for indptr, indices in BAD_CSR:
        with pytest.raises(N.NativeError, match="CF_EINVAL"):
            e.set_interactions(indptr, indices)
    with pytest.raises(N.NativeError, match="exclude_train"):   # none of them was installed
        e.score_topk(np.array([0]), 2, exclude_train=True)
    e.close()


@pytest.mark.parametrize("kind", ["mf", "svd"])
def test_bad_inputs_leave_the_tables_untouched(kind):
    from collaborativefilteringusingtensorflow_amd import _native as N
    T0 = C.init_tables(kind, 1, 10, 20, 8)
    e = make(kind, T0, 10, 20)
    names = C.tables_names(kind)
    good_ui, good_r = np.array([[0, 1], [2, 3]]), np.array([4.0, 1.0])
    for ui in ([[0, 1], [10, 3]], [[0, 20], [2, 3]], [[0, -1], [2, 3]], [[-1, 0], [2, 3]]):
        with pytest.raises(N.NativeError, match="out of range"):
            e.step(np.array(ui), good_r)
        with pytest.raises(N.NativeError, match="out of range"):
            e.eval(np.array(ui), good_r, 1, 5)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(N.NativeError, match="not finite"):
            e.step(good_ui, np.array([4.0, bad]))
    for n in names:
        assert np.array_equal(e.get_table(n), T0[n]), n
    if kind == "mf":       # K tables on an MF object
        a = np.zeros((8, 8), np.float32)
        with pytest.raises(N.NativeError, match="CF_EINVAL"):
            e.set_table("kernel", a)
        with pytest.raises(N.NativeError, match="CF_EINVAL"):
            e.get_table("acc_kernel")
    lo = e.step(good_ui, good_r)      # and a good batch still runs
    M = C.cast(T0, np.float64)
    assert abs(lo - PM.step(kind, M, good_ui, good_r, C.REG, C.LR)) <= 1e-5 * lo
    e.close()


def test_take_loss_sums_the_steps():
    ui, r = C.stream("mf")
    T0 = C.init_tables("mf", 1, C.NU, C.NI, 20)
    e = make("mf", T0, C.NU, C.NI)
    tot = sum(e.step(ui[s], r[s]) for s in range(5))
    e.step(ui[5], r[5], return_loss=False)
    _, losses = C.run_model("mf", T0, list(zip(ui[:6], r[:6])), np.float64)
    got = e.take_loss()
    assert abs(got - tot - losses[5]) <= 1e-5 * abs(got)
    assert abs(got - sum(losses)) <= 1e-5 * sum(losses)
    assert e.take_loss() == 0.0
    e.close()


def model_epoch(kind, d, B, tra, neg):
    """The float64 model over the stream MF/SVD/WRMF.train consumes."""
    from collaborativefilteringusingtensorflow_amd.sampler_rating import ExactSampler
    s = ExactSampler(tra, negRatio=neg, batch_size=B, seed=0)
    T0 = C.init_tables(kind, 11, C.NU, C.NI, d)
    T = C.cast(T0, np.float64)
    for _ in range(tra.nnz // B):
        ui, r = s._draw()
        PM.step(kind, T, ui, r, C.REG, C.LR, C.WEIGHT[kind])
    s.close()
    return T0, T


@pytest.mark.parametrize("kind,d,B", [("mf", 100, 1000), ("svd", 32, 100)])
def test_rating_train_loop(kind, d, B):
    from collaborativefilteringusingtensorflow_amd import rating as R
    from collaborativefilteringusingtensorflow_amd.mf import MF
    from collaborativefilteringusingtensorflow_amd.sampler_rating import ExactSampler
    from collaborativefilteringusingtensorflow_amd.svd import SVD
    tra = C.raw_train()
    tst_ui, tst_r = C.tst_tuples()
    T0, T = model_epoch(kind, d, B, tra, .0)
    want = R.evaluate(tst_r.astype(np.float64),
                      PM.predict(kind, T["user"], T["item"], T.get("kernel"), tst_ui, 1, 5), ["rmse"])[0]
    coo = tra.tocoo()
    tra_tuple = np.stack([coo.row, coo.col, coo.data], 1)
    tst_tuple = np.concatenate([tst_ui, tst_r[:, None]], 1).astype(np.float64)
    sampler = ExactSampler(tra, negRatio=.0, batch_size=B, seed=0)
    m = (MF if kind == "mf" else SVD)(C.NU, C.NI, ['rmse', 'mae', 'mse'], (1, 5), C.REG, d, B, max_iter=1, device=0)
    m.set_initial_tables(**{n: T0[n] for n in T0 if not n.startswith("acc_")})
    scores = m.train(1, tra_tuple, tst_tuple, sampler)
    print("%s: rmse gpu %.6f model %.6f" % (kind, scores[0], want))
    assert np.all(np.isfinite(scores)) and scores[0] <= 1.01 * want, (scores, want)
    assert abs(scores[2] - scores[0] ** 2) <= 1e-12 * scores[2]
    assert sampler.state() == (1, 0)
    m.close()
    sampler.close()


def _matrices(f):
    tra = sp.csr_matrix((np.ones(len(f["train_indices"])), f["train_indices"], f["train_indptr"]),
                        shape=(943, 1682))
    tst = sp.csr_matrix((np.ones(len(f["test_indices"])), f["test_indices"], f["test_indptr"]),
                        shape=(943, 1682))
    return tra, tst


def test_wrmf_train_loop(fold1):
    from collaborativefilteringusingtensorflow_amd.ranking import evaluateCV
    from collaborativefilteringusingtensorflow_amd.sampler_rating import ExactSampler
    from collaborativefilteringusingtensorflow_amd.wrmf import WRMF
    tra, tst = _matrices(fold1)
    T0, T = model_epoch("wrmf", 100, 100, tra, 1)
    ip, ix, tp, tx = (fold1[k] for k in ("train_indptr", "train_indices", "test_indptr", "test_indices"))
    users = [u for u in range(943) if tp[u + 1] > tp[u]]
    S = T["user"][users] @ T["item"].T
    pred = []
    for c, u in enumerate(users):
        S[c, ix[ip[u]:ip[u + 1]]] = -np.inf
        pred.append(np.argsort(-S[c], kind="stable")[:10].tolist())
    want = evaluateCV([set(tx[tp[u]:tp[u + 1]].tolist()) for u in users], pred, ['pre'], 10)[0]
    sampler = ExactSampler(tra, negRatio=1, batch_size=100, seed=0)
    m = WRMF(943, 1682, 10, 'cv', ['pre', 'recall', 'map', 'mrr', 'ndcg'], 2., C.REG, 100, 100, max_iter=1, device=0)
    m.set_initial_tables(user=T0["user"], item=T0["item"])
    scores = m.train(1, tra, tst, sampler)
    print("wrmf: pre@10 gpu %.6f model %.6f" % (scores[0], want))
    assert np.all(np.isfinite(scores)) and scores[0] >= 0.5 * want > 0, (scores, want)
    assert sampler.state() == (1, 0)
    m.close()
    sampler.close()


@pytest.mark.parametrize("name", ["testmf", "testsvd", "testwrmf"])
def test_driver_worker_end_to_end(fold1, tmp_path, name):
    """The three drivers: text folds -> loadSparseR (-> matBinarize) -> Sampler
    -> train -> scores (testmf.py:27-46, testsvd.py, testwrmf.py:33-51)."""
    import importlib
    drv = importlib.import_module("collaborativefilteringusingtensorflow_amd.drivers." + name)
    g = C.golden()
    tra = C.raw_train().tocoo()
    with open(tmp_path / "ratings__1_tra.txt", "w") as f:
        for u, i, r in zip(tra.row, tra.col, tra.data):
            f.write("%d\t%d\t%.1f\n" % (u, i, r))
    with open(tmp_path / "ratings__1_tst.txt", "w") as f:
        if name == "testwrmf":     # the whole binarised test fold, as the LRML driver test writes it
            ip, ix = fold1["test_indptr"], fold1["test_indices"]
            for u in range(943):
                for it in ix[ip[u]:ip[u + 1]]:
                    f.write("%d\t%d\t4.0\n" % (u, it))
        else:
            for (u, i), r in zip(g["tst_ui"], g["tst_r"]):
                f.write("%d\t%d\t%.1f\n" % (u, i, r))
    old = drv.max_iter
    drv.max_iter = 2
    try:
        scores = drv.worker(0, 943, 1682, str(tmp_path) + "/")
    finally:
        drv.max_iter = old
    if name == "testwrmf":     # pre, recall, map, mrr, ndcg @ 10
        assert len(scores) == 5 and np.all(np.isfinite(scores)) and scores[0] > 0.02, scores
    else:                      # rmse, mae, mse on ratings 1..5
        assert len(scores) == 3 and np.all(np.isfinite(scores)) and 0.5 < scores[0] < 4.0, scores
