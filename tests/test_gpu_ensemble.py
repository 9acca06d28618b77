"""Ensemble (src/models/pl/models/ensemble.py) on the native ensemble object
(csrc/cf_ensemble.hip) against the float64 oracle (oracle/cf_oracle.py
ens_step / ens_predict, pinned to autograd of the literal TF graph -- with its
[B] x [B, 1] broadcast -- in tests/test_oracle.py).

Tolerance: 1e-4 relative on the loss and on U, V, H and their accumulators
after several steps (fp32 device arithmetic, float atomics in any order,
against float64), batches from the reference's own sampler_uij_ranking
stream (tests/golden/sampler_streams.npz "uij_b100") and synthetic batches
with ragged B, hot rows and repeated items."""
import numpy as np
import pytest

from conftest import ENS_HOT, assert_close, get_stream
from oracle import cf_oracle as O

pytestmark = pytest.mark.gpu
# elementwise: |gpu - oracle| <= 4e-5 + 1e-4 |oracle| (the former max-relative 1e-4 at max|ref| ~ 0.4
# allowed 4e-5 on every element; the [B, B] ensemble loss sums B^2 terms in fp32)
RTOL, ATOL = 1e-4, 4e-5
# (indptr, indices) that no object takes, at n_users = 3, n_items = 4
BAD_CSR = [([0, 1, 2, 2], [0, 1, 2]),   # indptr does not span nnz = 3
           ([0, 2, 1, 3], [0, 1, 2]),   # indptr not monotone
           ([0, 2, 2, 2], [2, 1]),      # an unsorted row
           ([0, 1, 1, 1], [4])]         # item id 4


def make(K, nu, ni, d, reg, seed=5):
    from collaborativefilteringusingtensorflow_amd.ensemble import EnsembleEngine
    rng = np.random.RandomState(seed)
    U = O.init_table(rng, (K, nu, d))
    V = O.init_table(rng, (K, ni, d))
    H = O.init_table(rng, (K, d))
    e = EnsembleEngine(nu, ni, K, d, reg=reg)
    e.set_table("user", U)
    e.set_table("item", V)
    e.set_table("h", H)
    return e, U.astype(np.float64), V.astype(np.float64), H.astype(np.float64)


def check_tables(e, U, V, H, AU, AV, AH, tol=None):
    tol = tol or dict(rtol=RTOL, atol=ATOL)
    for name, o in (("user", U), ("item", V), ("h", H), ("acc_user", AU), ("acc_item", AV),
                    ("acc_h", AH)):
        assert_close(e.get_table(name), o, name, **tol)


@pytest.mark.parametrize("K,d,reg", [(3, 100, 0.01), (2, 20, 0.1), (1, 16, 0.05)])
def test_ensemble_reference_stream_matches_oracle(streams, fold1, K, d, reg):
    st = get_stream(streams, "uij_b100")
    e, U, V, H = make(K, 943, 1682, d, reg)
    AU, AV, AH = (np.full_like(x, 0.1) for x in (U, V, H))
    for s in range(10):
        uij = np.concatenate([st["pairs"][s], st["negs"][s]], 1)
        lg = e.step(uij)
        lo = O.ens_step(U, V, H, AU, AV, AH, uij, reg)
        assert abs(lg - lo) <= RTOL * abs(lo), (s, lg, lo)
    check_tables(e, U, V, H, AU, AV, AH)
    e.close()


@pytest.mark.parametrize("K,B,d", [(8, 257, 33), (3, 64, 100), (4, 1, 8), (2, 130, 256)])
def test_ensemble_ragged_hot_rows(K, B, d):
    rng = np.random.RandomState(K * 100 + B)
    nu, ni = 50, 80                     # small tables: many duplicates per batch
    e, U, V, H = make(K, nu, ni, d, 0.02, seed=B)
    AU, AV, AH = (np.full_like(x, 0.1) for x in (U, V, H))
    for s in range(6):
        uij = np.stack([rng.randint(0, nu, B), rng.randint(0, ni, B), rng.randint(0, ni, B)], 1)
        uij[: B // 3, 0] = 3            # a hot user
        uij[B // 2:, 2] = uij[B // 2:, 1]   # i == j rows
        lg = e.step(uij)
        lo = O.ens_step(U, V, H, AU, AV, AH, uij, 0.02)
        assert abs(lg - lo) <= RTOL * abs(lo), (s, lg, lo)
    # fp32-grounded band: the float32 oracle itself leaves rtol 1e-4 here
    check_tables(e, U, V, H, AU, AV, AH, tol=ENS_HOT)
    e.close()


def test_ensemble_take_loss_and_recommend(fold1):
    e, U, V, H = make(3, 943, 1682, 20, 0.01)
    e.set_interactions(fold1["train_indptr"], fold1["train_indices"])
    rng = np.random.RandomState(1)
    AU, AV, AH = (np.full_like(x, 0.1) for x in (U, V, H))
    tot = 0.0
    for s in range(5):
        uij = np.stack([rng.randint(0, 943, 100), rng.randint(0, 1682, 100),
                        rng.randint(0, 1682, 100)], 1)
        e.step(uij, return_loss=False)
        tot += O.ens_step(U, V, H, AU, AV, AH, uij, 0.01)
    assert abs(e.take_loss() - tot) <= RTOL * tot
    assert e.take_loss() == 0.0
    users = np.arange(0, 943, 5, dtype=np.int32)
    idx, val = e.score_topk(users, 10, return_values=True)
    S = O.ens_predict(U, V, H, users)
    ref = O.recommend(S, fold1["train_indptr"], fold1["train_indices"], users, 10)
    assert sum(1 for a, c in zip(idx.tolist(), ref) if a != c) <= 2
    got = np.take_along_axis(S, idx.astype(np.int64), 1)
    np.testing.assert_allclose(val, got, rtol=1e-4, atol=1e-6)
    e.close()


def test_ensemble_rejects_bad_ids():
    from collaborativefilteringusingtensorflow_amd import _native as N
    e, *_ = make(2, 10, 20, 8, 0.1)
    with pytest.raises(N.NativeError, match="out of range"):
        e.step(np.array([[0, 1, 20]]))
    with pytest.raises(N.NativeError, match="exclude_train"):
        e.score_topk(np.array([0]), 5, exclude_train=True)
    e.close()


def test_ensemble_rejects_bad_csr():
    """A CSR that does not span nnz, is not monotone, holds an unsorted row or
    an item past n_items is CF_EINVAL, and is not installed."""
    from collaborativefilteringusingtensorflow_amd import _native as N
    e, *_ = make(1, 3, 4, 1, 0.1)
    for indptr, indices in BAD_CSR:
        with pytest.raises(N.NativeError, match="CF_EINVAL"):
            e.set_interactions(indptr, indices)
    with pytest.raises(N.NativeError, match="exclude_train"):
        e.score_topk(np.array([0]), 2, exclude_train=True)
    e.close()


def test_ensemble_recommend_chunks_past_grid_y():
    """65,537 users in one call: more than one launch's grid.y (65,535).  The
    lists equal those of two calls that each fit, bit for bit."""
    nu = 65537
    e, *_ = make(1, nu, 8, 4, 0.1)
    users = np.arange(nu, dtype=np.int32)
    idx, val = e.score_topk(users, 2, exclude_train=False, return_values=True)
    ia, va = e.score_topk(users[:40000], 2, exclude_train=False, return_values=True)
    ib, vb = e.score_topk(users[40000:], 2, exclude_train=False, return_values=True)
    assert np.array_equal(idx, np.concatenate([ia, ib]))
    assert np.array_equal(val.view(np.uint32), np.concatenate([va, vb]).view(np.uint32))
    e.close()


def test_ensemble_train_loop(fold1):
    """Ensemble.train on ml-100k fold 1 with the exact reference stream:
    losses fall and the top-10 precision beats random by a wide margin."""
    import scipy.sparse as sp
    from collaborativefilteringusingtensorflow_amd.ensemble import Ensemble
    from collaborativefilteringusingtensorflow_amd.sampler_uij_ranking import ExactSampler
    f = fold1
    tra = sp.csr_matrix((np.ones(len(f["train_indices"])), f["train_indices"], f["train_indptr"]),
                        shape=(943, 1682))
    tst = sp.csr_matrix((np.ones(len(f["test_indices"])), f["test_indices"], f["test_indptr"]),
                        shape=(943, 1682))
    sampler = ExactSampler(tra, batch_size=100, seed=0)
    en = Ensemble(943, 1682, 3, 10, 'cv', ['pre', 'recall', 'map', 'mrr', 'ndcg'], 0.01, 20, 100,
                  max_iter=3, device=0, seed=3, verbose=True)
    scores = en.train(1, tra, tst, sampler)
    assert np.all(np.isfinite(scores))
    assert scores[0] > 0.05, scores
    en.close()


@pytest.mark.parametrize("stream,K,d,lam,singles", [("rank_b100_w5", 5, 100, 1.0, False),
                                                    ("rank_b100_w1", 2, 20, 1.0, False),
                                                    ("rank_b100_w5", 3, 100, 0.1, True),
                                                    ("rank_b50_w5", 8, 33, 0.5, True)])
def test_ensemble_w_variants_match_oracle(streams, stream, K, d, lam, singles):
    """ensemble_.py (singles off, lam 1) and ensemble__.py (members' BPR +
    lam * ensemble) on the reference's captured sampler_ranking streams."""
    st = get_stream(streams, stream)
    e, U, V, H = make(K, 943, 1682, d, 0.1)
    AU, AV, AH = (np.full_like(x, 0.1) for x in (U, V, H))
    tot = 0.0
    for s in range(8):
        lg = e.step_w(st["pairs"][s], st["negs"][s], lam=lam, singles=singles)
        lo = O.ens_w_step(U, V, H, AU, AV, AH, st["pairs"][s], st["negs"][s], 0.1, lam, singles)
        assert abs(lg - lo) <= RTOL * abs(lo), (s, lg, lo)
        tot += lg
    check_tables(e, U, V, H, AU, AV, AH)
    assert abs(e.take_loss() - tot) <= 1e-6 * tot
    e.close()


@pytest.mark.parametrize("variant", ["ensemble_", "ensemble__"])
def test_ensemble_w_drop_in_trains(fold1, variant):
    import importlib
    import scipy.sparse as sp
    from collaborativefilteringusingtensorflow_amd.sampler_ranking import ExactSampler
    mod = importlib.import_module("collaborativefilteringusingtensorflow_amd." + variant)
    f = fold1
    tra = sp.csr_matrix((np.ones(len(f["train_indices"])), f["train_indices"], f["train_indptr"]),
                        shape=(943, 1682))
    tst = sp.csr_matrix((np.ones(len(f["test_indices"])), f["test_indices"], f["test_indptr"]),
                        shape=(943, 1682))
    m = ['pre', 'recall', 'map', 'mrr', 'ndcg']
    if variant == "ensemble_":
        en = mod.Ensemble(943, 1682, 3, 10, 'cv', m, 0.1, 32, 100, max_iter=3, device=0, seed=2)
    else:
        en = mod.Ensemble(943, 1682, 3, 0.1, 10, 'cv', m, 0.1, 32, 100, max_iter=3, device=0, seed=2)
    scores = en.train(1, tra, tst, ExactSampler(tra, n_neg=5, batch_size=100, seed=4))
    assert np.all(np.isfinite(scores)) and scores[0] > 0.05, scores
    en.close()
