"""The sampler_rating drop-in: ``ExactSampler`` (cf_rating_sampler, the native
MT19937 restatement) against the reference's own captured streams
(tests/golden/rating_stream.npz) bit for bit, and against a single-threaded
numpy transcription of sampler_rating.py:22-39 over three epochs."""
import numpy as np
import pytest
import scipy.sparse as sp

import pointwise_cases as C
from collaborativefilteringusingtensorflow_amd.sampler_rating import ExactSampler, Sampler


def binarised(fold1):
    return sp.csr_matrix((np.ones(len(fold1["train_indices"])), fold1["train_indices"], fold1["train_indptr"]),
                         shape=(C.NU, C.NI))


def test_exact_sampler_reproduces_the_mf_stream():
    g = C.golden()
    s = ExactSampler(C.raw_train(), negRatio=.0, batch_size=int(g["batch_size"]), seed=int(g["seed"]))
    for k in range(g["mf_ui"].shape[0]):
        b = s.next_batch()
        assert b.dtype == np.float64 and b.shape == (100, 3)
        assert np.array_equal(b[:, :2], g["mf_ui"][k]) and np.array_equal(b[:, 2], g["mf_r"][k]), k
    assert set(np.unique(g["mf_r"]).tolist()) <= {1, 2, 3, 4, 5}
    assert s.state() == (0, 40)
    s.close()


def test_exact_sampler_reproduces_the_wrmf_stream(fold1):
    g = C.golden()
    s = ExactSampler(binarised(fold1), negRatio=1, batch_size=int(g["batch_size"]), seed=int(g["seed"]))
    ip, ix = fold1["train_indptr"], fold1["train_indices"]
    for k in range(g["wrmf_ui"].shape[0]):
        ui, r = s._draw()           # the native types the engine is fed with
        assert ui.dtype == np.int32 and r.dtype == np.float32 and ui.shape == (200, 2)
        assert np.array_equal(ui, g["wrmf_ui"][k]) and np.array_equal(r, g["wrmf_r"][k]), k
        assert (r == 0).sum() == 100
        for (u, i), rr in zip(ui, r):   # a negative's item is outside Pos(user), a positive's inside
            assert (i in ix[ip[u]:ip[u + 1]]) == (rr == 1)
    s.close()


def transcription(R, negRatio, B, seed, n_batches):
    """sampler_rating.py:22-39 on one thread: the same calls on a seeded legacy
    RandomState, the tuple array shuffled through views as there."""
    rng = np.random.RandomState(seed)
    lil = sp.lil_matrix(R)
    tuples = np.array([(u, i, lil[u, i]) for u, i in np.asarray(lil.nonzero()).T])
    pos = {u: set(row) for u, row in enumerate(lil.rows)}
    n_users, n_items = lil.shape
    out = []
    while True:
        for k in range(int(len(tuples) / B)):
            batch = tuples[k * B:(k + 1) * B, :]
            num_neg = int(B * negRatio)
            if num_neg > 0:
                neg = []
                for _ in range(num_neg):
                    user, item = rng.randint(0, n_users), rng.randint(0, n_items)
                    while item in pos[user]:
                        item = rng.randint(0, n_items)
                    neg.append([user, item, 0])
                batch = np.concatenate([batch, np.array(neg)])
            rng.shuffle(batch)
            out.append(batch.copy())
            if len(out) == n_batches:
                return out


def small_matrix(seed=3, nu=40, ni=60, nnz=520):
    rng = np.random.RandomState(seed)
    flat = rng.choice(nu * ni, nnz, replace=False)
    return sp.csr_matrix((rng.randint(1, 6, nnz).astype(np.float64), (flat // ni, flat % ni)), shape=(nu, ni))


@pytest.mark.parametrize("negRatio", [.0, .5])
def test_three_epochs_equal_the_transcription(negRatio):
    R = small_matrix()
    B = 50
    per_epoch = R.nnz // B
    assert R.nnz % B != 0                      # a tail that is never emitted
    want = transcription(R, negRatio, B, 23, 3 * per_epoch)
    s = ExactSampler(R, negRatio=negRatio, batch_size=B, seed=23)
    got = [s.next_batch() for _ in range(3 * per_epoch)]
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape == (B + int(B * negRatio), 3)
        assert np.array_equal(g, w), k
    assert s.state() == (3, 0)
    coo = R.tocoo()
    tail = set(zip(coo.row[np.lexsort((coo.col, coo.row))][per_epoch * B:].tolist(),
                   coo.col[np.lexsort((coo.col, coo.row))][per_epoch * B:].tolist()))
    dense = R.toarray()
    for k in range(per_epoch):
        rows = [[tuple(x) for x in got[e * per_epoch + k][got[e * per_epoch + k][:, 2] > 0].tolist()]
                for e in range(3)]
        assert set(rows[0]) == set(rows[1]) == set(rows[2])      # the same sets every epoch
        assert not ({(int(u), int(i)) for u, i, _ in rows[0]} & tail)
        for e in range(3):
            b = got[e * per_epoch + k]
            negs = b[b[:, 2] == 0]
            assert len(negs) == int(B * negRatio)
            for u, i, _ in negs:
                assert dense[int(u), int(i)] == 0
    if negRatio == 0:
        # the in-place order carries over: epoch 2's batch is a permutation of epoch 1's *order*,
        # not of the sorted slice -- pinned by equality with the transcription above; and the
        # orders do differ from epoch to epoch
        assert any(not np.array_equal(got[k], got[per_epoch + k]) for k in range(per_epoch))
    s.close()


def test_sampler_seeds_itself_and_checks_arguments():
    R = small_matrix()
    a, b = Sampler(R, batch_size=50), Sampler(R, batch_size=50)
    assert not np.array_equal(a.next_batch(), b.next_batch())      # OS-seeded, as the reference never seeds
    a.close()
    b.close()
    from collaborativefilteringusingtensorflow_amd import _native as N
    with pytest.raises(N.NativeError):
        ExactSampler(R, batch_size=R.nnz + 1)
    with pytest.raises(ValueError):
        ExactSampler(R, batch_size=10, seed=2 ** 32)
