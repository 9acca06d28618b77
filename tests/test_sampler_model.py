"""CPU checks of tests/sampler_model.py, the exact host model the GPU sampler
answers to (tests/test_gpu_sampler_exact.py): the model has to be a sampler
before the device can be held to it."""
import numpy as np
import pytest

import sampler_model as SM

SEEDS = (0, 20261015, (1 << 64) - 1)
EPOCHS = (0, 1000003)
WIDTH_NS = sorted(set(range(1, 301)) | {(1 << k) + d for k in range(8, 17) for d in (-1, 0, 1)})


def toy_graph(seed=3, n_users=37, n_items=53):
    rng = np.random.RandomState(seed)
    rows = [np.sort(rng.choice(n_items, size=rng.randint(0, 30), replace=False)) for _ in range(n_users)]
    rows[0] = []            # first and last users without a row
    rows[-1] = []
    rows[5] = [0, n_items - 1]
    return SM.csr_from_rows(rows) + (n_items,)


def test_mix64_known_values():
    """SplitMix64's published first outputs for seed 0 (mix64(z) adds the
    golden-ratio increment itself, so the stream is mix64(0), mix64(gamma), ..)."""
    g = 0x9E3779B97F4A7C15
    assert SM.mix64(0) == 0xE220A8397B1DCDAF
    assert SM.mix64(g) == 0x6E789E6AA1B965F4
    assert SM.mix64(2 * g & SM.M64) == 0x06C45D188009454F
    z = np.array([0, g, 2 * g & SM.M64], dtype=np.uint64)
    assert [int(v) for v in SM.mix64_np(z)] == [SM.mix64(int(v)) for v in z]


def test_perm_key_fields():
    for n, bits, shift in [(1, 1, 1), (2, 1, 1), (3, 2, 1), (4, 2, 1), (5, 3, 1), (16, 4, 2), (17, 5, 2),
                           (65536, 16, 8), (65537, 17, 8), (1 << 21, 21, 10), ((1 << 21) + 1, 22, 11)]:
        p = SM.make_perm_key(n, 7, 1)
        assert (p.bits, p.mask, p.shift) == (bits, (1 << bits) - 1, shift), n
        assert all(m & 1 for m in p.m) and all(k <= p.mask for k in p.k)
        assert len({*p.m}) == 3


@pytest.mark.parametrize("seed", SEEDS)
def test_permute_is_a_bijection(seed):
    """[0, n) onto [0, n) for every n in 1..300 and around every power of two
    up to 2^16, two epochs; the scalar and the array form agree."""
    for epoch in EPOCHS:
        for n in WIDTH_NS:
            p = SM.make_perm_key(n, seed, epoch)
            img = SM.permute_np(np.arange(n, dtype=np.uint64), p)
            assert np.array_equal(np.sort(img), np.arange(n, dtype=np.uint64)), (n, epoch)
            if n <= 300:
                assert [SM.permute(s, p) for s in range(n)] == img.tolist(), (n, epoch)
    # the epochs and the seeds give different orders
    a = SM.permute_np(np.arange(300, dtype=np.uint64), SM.make_perm_key(300, seed, 0))
    b = SM.permute_np(np.arange(300, dtype=np.uint64), SM.make_perm_key(300, seed, 1))
    c = SM.permute_np(np.arange(300, dtype=np.uint64), SM.make_perm_key(300, seed ^ 1, 0))
    assert not np.array_equal(a, b) and not np.array_equal(a, c)


def test_mulhi_matches_python_integers():
    rng = np.random.RandomState(1)
    h = rng.randint(0, 1 << 32, size=500).astype(np.uint64) << np.uint64(32) | rng.randint(0, 1 << 32, size=500).astype(np.uint64)
    h[:3] = [0, SM.M64, 1 << 63]
    for n in (1, 2, 3, 1003, 100000, (1 << 32) - 1):
        assert SM.mulhi_np(h, n).tolist() == [(int(v) * n) >> 64 for v in h], n
    n = rng.randint(1, 1 << 31, size=500)
    assert SM.mulhi_np(h, n).tolist() == [(int(v) * int(m)) >> 64 for v, m in zip(h, n)]


@pytest.mark.parametrize("G", [0, 3])
@pytest.mark.parametrize("srt", [False, True], ids=["plain", "sorted"])
def test_array_form_equals_scalar_definition(srt, G):
    """Model.sample (numpy) against Model.sample_scalar (Python integers, a
    set per user) over two epochs and a change of B."""
    ip, ix, ni = toy_graph()
    a = SM.Model(ip, ix, ni, 5, G, 11, sorted=srt)
    b = SM.Model(ip, ix, ni, 5, G, 11, sorted=srt)
    for B in [64] * (2 * (len(ix) // 64) + 1) + [7, 7, 64]:
        x, y = a.sample(B), b.sample_scalar(B)
        for xa, ya in zip(x, y):
            assert (xa is None and ya is None) or np.array_equal(xa, ya)
        assert a.state() == b.state()


@pytest.mark.parametrize("B", [1, 10, 64, 97])
def test_sorted_and_unsorted_batches_are_the_same_sets(B):
    ip, ix, ni = toy_graph()
    a = SM.Model(ip, ix, ni, 1, 0, 5, sorted=False)
    b = SM.Model(ip, ix, ni, 1, 0, 5, sorted=True)
    per_epoch = len(ix) // B
    seen = []
    for n in range(per_epoch + 2):
        pa, pb = a.sample(B)[0], b.sample(B)[0]
        ka, kb = pa[:, 0].astype(np.int64) * ni + pa[:, 1], pb[:, 0].astype(np.int64) * ni + pb[:, 1]
        assert np.array_equal(np.sort(ka), kb), n            # the same set, in CSR order
        assert (np.diff(kb) > 0).all() or B == 1
        if n < per_epoch:
            seen.append(ka)
    seen = np.concatenate(seen)
    assert len(np.unique(seen)) == per_epoch * B             # an epoch draws distinct pairs
    assert a.state() == b.state() == (1, 2)


def test_negatives_outside_pos_and_groups_inside_column():
    ip, ix, ni = toy_graph()
    pos = [set(ix[ip[u]:ip[u + 1]].tolist()) for u in range(len(ip) - 1)]
    m = SM.Model(ip, ix, ni, 7, 4, 9)
    for _ in range(12):
        pairs, negs, groups = m.sample(50)
        assert negs.min() >= 0 and negs.max() < ni
        for (u, i), js, gs in zip(pairs, negs, groups):
            assert i in pos[u]
            assert not any(int(j) in pos[u] for j in js)
            assert all(i in pos[int(g)] for g in gs)


def test_state_machine():
    ip, ix, ni = toy_graph()
    nnz = len(ix)
    B = 50
    per = nnz // B
    m = SM.Model(ip, ix, ni, 1, 0, 2)
    assert m.state() == (0, 0)
    for b in range(per):
        m.sample(B)
        assert m.state() == (0, b + 1)
    first = m.sample(B)[0]                 # rollover: lazily, at the next draw
    assert m.state() == (1, 1)
    assert np.array_equal(first, m.draw(1, 0, B)[0])
    m.sample(20)                           # a new B inside an epoch: the next epoch's batch 0
    assert m.state() == (2, 1)
    m.sample(B)                            # and the change back
    assert m.state() == (3, 1)
    m.set_state(3, 0)
    m.sample(20)                           # a new B at batch 0 stays in the epoch
    assert m.state() == (3, 1)
    f = SM.Model(ip, ix, ni, 1, 0, 2)      # set_state on a fresh model keeps the position
    f.set_state(7, 3)
    got = f.sample(B)[0]
    assert f.state() == (7, 4) and np.array_equal(got, f.draw(7, 3 * B, B)[0])
    f.set_state(7, per)                    # past the last whole batch: rolls over
    f.sample(B)
    assert f.state() == (8, 1)
    w = SM.Model(ip, ix, ni, 1, 0, 2)      # B == nnz: one batch per epoch, the whole pair set
    for ep in range(3):
        p = w.sample(nnz)[0]
        assert w.state() == (ep, 1)
        assert len(np.unique(p[:, 0].astype(np.int64) * ni + p[:, 1])) == nnz
    with pytest.raises(ValueError):
        w.sample(nnz + 1)
    with pytest.raises(ValueError):
        w.set_state(-1, 0)
