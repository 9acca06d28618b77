"""Engine-owned memory has one owner (cf_debug_live_bytes), and a batch drawn
ahead has one record: destroying an engine returns every device and pinned
byte it allocated, option changes that re-size buffers keep the accounting,
and dropping a drawn-ahead batch clears its speculative phantom counts too.

ML-100K fold 1 (943 x 1,682), d = 16.
"""
import numpy as np
import pytest
import torch.multiprocessing as mp

from collaborativefilteringusingtensorflow_amd.engine import Engine, live_bytes
from test_gpu_distributed import _draw_ahead_worker, _free_port

pytestmark = pytest.mark.gpu
NU, NI, D, B = 943, 1682, 16, 256

# the smallest engines that between them reach every allocation site
ENGINES = {
    # srec / slotP / slotN / spec buffers / epoch orders
    "bpr-psort": ("bpr", dict(n_neg=1, reg=0.05), {"pos_sort": 1, "sorted_batches": 1, "spec_neg": 1}),
    # + the fixed-point buffers
    "bpr-psort-det": ("bpr", dict(n_neg=1, reg=0.05),
                      {"pos_sort": 1, "sorted_batches": 1, "spec_neg": 1, "deterministic": 1}),
    # item records, the user-row stash, the sort-based deterministic buffers
    "cml-records-det": ("cml", dict(n_neg=5, margin=1.0, reg_cov=1.0, clip_norm=1.0),
                        {"item_slots": 1, "deterministic": 1}),
    # bias tables, pinned staging of host-fed batches
    "gbpr-host-fed": ("gbpr", dict(n_neg=1, gsize=3, rho=0.4, reg=0.01), {}),
}


@pytest.mark.parametrize("name", sorted(ENGINES))
def test_destroy_returns_every_byte(fold1, name):
    model, kw, opts = ENGINES[name]
    before = live_bytes()
    e = Engine(model, NU, NI, D, seed=7, **kw)
    for k, v in opts.items():
        e.set_option(k, v)
    e.set_interactions(fold1["train_indptr"], fold1["train_indices"])
    e.init_params(0.0, 0.1, seed=3)
    if name == "gbpr-host-fed":
        for _ in range(3):
            pairs, negs, groups = e.sample(B)
            e.step(pairs, negs, groups)
    else:
        e.train_steps(B, 3)
    e.score_topk(np.arange(8, dtype=np.int32), 5)
    alive = live_bytes()
    print(name, "before", before, "alive", alive)
    assert alive[0] > before[0] and alive[1] > before[1]
    e.close()
    assert live_bytes() == before


def _ensemble():
    from collaborativefilteringusingtensorflow_amd.ensemble import EnsembleEngine
    return EnsembleEngine(NU, NI, 2, D)


def _lrml():
    from collaborativefilteringusingtensorflow_amd.lrml import LRMLEngine
    return LRMLEngine(NU, NI, D, 4)


def _pointwise(kind):
    from collaborativefilteringusingtensorflow_amd._pointwise import PointwiseEngine
    return PointwiseEngine(NU, NI, D, kind=kind)


def _ids(rng, n, *highs):
    return np.stack([rng.randint(0, h, n) for h in highs], 1).astype(np.int32)


# name -> (constructor, a step of b random in-range rows)
OBJECTS = {
    "ensemble-step": (_ensemble, lambda e, rng, b: e.step(_ids(rng, b, NU, NI, NI))),
    "ensemble-step_w": (_ensemble, lambda e, rng, b: e.step_w(_ids(rng, b, NU, NI), _ids(rng, b, NI, NI))),
    "lrml": (_lrml, lambda e, rng, b: e.step(_ids(rng, b, NU, NI), _ids(rng, b, NU, NI))),
    "pointwise-mf": (lambda: _pointwise("mf"),
                     lambda e, rng, b: e.step(_ids(rng, b, NU, NI), rng.randint(1, 6, b).astype(np.float32))),
    "pointwise-svd": (lambda: _pointwise("svd"),
                      lambda e, rng, b: e.step(_ids(rng, b, NU, NI), rng.randint(1, 6, b).astype(np.float32))),
}


@pytest.mark.parametrize("name", sorted(OBJECTS))
def test_objects_count_and_return_every_byte(fold1, name):
    """The ensemble, LRML and pointwise objects hold their memory in the
    engine's buffer owner: a larger batch grows the count, a smaller one after
    it does not shrink it, per-call scratch (recommend, eval) is gone when the
    call returns, and close() returns everything."""
    create, step = OBJECTS[name]
    rng = np.random.RandomState(11)
    before = live_bytes()
    e = create()
    e.set_interactions(fold1["train_indptr"], fold1["train_indices"])
    e.init_params(seed=3)
    created = live_bytes()[0]
    dev = []
    for b in (64, 257, 64):   # 257: past a 16-row tile, a block and one loss partial
        assert np.isfinite(step(e, rng, b))
        dev.append(live_bytes()[0])
    if name == "pointwise-svd":   # svd.py has no recommend
        ui, r = _ids(rng, 100, NU, NI), rng.randint(1, 6, 100).astype(np.float32)
        assert e.eval(ui, r, 1, 5, return_pred=True)[0].shape == (100,)
        assert e.eval(ui, r, 1, 5, return_pred=False)[0] is None
    else:
        assert e.score_topk(np.arange(8, dtype=np.int32), 5, exclude_train=True).shape == (8, 5)
    print(name, "before", before, "created", created, "steps", dev, "end", live_bytes())
    assert created > before[0]
    assert dev[1] > dev[0]
    assert dev[2] == dev[1]
    assert live_bytes()[0] == dev[2]
    e.close()
    assert live_bytes() == before


@pytest.mark.parametrize("name", ["ensemble-step", "lrml", "pointwise-mf"])
def test_rejected_calls_leave_the_count(fold1, name):
    import ctypes
    from collaborativefilteringusingtensorflow_amd import _native as N
    create, step = OBJECTS[name]
    rng = np.random.RandomState(12)
    e = create()
    e.set_interactions(fold1["train_indptr"], fold1["train_indices"])
    e.init_params(seed=3)
    step(e, rng, 64)
    held = live_bytes()

    def bad_step():
        ids = _ids(rng, 64, NU, NI, NI)
        ids[63, 1] = NI   # one item past the table
        if name == "ensemble-step":
            e.step(ids)
        elif name == "lrml":
            e.step(ids[:, :2], _ids(rng, 64, NU, NI))
        else:
            e.step(ids[:, :2], np.ones(64, np.float32))

    def bad_table():   # past the wrapper's own shape check
        a = np.zeros(3, np.float32)
        N.check(e._fn("set_table")(e._h, 0, a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), a.size), "set_table")

    def bad_csr():
        indptr = np.zeros(NU + 1, np.int64)
        indptr[1:] = 2
        e.set_interactions(indptr, np.array([2, 1], np.int32))

    for call in (bad_step, bad_table, bad_csr):
        with pytest.raises(N.NativeError, match="CF_EINVAL"):
            call()
        assert live_bytes() == held, call.__name__
    assert np.isfinite(step(e, rng, 64))
    assert e.score_topk(np.arange(8, dtype=np.int32), 5, exclude_train=True).shape == (8, 5)   # the CSR stayed
    e.close()


def test_option_reallocation_keeps_accounting(fold1):
    before = live_bytes()
    e = Engine("bpr", NU, NI, D, n_neg=1, reg=0.05, seed=7)
    e.set_option("pos_sort", 1)
    e.set_option("slot_max_user", 2)
    e.set_interactions(fold1["train_indptr"], fold1["train_indices"])
    e.init_params(0.0, 0.1, seed=3)

    def toggle(option, *values):
        for v in values:
            e.set_option(option, v)
            e.train_steps(B, 1)
        dev = live_bytes()[0]
        print(option, values, dev)
        return dev

    e.train_steps(B, 1)
    m0 = live_bytes()[0]
    # item records stash each pair's user row (stashU, [B, d] floats), and the
    # stash stays for the next switch to records: the one buffer that is larger
    # after the round trip
    m1 = toggle("item_slots", 1, 0)
    assert m1 == m0 + B * D * 4
    assert toggle("pos_sort", 0, 1) == m1
    assert toggle("slot_max_user", 4) > m1      # the user slot rows double
    assert toggle("slot_max_user", 2) == m1
    m2 = toggle("deterministic", 1)
    assert m2 > m1
    # the fixed-point buffers (slotP64, GU64, GV64, hotU, hot_n, fx_bad) are
    # kept for the next deterministic step
    assert toggle("deterministic", 0) >= m1
    e.close()
    assert live_bytes() == before


def test_drop_of_drawn_ahead_batch_with_spec_counts(fold1):
    """BPR, dense_item_apply, pos_sort 1, spec_neg 1, W = 1 through
    cf_step_local_grad / cf_step_local_apply(next_B) at world size 1: the
    batch drawn ahead was counted with speculative phantoms (n_items 1,682 <=
    2 B (1 + W) = 2,048 at B = 512), and dropping it (cf_sample) must uncount
    them, rewind the sampler and leave the steps after it as if it had never
    been drawn."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_draw_ahead_worker, args=(_free_port(), fold1, q, "allreduce", 1,
                                                     {"pos_sort": 1, "spec_neg": 1}, 512))
    p.start()
    a, b = q.get(timeout=300)
    p.join(timeout=120)
    assert p.exitcode == 0
    for x, y in zip(a[:3], b[:3]):   # float-atomic item sums: last-bit order effects only
        assert np.abs(x - y).max() <= 1e-6 * np.abs(y).max()
    assert a[3] == b[3]                                                # sampler_state()
    assert np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5])   # the next sample
