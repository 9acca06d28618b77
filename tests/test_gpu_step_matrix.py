"""Every step-kernel instantiation on the device, at its width and count
edges (tests/step_matrix.py: the case table, the host model of the dispatch
and the edge batches; tests/test_step_matrix.py shows on the CPU that the
table reaches every instantiation and that the float32 oracle alone stays
inside half of every band asserted here).

Each case builds one engine, checks that cf_step_path reports the path the
host model predicts, and takes three host-fed steps on the three edge batches
against the float64 oracle: BPR / AMF / CML under conftest.LocalStepCheck
(every element within the a-priori fp32 bound, untouched rows bit-identical,
the loss within 1e-5; BPR / AMF also the three-step trajectory in the default
band), GBPR / tuples / apr step by step from the engine's own tables in the
default band.  Deterministic cases run the steps twice from the same state
and must agree bit for bit.  No tolerance here is new."""
import numpy as np
import pytest

import step_matrix as M
from conftest import LocalStepCheck, assert_close
from oracle import cf_oracle as O

pytestmark = pytest.mark.gpu

RTOL = 1e-5
TABLES4 = ("user", "item", "acc_user", "acc_item")
TABLES6 = ("user", "item", "bias", "acc_user", "acc_item", "acc_bias")


def _engine(c, fold1, nu, ni):
    from collaborativefilteringusingtensorflow_amd.engine import Engine
    kw = dict(M.HP[c.model])
    if c.amf_mode == "apr":
        kw.update(epsilon=M.APR_EPS, amf_mode="apr")
    e = Engine(c.model, nu, ni, c.d, n_neg=c.W, gsize=max(c.G, 1), seed=7, **kw)
    if c.item_slots is not None:
        e.set_option("item_slots", c.item_slots)
    if c.slot_max is not None:
        e.set_option("slot_max", c.slot_max)
        e.set_option("slot_max_user", c.slot_max)
    for k, v in c.opts.items():
        e.set_option(k, v)
    if c.table == "small":
        e.set_interactions(fold1["train_indptr"], fold1["train_indices"])
    else:
        e.set_interactions(*M.tiny_csr(nu, ni))
    return e


def _init_tables(c, nu, ni):
    rng = np.random.RandomState(3)
    std = M.INIT_STD.get(c.model, 0.1)
    T = {"user": O.init_table(rng, (nu, c.d), stddev=std, truncated=(c.model != "cml")),
         "item": O.init_table(rng, (ni, c.d), stddev=std, truncated=(c.model != "cml"))}
    if c.model in ("gbpr",) + tuple(M.TUPLE_MODELS):
        T["bias"] = O.init_table(rng, (ni,))
        T["acc_bias"] = np.full((ni,), 0.1, np.float32)
    T["acc_user"] = np.full((nu, c.d), 0.1, np.float32)
    T["acc_item"] = np.full((ni, c.d), 0.1, np.float32)
    return T


def _oracle_step(c, T, b):
    """One float64 oracle step on the tables T (dict, in place); the loss."""
    hp = M.HP[c.model]
    four = (T["user"], T["item"], T["acc_user"], T["acc_item"])
    if c.model == "bpr":
        return O.bpr_step(*four, b["pairs"], b["negs"], hp["reg"])
    if c.model == "amf" and c.amf_mode == "apr":
        return O.amf_apr_step(*four, b["pairs"], b["negs"], hp["reg"], M.APR_EPS, reg_adv=hp["reg_adv"])
    if c.model == "amf":
        return O.amf_step(*four, b["pairs"], b["negs"], hp["reg"], bool(c.phase), reg_adv=hp["reg_adv"])
    six = (T["user"], T["item"], T["bias"], T["acc_user"], T["acc_item"], T["acc_bias"])
    if c.model == "gbpr":
        return O.gbpr_step(*six, b["pairs"], b["negs"], b["groups"], hp["rho"], hp["reg"])
    return O.plr_step(*six, b["tuples"], b["coefs"], 0 if c.model == "prigp" else 1, hp["reg"],
                      hp.get("alpha", 1.0), hp.get("beta", 1.0), hp.get("gamma", 1.0))


def _step(c, e, b):
    if c.model in M.TUPLE_MODELS:
        return e.step_plr(b["tuples"], b["coefs"])
    return e.step(b["pairs"], b["negs"], b["groups"])


def _untouched(b, nu, ni):
    cu, cp, cn = M.occurrence_counts(b, nu, ni)
    return np.flatnonzero(cu == 0), np.flatnonzero(cp + cn == 0)


def _local_steps(c, e, batches, names, nu, ni):
    """Each step from the engine's own pre-step tables against one float64
    oracle step, elementwise in the default band on every table."""
    losses = []
    for s, b in enumerate(batches):
        pre = {t: e.get_table(t) for t in names}
        T = {t: pre[t].astype(np.float64) for t in names}
        lg = _step(c, e, b)
        lo = _oracle_step(c, T, b)
        assert abs(lg - lo) <= RTOL * abs(lo), (s, lg, lo)
        ou, oi = _untouched(b, nu, ni)
        for t in names:
            got = e.get_table(t)
            assert_close(got, T[t], "step %d %s" % (s, t))
            rows = ou if t in ("user", "acc_user") else oi
            assert np.array_equal(got[rows], pre[t][rows]), "step %d %s: an untouched row moved" % (s, t)
        losses.append(lg)
    return losses


def _bounded_steps(c, e, batches, T0):
    """BPR / AMF / CML: every step under LocalStepCheck; BPR / AMF also the
    trajectory against the float64 oracle in the default band."""
    hp = M.HP[c.model]
    if c.model == "cml":
        chk = LocalStepCheck(model="cml", **hp)
    else:
        chk = LocalStepCheck(hp["reg"], adversarial=None if c.model == "bpr" else bool(c.phase),
                             reg_adv=hp.get("reg_adv", 1.0))
    T = {t: T0[t].astype(np.float64) for t in TABLES4}
    losses = []
    for s, b in enumerate(batches):
        chk.before(e)
        lg = e.step(b["pairs"], b["negs"])
        chk.after(e, b["pairs"], b["negs"], lg, "step %d" % s)
        if c.model != "cml":
            lo = _oracle_step(c, T, b)
            assert abs(lg - lo) <= RTOL * abs(lo), (s, lg, lo)
        losses.append(lg)
    if c.model != "cml":
        for t in TABLES4:
            assert_close(e.get_table(t), T[t], "after three steps: " + t)
    return losses


@pytest.mark.parametrize("c", M.CASES, ids=M.case_id)
def test_step_matrix(fold1, c):
    from collaborativefilteringusingtensorflow_amd._native import NativeError
    nu, ni = M.table_shape(c)
    batches = M.edge_batches(c.model, c.W, c.G, nu, ni)
    plan = M.case_plan(c)
    if plan.refused:
        # amf_mode apr takes neither option: setting it is what the engine refuses,
        # and the engine goes on stepping as it was
        e = _engine(c._replace(opts={}, item_slots=None), fold1, nu, ni)
        e.begin_phase(c.phase)
        if c.item_slots == 1:
            with pytest.raises(NativeError, match="item_slots 1 .* cannot carry apr"):
                e.set_option("item_slots", 1)
        for k, v in c.opts.items():
            with pytest.raises(NativeError, match="deterministic mode does not cover amf_mode apr"):
                e.set_option(k, v)
        assert not e.step_path(batches[0]["B"])[1]["deterministic"]
        assert np.isfinite(e.step(batches[0]["pairs"], batches[0]["negs"]))
        e.close()
        return
    e = _engine(c, fold1, nu, ni)
    T0 = _init_tables(c, nu, ni)
    names = TABLES6 if "bias" in T0 else TABLES4
    e.set_params(**T0)
    if c.model == "amf" and c.phase:
        e.begin_phase(1)
    for b in batches:
        want = M.case_plan(c, b["B"]).flags
        got = e.step_path(b["B"])[1]
        assert {k: got[k] for k in want} == want, (b["B"], got, want)
    e.profile_reset()
    e.profile(True)
    if c.model in ("bpr", "cml") or (c.model == "amf" and c.amf_mode != "apr"):
        losses = _bounded_steps(c, e, batches, T0)
    else:
        losses = _local_steps(c, e, batches, names, nu, ni)
    e.profile(False)
    assert e.profile_read("psort")[1] == (len(batches) if plan.kind == "sorted" else 0)
    if plan.flags["deterministic"]:
        # the same three steps from the same state: bit for bit
        first = {t: e.get_table(t) for t in names}
        e.set_params(**T0)
        again = [_step(c, e, b) for b in batches]
        assert again == losses
        for t in names:
            assert np.array_equal(e.get_table(t), first[t]), t
    e.close()


# ---------------------------------------------------------------------------
# tile and key-width edges
# ---------------------------------------------------------------------------
def _bpr16(nu, ni, W, opts):
    from collaborativefilteringusingtensorflow_amd.engine import Engine
    e = Engine("bpr", nu, ni, 16, n_neg=W, seed=7, **M.HP["bpr"])
    e.set_option("item_slots", 0)
    for k, v in opts.items():
        e.set_option(k, v)
    e.set_interactions(*M.tiny_csr(nu, ni))
    rng = np.random.RandomState(5)
    e.set_table("user", O.init_table(rng, (nu, 16)))
    e.set_table("item", O.init_table(rng, (ni, 16)))
    return e


def _two_bounded_steps(e, batches):
    chk = LocalStepCheck(M.HP["bpr"]["reg"])
    e.profile_reset()
    e.profile(True)
    for s, (pairs, negs) in enumerate(batches):
        chk.before(e)
        lg = e.step(pairs, negs)
        chk.after(e, pairs, negs, lg, "step %d" % s)
    e.profile(False)
    return e.profile_read("psort")[1]


@pytest.mark.parametrize("W", [1, 5])
@pytest.mark.parametrize("n_items", [2047, 2048, 2049, 4095, 4096])
def test_psort_scan_tile_edges(n_items, W):
    """n_items + 1 scan entries exactly fill, or just spill into, a 2,048-entry
    tile; the ids at the tile's edge and the table's end are duplicated in one
    batch and singletons in the other."""
    e = _bpr16(500, n_items, W, {"pos_sort": 1})
    assert e.step_path(300)[1]["pos_sort"]
    assert _two_bounded_steps(e, M.tile_edge_batches(500, n_items, W)) == 2
    e.close()


@pytest.mark.parametrize("W", [1, 5])
@pytest.mark.parametrize("n_rows", [4095, 4096, 4097])
def test_deterministic_sort_key_width(n_rows, W):
    """n_users + n_items at a power of two: the highest user and item keys of
    the deterministic mode's radix sort (key_bits) are in both batches."""
    n_items = n_rows - 500
    e = _bpr16(500, n_items, W, {"deterministic": 1, "pos_sort": 0})
    f = e.step_path(300)[1]
    assert f["deterministic"] and not f["pos_sort"]
    assert _two_bounded_steps(e, M.tile_edge_batches(500, n_items, W)) == 0
    e.close()


# ---------------------------------------------------------------------------
# the instantiations that carry the next step's draw
# ---------------------------------------------------------------------------
DRAW_HOSTS = [
    # (model, W, G, options, the path cf_step_path reports)
    ("bpr", 1, 0, dict(pipeline=2, grad_path=2), dict(phased=True, pos_sort=False)),
    ("amf", 5, 0, dict(pipeline=2, grad_path=2), dict(phased=True, pos_sort=False)),
    ("cml", 5, 0, dict(pipeline=2, grad_path=2), dict(phased=True, pos_sort=False)),
    ("gbpr", 5, 1, dict(pipeline=2, grad_path=2), dict(phased=True, pos_sort=False)),
    ("bpr", 1, 0, dict(pipeline=3, pos_sort=1, item_slots=0), dict(pos_sort=True)),
    ("amf", 5, 0, dict(pipeline=3, pos_sort=1, item_slots=0), dict(pos_sort=True)),
    ("bpr", 5, 0, dict(pipeline=1, grad_path=1), dict(phased=False, pos_sort=False)),
    ("gbpr", 2, 3, dict(pipeline=1), dict(phased=False, pos_sort=False)),
]


def _sampling_engine(fold1, model, d, W, G, opts):
    from collaborativefilteringusingtensorflow_amd.engine import Engine
    e = Engine(model, 943, 1682, d, n_neg=W, gsize=max(G, 1), seed=31, **M.HP[model])
    for k, v in opts.items():
        e.set_option(k, v)
    e.set_interactions(fold1["train_indptr"], fold1["train_indices"])
    e.init_params(0.0, 0.1, truncated=(model != "cml"), seed=5)
    if model == "amf":
        e.begin_phase(1)
    return e


@pytest.mark.parametrize("d", [7, 100, 128])
@pytest.mark.parametrize("model,W,G,opts,path", DRAW_HOSTS,
                         ids=["%s-w%d-p%d" % (m, W, o["pipeline"]) for m, W, _g, o, _p in DRAW_HOSTS])
def test_draw_hosting_instantiations(fold1, model, W, G, opts, path, d):
    """train_steps (the next step's draw fused into the gradient launch under
    pipeline 2, into the sorted gradient launch under pipeline 3, into the
    apply launch under pipeline 1) trains what the host-fed sample + step
    stream trains, at the widths tests/test_gpu_pipeline.py does not run
    (the assertion of its test_train_steps_equals_host_fed_stream; CML bit
    for bit in deterministic mode instead, see below)."""
    B, K = 250, 5
    host_opts = {k: v for k, v in opts.items() if k != "pipeline"}
    host = _sampling_engine(fold1, model, d, W, G, host_opts)
    dev = _sampling_engine(fold1, model, d, W, G, opts)
    got = dev.step_path(B)[1]
    assert got["pipeline"] == opts["pipeline"] and {k: got[k] for k in path} == path, got
    if model == "cml":
        # two float32 CML runs whose sums add in different orders drift apart
        # through the hinge, the argmin and the rank weight's indicators
        # (DESIGN 4.1), so no band between them is sound: all run in
        # deterministic mode instead, where neither the fused draw nor the way
        # the batch arrives may change a bit -- against the host-fed sample +
        # step stream and against single device-drawn steps (no fused draw)
        single = _sampling_engine(fold1, model, d, W, G, host_opts)
        for e in (host, single, dev):
            e.set_option("deterministic", 1)
        loss_h = 0.0
        for _ in range(K):
            pairs, negs, _g = host.sample(B)
            loss_h += host.step(pairs, negs)
        loss_s = sum(single.train_steps(B, 1) for _ in range(K))
        loss_d = dev.train_steps(B, K)
        assert host.sampler_state() == dev.sampler_state() == single.sampler_state()
        for name, ref, loss in (("single steps", single, loss_s), ("host-fed", host, loss_h)):
            assert abs(loss_d - loss) <= RTOL * abs(loss), (name, loss_d, loss)
            for t in TABLES4:
                assert np.array_equal(dev.get_table(t), ref.get_table(t)), (name, t)
        for e in (host, single, dev):
            e.close()
        return
    loss_h = 0.0
    for _ in range(K):
        pairs, negs, groups = host.sample(B)
        loss_h += host.step(pairs, negs, groups)
    ref = {t: host.get_table(t) for t in (TABLES6 if model == "gbpr" else TABLES4)}
    loss_d = dev.train_steps(B, K)
    assert abs(loss_d - loss_h) <= RTOL * abs(loss_h), (loss_d, loss_h)
    assert host.sampler_state() == dev.sampler_state()
    for t in ref:
        assert_close(dev.get_table(t), ref[t], t)
    host.close()
    dev.close()
