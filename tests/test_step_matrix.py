"""CPU checks of tests/step_matrix.py: the case table reaches every gradient
instantiation the dispatch can pick, the edge batches hold the occurrence
counts and tile alignments they are built for, and the float32 oracle alone
stays well inside the bands tests/test_gpu_step_matrix.py asserts -- so a
device result outside a band is the device's, not the input's."""
import itertools

import numpy as np
import pytest

import step_matrix as M
from conftest import ATOL, RTOL
from oracle import cf_oracle as O
from oracle import fp32_bound as FB


# ---------------------------------------------------------------------------
# dispatch
# ---------------------------------------------------------------------------
def test_plan_of_known_shapes():
    """The host model against shapes whose path the GPU tests pin by flag or
    launch count (tests/test_gpu_lds_grad.py, test_gpu_pos_sort.py)."""
    p = M.plan_of("bpr", 128, 5, 0, dict(item_slots=0, B=512))
    assert (p.kind, p.epl, p.layout, p.flags["lds"], p.flags["phased"]) == ("lds", 8, "vector", True, True)
    p = M.plan_of("gbpr", 64, 5, 1, dict(B=512))
    assert (p.kind, p.epl, p.layout) == ("lds", 4, "scalar")
    p = M.plan_of("gbpr", 64, 5, 1, dict(grad_path=2, B=512))
    assert (p.kind, p.pairs_per_group, p.full) == ("phased", 2, True)
    p = M.plan_of("gbpr", 128, 5, 1, dict(grad_path=2, B=512))
    assert (p.kind, p.pairs_per_group, p.full) == ("phased", 1, False)
    p = M.plan_of("cml", 50, 5, 0, dict(pos_sort=1, B=512))             # auto keeps CML W = 5 generic
    assert p.kind == "generic" and not p.flags["pos_sort"]
    p = M.plan_of("cml", 50, 5, 0, dict(pos_sort=1, grad_path=2, B=512))
    assert p.kind == "sorted" and p.flags["pos_sort"] and p.flags["phased"]
    p = M.plan_of("bpr", 128, 1, 0, dict(pos_sort=1, item_slots=0, deterministic=1, B=512))
    assert (p.kind, p.epl, p.layout, p.full, p.fx) == ("sorted", 8, "vector", False, True)
    p = M.plan_of("bpr", 128, 1, 0, dict(pos_sort=1, item_slots=0, B=512))
    assert (p.full, p.fx) == (True, False)
    p = M.plan_of("bpr", 128, 1, 0, dict(pos_sort=1, B=512))            # records by default at d = 128
    assert p.kind == "phased" and p.flags["item_records"] and not p.flags["pos_sort"]
    p = M.plan_of("bpr", 64, 1, 0, dict(B=1 << 18))                     # auto pos_sort from 2^18
    assert p.kind == "sorted"
    p = M.plan_of("bpr", 200, 5, 0, dict(grad_path=2, B=512))           # no phased kernel past d = 128
    assert (p.kind, p.wt, p.epl) == ("generic", 0, 16)
    p = M.plan_of("amf", 40, 5, 0, dict(amf_mode="apr", phase=1, B=512))
    assert (p.kind, p.wt) == ("apr", 5)
    assert M.plan_of("amf", 40, 5, 0, dict(amf_mode="apr", phase=1, deterministic=1)).refused
    assert M.plan_of("cml", 40, 17, 0).refused and M.plan_of("bpr", 257, 1, 0).refused
    # both applies: small tables are visited row by row, large ones through the owners
    p = M.plan_of("bpr", 64, 1, 0, dict(pos_sort=1, B=587, n_users=943, n_items=1682))
    assert p.dense_items and p.dense_users
    p = M.plan_of("bpr", 64, 1, 0, dict(pos_sort=1, B=587, n_users=1237, n_items=2379))
    assert not p.dense_items and not p.dense_users


def _reachable():
    """Every instantiation plan_of produces over the ABI's ranges: d 1..256;
    W 1..64 (CML 16) through the values the dispatch compares it with and
    their neighbours; G 1..16 likewise; every value of the options that
    select a path.  (pos_sort 2 = auto is pos_sort 1 from 2^18 pairs up and 0
    below; a fused draw changes DRAW, which is no part of the tuple.)"""
    out = set()
    Ws = (1, 2, 3, 4, 5, 6, 16, 17, 64)
    variants = [("bpr", 0, "reference", (0,)), ("amf", 0, "reference", (0,)), ("amf", 1, "reference", (0,)),
                ("amf", 0, "apr", (0,)), ("amf", 1, "apr", (0,)), ("cml", 0, "reference", (0,)),
                ("gbpr", 0, "reference", (1, 2, 16)), ("prigp", 0, "reference", (0,)),
                ("cplr", 0, "reference", (0,))]
    for (model, phase, mode, Gs), gp, ps, det, isl, pipe in itertools.product(
            variants, (0, 1, 2, 3), (0, 1), (0, 1), (0, 1), (1, 2)):
        o = dict(grad_path=gp, pos_sort=ps, deterministic=det, item_slots=isl, pipeline=pipe, phase=phase,
                 amf_mode=mode, B=587)
        for W in ([M.TUPLE_MODELS[model]] if model in M.TUPLE_MODELS else Ws):
            for G in Gs:
                for d in range(1, M.MAX_D + 1):
                    p = M.plan_of(model, d, W, G, o)
                    if not p.refused:
                        out.add(p.inst)
    return out


def test_cases_cover_every_reachable_instantiation():
    reach = _reachable()
    covered = {M.case_plan(c).inst for c in M.CASES if not M.case_plan(c).refused}
    print("matrix cases: %d; instantiations reachable: %d, covered: %d"
          % (len(M.CASES), len(reach), len(covered & reach)))
    assert covered <= reach, sorted(covered - reach)      # the model and the enumeration agree
    missing = sorted(reach - covered)
    assert not missing, "no case in step_matrix.CASES runs %d instantiations: %s" % (len(missing), missing[:12])


def test_cases_are_what_they_say():
    """Each row takes the path it is filed under, on both table sizes, and the
    two table sizes take the two applies."""
    kinds = {"generic": ("generic",), "phased": ("phased",), "sorted": ("sorted",), "detsorted": ("sorted",),
             "lds": ("lds",), "apr": ("apr",), "tuple": ("tuple",),
             "det": ("generic", "phased", "lds")}
    ids = [M.case_id(c) for c in M.CASES]
    assert len(set(ids)) == len(ids)
    for c in M.CASES:
        p = M.case_plan(c)
        if p.refused:
            continue
        assert p.kind in kinds[c.path], (M.case_id(c), p.kind)
        assert p.fx == (c.path == "detsorted"), M.case_id(c)
        assert p.flags["deterministic"] == (c.path in ("det", "detsorted")), M.case_id(c)
        for B in M.BATCH_SIZES:
            q = M.case_plan(c, B)
            assert q.inst == p.inst
            if c.model in ("bpr", "amf", "cml") and c.path != "det" and c.path != "detsorted":
                assert q.dense_items == (c.table == "small"), M.case_id(c)
            if q.flags["pos_sort"]:
                assert q.dense_users == (c.table == "small"), M.case_id(c)
    assert sum(M.case_plan(c).refused for c in M.CASES) == 2


# ---------------------------------------------------------------------------
# edge batches
# ---------------------------------------------------------------------------
SHAPES = [("bpr", 1, 0), ("bpr", 3, 0), ("bpr", 5, 0), ("gbpr", 5, 1), ("gbpr", 2, 3), ("gbpr", 1, 16),
          ("gbpr", 1, 1), ("prigp", 3, 0), ("cplr", 2, 0)]


def _tables_of(model, W, G, table):
    c = M.Case("x", model, 64, W, G, {}, 0, "reference", None, None, table)
    return M.table_shape(c)


@pytest.mark.parametrize("table", ["small", "large"])
@pytest.mark.parametrize("model,W,G", SHAPES)
def test_edge_batches_hold_the_prescribed_counts(model, W, G, table):
    nu, ni = _tables_of(model, W, G, table)
    bs = M.edge_batches(model, W, G, nu, ni)
    assert [b["B"] for b in bs] == list(M.BATCH_SIZES)
    prev = None
    for b in bs:
        cu, cp, cn = M.occurrence_counts(b, nu, ni)
        n = b["named"]
        assert set(cu[cu > 0].tolist()) == set(M.USER_COUNTS)
        only_p, only_n, both = (cp > 0) & (cn == 0), (cn > 0) & (cp == 0), (cp > 0) & (cn > 0)
        assert set(cp[only_p].tolist()) == set(M.POS_COUNTS)
        assert set(cn[only_n].tolist()) == set(M.NEG_COUNTS)
        assert sorted(zip(cp[both].tolist(), cn[both].tolist())) == [(1, 1), (1, 1), (3, 3)]
        assert int((cp[only_p] == 128).sum()) == 2
        # 128 positives at offP = 0 span exactly capP blocks, the other 128 capP + 1
        blocks = M.psort_blocks(b["pairs"][:, 1], ni)
        assert n["L"] == int(np.flatnonzero(cp)[0])
        assert blocks[n["L"]] == M.CAP_P and blocks[n["a2"]] == M.CAP_P + 1
        # the named pairs
        i, j = b["pairs"][:, 1], b["negs"]
        assert ((j == i[:, None]).any(axis=1) & (i == n["yji"])).sum() == 1          # j == i
        px, qx = np.flatnonzero(i == n["x11"]), np.flatnonzero((j == n["x11"]).any(axis=1))
        assert len(px) == 1 and len(qx) == 1 and px[0] != qx[0]
        if W >= 2:
            assert ((j == n["zrep"]).sum(axis=1) == 2).sum() == 1
        if model == "gbpr":
            u, g = b["pairs"][:, 0], b["groups"]
            assert (g == u[:, None]).any()                                         # member == own u
            in_u, in_g = set(u.tolist()), set(g.reshape(-1).tolist())
            assert any(cu[x] == 3 and (u == x).sum() == 1 and (g == x).sum() == 2 for x in in_u & in_g)
            if G >= 2:
                assert any((np.sort(r)[1:] == np.sort(r)[:-1]).any() for r in g)   # twice in one group
        if model in M.TUPLE_MODELS:
            assert b["tuples"].shape == (b["B"], W + 2)
        # the hot rows moved: last batch's hottest rows are singletons here
        if prev is not None:
            tot = cp + cn
            assert all(tot[k] == 1 for k in prev["hot_items"][:40])
            if table == "large" or G < 3:   # (943 users at G >= 3: one singleton, edge_batches' docstring)
                assert len(prev["hot_users"]) >= 6 and all(cu[k] == 1 for k in prev["hot_users"][:32])
            assert not (set(prev["named"].values()) & set(n.values())) - {None}
        prev = b


@pytest.mark.parametrize("table", ["small", "large"])
@pytest.mark.parametrize("model,W,G", [("bpr", 1, 0), ("bpr", 5, 0), ("gbpr", 5, 1), ("gbpr", 2, 3)])
def test_deterministic_batches_hit_the_tile_edges(model, W, G, table):
    nu, ni = _tables_of(model, W, G, table)
    bs = M.edge_batches(model, W, G, nu, ni)
    assert [b["nU"] % M.kDetTile == 0 for b in bs] == [False, True, False]
    for b in bs:
        # the split is the host sort's: users first, then items offset by n_users
        items = [r for r in b["det"] if r[0] >= nu]
        assert {r[1] for r in items} >= {127, 128, 129}
        assert all(r[4] is None for r in items if r[1] == 127)       # below 2 tiles: slot by slot
        tiled = [r for r in items if r[4] is not None]
        gs = lambda r: r[2]                                           # noqa: E731
        ge = lambda r: r[2] + r[1]                                    # noqa: E731
        starts = [r for r in tiled if gs(r) % 64 == 0 and ge(r) % 64 != 0]
        ends = [r for r in tiled if gs(r) % 64 != 0 and ge(r) % 64 == 0]
        both = [r for r in tiled if gs(r) % 64 == 0 and ge(r) % 64 == 0]
        one = [r for r in tiled if r[1] == 128 and r[4] == 1 and r[3] > 0 and r[5] > 0]
        assert starts and ends and both and one, (b["nU"], tiled)
        for r in tiled:
            assert r[3] + 64 * r[4] + r[5] == r[1] and 0 <= r[3] < 64 and 0 <= r[5] < 64


def test_tile_edge_batches():
    for ni in (2047, 2048, 2049, 4095, 4096):
        for W in (1, 5):
            (p0, n0), (p1, n1) = M.tile_edge_batches(500, ni, W)
            edge, near = M.tile_edge_ids(ni)
            assert set(edge) >= {0, 2046, ni - 1} and len(near) >= 2
            for it in edge:
                assert (p0[:, 1] == it).sum() == 3 and (n0 == it).sum() == 2      # duplicated, then
                assert (p1[:, 1] == it).sum() == 1 and (n1 == it).sum() == 1      # exactly once
            for it in near:
                assert (p0[:, 1] == it).sum() == 1 and (n0 == it).sum() == 1
                assert (p1[:, 1] == it).sum() == 3 and (n1 == it).sum() == 2
            assert (p0[:, 0] == 499).any() and (p1[:, 0] == 499).any()
            assert p0.max() < max(500, ni) and n0.max() < ni and n1.max() < ni and p1[:, 1].max() < ni


# ---------------------------------------------------------------------------
# the bands are satisfiable by the reference alone
# ---------------------------------------------------------------------------
def _init(model, nu, ni, d, seed=3):
    rng = np.random.RandomState(seed)
    std = M.INIT_STD.get(model, 0.1)
    U = O.init_table(rng, (nu, d), stddev=std, truncated=(model != "cml"))
    V = O.init_table(rng, (ni, d), stddev=std, truncated=(model != "cml"))
    b = O.init_table(rng, (ni,))
    return U, V, b


def _dedup32(X, A, rows, grads, lr, order, rng):
    """cf_oracle.dedup_adagrad in float32, each row's occurrences added one
    after the other in reverse or in shuffled order (np.add.at adds in the
    order given, unbuffered)."""
    rows = np.asarray(rows).reshape(-1)
    g = np.asarray(grads, np.float32).reshape((rows.shape[0],) + X.shape[1:])
    perm = np.arange(rows.shape[0])[::-1] if order == "reverse" else rng.permutation(rows.shape[0])
    uniq, inv = np.unique(rows, return_inverse=True)
    G = np.zeros((uniq.shape[0],) + X.shape[1:], np.float32)
    np.add.at(G, inv[perm], g[perm])
    A[uniq] += G * G
    X[uniq] -= (np.float32(lr) * G) / np.sqrt(A[uniq])


def _plr_ordered_step(T, b, model, order, rng):
    """cf_oracle.plr_step in float32 with the dedup-sums in another order."""
    U, V, AU, AV, bias, Ab = T
    hp = M.HP[model]
    kind = 0 if model == "prigp" else 1
    t = b["tuples"]
    u, X = t[:, 0], t[:, 1:]
    Uu, VX, bX = U[u], V[X], bias[X]
    s = np.sum(Uu[:, None, :] * VX, axis=-1) + bX
    ds = np.zeros_like(s)
    for a, bb, coef, w in O.plr_terms(kind, b["coefs"], t.shape[0], hp.get("alpha", 1.0), hp.get("beta", 1.0),
                                      hp.get("gamma", 1.0), np.float32):
        z = coef * (s[:, a] - s[:, bb])
        g = w * coef * (-1.0 / (1.0 + np.exp(z))).astype(np.float32)
        ds[:, a] += g
        ds[:, bb] -= g
    reg = np.float32(hp["reg"])
    _dedup32(U, AU, u, np.sum(ds[:, :, None] * VX, axis=1) + reg * Uu, 0.1, order, rng)
    _dedup32(V, AV, X.reshape(-1), (ds[:, :, None] * Uu[:, None, :] + reg * VX).reshape(-1, U.shape[1]), 0.1,
             order, rng)
    if kind == 1:
        _dedup32(bias, Ab, X.reshape(-1), (ds + reg * bX).reshape(-1), 0.1, order, rng)


def _reversed_step(T, b, model, phase):
    """One BPR / AMF step in float32 with every dedup-sum added in reverse."""
    U, V, AU, AV = T
    hp = M.HP[model]
    c_scale = None
    if model == "amf" and phase:
        pairs, negs = b["pairs"], b["negs"]
        Uu, Vi, Vj = U[pairs[:, 0]], V[pairs[:, 1]], V[negs]
        x = np.sum(Uu * Vi, axis=1)[:, None] - np.sum(Uu[:, None, :] * Vj, axis=-1)
        c_scale = (np.float32(1) + np.float32(hp["reg_adv"]) * ((x >= -80) & (x <= 1e8))).astype(np.float32)
    _, _, (ur, ug), (vr, vg) = O.bpr_loss_grads(U, V, b["pairs"], b["negs"], hp["reg"], c_scale)
    _dedup32(U, AU, ur, ug, 0.1, "reverse", None)
    _dedup32(V, AV, vr, vg, 0.1, "reverse", None)


def _band_ratio(T32, T64):
    return max(float(np.max(np.abs(a.astype(np.float64) - r) / (ATOL + RTOL * np.abs(r))))
               for a, r in zip(T32, T64))


def _oracle_step(model, T, b, phase):
    hp = M.HP[model]
    if model == "bpr":
        return O.bpr_step(T[0], T[1], T[2], T[3], b["pairs"], b["negs"], hp["reg"])
    if model == "amf" and phase == "apr":
        return O.amf_apr_step(T[0], T[1], T[2], T[3], b["pairs"], b["negs"], hp["reg"], M.APR_EPS,
                              reg_adv=hp["reg_adv"])
    if model == "amf":
        return O.amf_step(T[0], T[1], T[2], T[3], b["pairs"], b["negs"], hp["reg"], bool(phase), hp["reg_adv"])
    if model == "gbpr":
        return O.gbpr_step(T[0], T[1], T[4], T[2], T[3], T[5], b["pairs"], b["negs"], b["groups"],
                           hp["rho"], hp["reg"])
    kind = 0 if model == "prigp" else 1
    return O.plr_step(T[0], T[1], T[4], T[2], T[3], T[5], b["tuples"], b["coefs"], kind, hp["reg"],
                      hp.get("alpha", 1.0), hp.get("beta", 1.0), hp.get("gamma", 1.0))


BAND_SHAPES = [("bpr", 1, 0, 0), ("bpr", 3, 0, 0), ("bpr", 5, 0, 0), ("amf", 1, 0, 0), ("amf", 5, 0, 1),
               ("amf", 3, 0, 1), ("amf", 1, 0, "apr"), ("amf", 3, 0, "apr"), ("amf", 5, 0, "apr"),
               ("gbpr", 5, 1, 0), ("gbpr", 2, 3, 0), ("gbpr", 1, 16, 0), ("gbpr", 1, 1, 0),
               ("prigp", 3, 0, 0), ("cplr", 2, 0, 0)]


@pytest.mark.parametrize("table,d", [("small", 7), ("small", 64), ("small", 129), ("small", 256),
                                     ("large", 100), ("large", 128)])
@pytest.mark.parametrize("model,W,G,phase", BAND_SHAPES)
def test_float32_oracle_stays_in_half_the_band(model, W, G, phase, table, d):
    """float32 arithmetic alone (cf_oracle on float32 tables, natural order;
    BPR / AMF also with every dedup-sum reversed, the tuple models reversed
    and shuffled) stays within half of
    conftest.assert_close's default band around the float64 oracle after one
    and after three steps on every edge batch.  A condition on the input: if
    it fails, the batch is wrong, not the cap."""
    nu, ni = _tables_of(model, W, G, table)
    bs = M.edge_batches(model, W, G, nu, ni)
    U, V, b = _init(model, nu, ni, d)
    acc = lambda x: np.full_like(x, 0.1)                      # noqa: E731
    T32 = [U.copy(), V.copy(), acc(U), acc(V), b.copy(), acc(b)]
    T64 = [t.astype(np.float64) for t in T32]
    R32 = [t.copy() for t in T32[:4]] if model in ("bpr", "amf") and phase != "apr" else None
    P32 = ([[t.copy() for t in T32], [t.copy() for t in T32]] if model in M.TUPLE_MODELS else [])
    prng = np.random.RandomState(9)
    worst = []
    for s, bt in enumerate(bs):
        lo = _oracle_step(model, T64, bt, phase)
        l32 = _oracle_step(model, T32, bt, phase)
        assert abs(l32 - lo) <= 0.5e-5 * abs(lo), (s, l32, lo)
        if R32 is not None:
            _reversed_step(R32, bt, model, phase)
        for P, order in zip(P32, ("reverse", "shuffle")):
            _plr_ordered_step(P, bt, model, order, prng)
        if s in (0, 2):
            worst += [_band_ratio([P[k] for k in (0, 1, 2, 3, 4, 5)], T64) for P in P32]
            worst.append(_band_ratio(T32, T64))
            if R32 is not None:
                worst.append(_band_ratio(R32, T64[:4]))
    print("%s W%d G%d d%d %s: float32 oracle / band %s" % (model, W, G, d, table,
                                                           " ".join("%.3f" % w for w in worst)))
    assert max(worst) <= 0.5, worst


@pytest.mark.parametrize("table,d", [("small", 7), ("small", 64), ("small", 256), ("large", 128)])
@pytest.mark.parametrize("W", [1, 3, 5])
def test_cml_bound_leaves_its_existing_share_unbounded(W, table, d):
    """CML: a pair within rounding of a branch point may take either branch in
    float32, so fp32_bound.cml_step_bounded leaves its rows unbounded; on the
    edge batches that is at most the share conftest.LocalStepCheck already
    allows (1 % of the touched rows, or 2), from the float32 oracle's own
    trajectory."""
    nu, ni = _tables_of("cml", W, 0, table)
    bs = M.edge_batches("cml", W, 0, nu, ni)
    U, V, _ = _init("cml", nu, ni, d)
    T32 = [U, V, np.full_like(U, 0.1), np.full_like(V, 0.1)]
    hp = M.HP["cml"]
    n_bad = 0
    for bt in bs:
        L = [t.astype(np.float64) for t in T32]
        E = FB.zero_bounds(L[0], L[1], acc_exact=True)
        FB.cml_step_bounded(*L, E, bt["pairs"], bt["negs"], margin=hp["margin"], reg_cov=hp["reg_cov"],
                            clip_norm=hp["clip_norm"], use_rank_weight=hp["use_rank_weight"])
        for t in FB.TABLES:
            bad = (~np.isfinite(E[t])).any(axis=1)
            touched = (E[t] != 0).any(axis=1)
            n_bad += int(bad.sum())
            assert bad.sum() <= max(2, 0.01 * touched.sum()), (t, int(bad.sum()), int(touched.sum()))
        O.cml_step(*T32, bt["pairs"], bt["negs"], hp["margin"], hp["reg_cov"], hp["clip_norm"],
                   use_rank_weight=hp["use_rank_weight"])
    print("cml W%d d%d %s: %d rows unbounded" % (W, d, table, n_bad))
