"""Host model of the training step's kernel dispatch, the matrix of cases
that runs every gradient instantiation at its width edges, and the host-fed
edge batches those cases step on.  No GPU.

``plan_of`` restates in Python what the engine decides at run time:

* ``grad_plan``, ``fast_w``, ``lds_path`` (csrc/cf_kernels.hip) and
  ``epl_for`` / ``with_epl`` (csrc/cf_kernels_impl.h): which gradient kernel
  a step takes, its compile-time W, pairs per group and slots per lane;
* the FULL rules of ``launch_sort_e`` and ``launch_grad_fast``
  (csrc/cf_kernels_impl.h) and the vector row layout (``vec_rows``);
* ``psort_possible`` / ``psort_active``, the ``dense_items`` /
  ``dense_users`` rule of ``apply_args`` and the flags of ``cf_step_path``
  (csrc/cf_engine.cpp).

A kernel instantiation is the tuple ``Plan.inst`` = (kind, model,
compile-time W, EPL, layout, FULL, FX).  tests/test_step_matrix.py requires
every tuple ``plan_of`` can produce over the ABI's ranges to be produced by an
entry of ``CASES``; tests/test_gpu_step_matrix.py runs each entry on the
device against the float64 oracle.  A new instantiation therefore needs a row
in ``CASES``.
"""
import collections
import functools

import numpy as np

kGL = 16                 # lanes per row group
kGroupsPerBlock = 16
kPairsPerBlock = 32
kPsortPPB = 16           # positions per positive-sorted gradient block
kPsortTile = 2048        # entries per psort scan tile
kDetTile = 64            # slots per deterministic whole-tile sum
FAST_PAIRS_W1, FAST_PAIRS_W5, FAST_PAIRS_GBPR_W5, SORT_TILES = 1, 1, 2, 1
CAP_U, CAP_V, CAP_P = 2, 32, 8
PSORT_AUTO_B = 1 << 18
MAX_D, MAX_W, MAX_W_CML, MAX_G = 256, 64, 16, 16

PAIR_MODELS = ("bpr", "amf", "cml", "gbpr")
TUPLE_MODELS = {"prigp": 3, "cplr": 2}       # n_neg: the tuple holds n_neg + 1 items

Plan = collections.namedtuple(
    "Plan", "kind model wt pairs_per_group epl layout full fx flags dense_items dense_users refused")
Plan.inst = property(lambda p: (p.kind, p.model, p.wt, p.epl, p.layout, p.full, p.fx))


def epl_for(d):
    e = (d + kGL - 1) // kGL
    return 1 if e <= 1 else 2 if e <= 2 else 4 if e <= 4 else 8 if e <= 8 else 16


def _lds_path(model, d, W, G, grad_path, apr, srec):
    if apr:
        return False
    if grad_path not in (0, 3) or W != 5 or srec:
        return False
    if model in ("bpr", "amf", "cml"):
        return d == 128
    if model == "gbpr":
        return d == 64 and G == 1
    return False


def _fast_w(model, d, W, G, grad_path, apr, srec):
    if apr:
        return 0
    if _lds_path(model, d, W, G, grad_path, apr, srec):
        return 5
    ok = (grad_path != 1 and epl_for(d) <= 8 and (model != "gbpr" or G == 1)
          and not (grad_path == 0 and model == "cml" and W == 5))
    return W if ok and W in (1, 5) else 0


def _grad_plan(model, d, W, G, grad_path, apr, srec, draw):
    """(kind, compile-time W, pairs per 16-lane group) as grad_plan has them."""
    e = epl_for(d)
    fw = _fast_w(model, d, W, G, grad_path, apr, srec)
    if model in TUPLE_MODELS:
        return ("tuple" if W in (2, 3) and not srec else None), W, kPairsPerBlock // kGroupsPerBlock
    if srec:
        one = (fw == 1 and FAST_PAIRS_W1 == 1) or (fw == 5 and FAST_PAIRS_W5 == 1)
        return ("sorted" if one and model != "gbpr" else None), fw, 1
    if _lds_path(model, d, W, G, grad_path, apr, srec) and not draw:
        return "lds", 5, 1
    if fw != 0:
        P = FAST_PAIRS_W1 if fw == 1 else FAST_PAIRS_GBPR_W5 if (model == "gbpr" and e <= 4) else FAST_PAIRS_W5
        return "phased", fw, P
    wt = 1 if W == 1 else 5 if (W == 5 and e <= 8) else 0
    return ("apr" if apr and model == "amf" else "generic"), wt, kPairsPerBlock // kGroupsPerBlock


def plan_of(model, d, W, G, options=None):
    """What the engine does with a step of ``options['B']`` pairs.

    options: grad_path (0), pos_sort (2 = auto), deterministic (0),
    item_slots (None = the engine's default: records from d = 128 up, never
    with apr), pipeline (1), phase (0; AMF), amf_mode ("reference"), B,
    n_users, n_items, draw (False: the launch carries no fused draw).
    """
    o = dict(grad_path=0, pos_sort=2, deterministic=0, item_slots=None, pipeline=1, phase=0,
             amf_mode="reference", B=1, n_users=943, n_items=1682, draw=False)
    o.update(options or {})
    tup = model in TUPLE_MODELS
    apr_mode = o["amf_mode"] == "apr"
    refused = (not 1 <= d <= MAX_D or not 1 <= W <= MAX_W or (model == "cml" and W > MAX_W_CML)
               or (model == "gbpr" and not 1 <= G <= MAX_G) or (tup and W != TUPLE_MODELS[model])
               or (apr_mode and model != "amf")
               or (apr_mode and (o["deterministic"] == 1 or o["item_slots"] == 1)))
    G = G if model == "gbpr" else 0
    B, nu, ni = o["B"], o["n_users"], o["n_items"]
    item_recs = (d >= 128 and not apr_mode) if o["item_slots"] is None else bool(o["item_slots"])
    det = bool(o["deterministic"])
    apr = model == "amf" and o["phase"] == 1 and apr_mode
    gp = o["grad_path"]
    possible = (o["pos_sort"] != 0 and not item_recs and not apr_mode and model in ("bpr", "amf", "cml")
                and nu * CAP_U <= 2 ** 31 - 1 and d <= 128 and W in (1, 5))
    active = (possible and not (o["pos_sort"] == 2 and B < PSORT_AUTO_B) and o["pipeline"] != 2
              and gp != 1 and not (gp == 0 and model == "cml" and W == 5))
    kind, wt, ppg = _grad_plan(model, d, W, G, gp, apr, active, o["draw"])
    kind0 = _grad_plan(model, d, W, G, gp, apr, False, False)[0]      # what cf_step_path looks at
    if kind is None:
        refused = True
    e = epl_for(d)
    fx = det and active
    whole = d == kGL * e
    if kind == "sorted":
        full = e >= 4 and whole and not (e == 8 and fx)
    elif kind == "phased":
        full = e == 4 and whole and not o["draw"]
    else:
        full = False            # no such template argument: the row helpers test d at run time
    if kind == "lds":
        e = 4 if model == "gbpr" else 8
    layout = "vector" if e >= 8 and whole else "scalar"
    flags = dict(phased=kind0 in ("phased", "lds"), pos_sort=active, lds=(not active and kind0 == "lds"),
                 deterministic=det, item_records=item_recs)
    dense_items = dense_users = False
    if active:
        dense_items = ni <= 2 * B * (1 + W)
        dense_users = nu <= 2 * B * (1 + G)
    elif not det and model in ("bpr", "amf", "cml"):
        dense_items = ni <= 2 * B * (1 + W)
    return Plan(kind, model, wt, ppg, e, layout, full, fx, flags, dense_items, dense_users, refused)


# ---------------------------------------------------------------------------
# the matrix
# ---------------------------------------------------------------------------
CORE = (7, 16, 24, 32, 40, 64, 100, 128)      # a ragged and a full width per EPL 1..8
WIDE = (200, 256)                             # EPL 16
EDGE_D = (17, 33, 65, 127, 129)               # one element in the last slot / one lane masked / one past
LARGE_D = (7, 64, 100, 128)
# one ragged and one full width per (EPL, layout): the rows that exist only
# to reach the run-time-W instantiations (compile-time W = 0)
PER_EPL = (7, 24, 40, 100, 128, 200, 256)

HP = {"bpr": dict(reg=0.05), "amf": dict(reg=0.05, reg_adv=0.25),
      "cml": dict(margin=1.0, reg_cov=1.0, clip_norm=1.0, use_rank_weight=True),
      "gbpr": dict(rho=0.4, reg=0.01), "prigp": dict(reg=0.01, alpha=0.5),
      "cplr": dict(reg=0.02, alpha=0.7, beta=1.3, gamma=0.5)}
APR_EPS = 0.5
# stddev of the initial tables of the models whose three-step trajectory is
# held to the strict band.  acc' = acc + G^2 carries 2 G dG, and dG of a
# 129-occurrence row grows with the size of its terms: at 0.1 the float32
# oracle's own sums reach 0.32 of the band for BPR and 0.70 for AMF's
# adversarial phase (every term scaled by 1 + reg_adv) at W = 5
# (tests/test_step_matrix.py), and the device's sums -- another order, a
# 6-ulp logistic -- 0.84; at 0.05 both stay below half of it
INIT_STD = {"bpr": 0.05, "amf": 0.05}

BATCH_SIZES = (587, 576, 587)     # 576 = 9 * 64: nU % 64 == 0 in the second batch only
B_MAX = max(BATCH_SIZES)

Case = collections.namedtuple("Case", "path model d W G opts phase amf_mode slot_max item_slots table")


def case_id(c):
    s = "%s-%s-d%d-w%d" % (c.path, c.model, c.d, c.W)
    if c.model == "gbpr":
        s += "g%d" % c.G
    if c.model == "amf":
        s += "-ph%d" % c.phase
    if c.slot_max is not None:
        s += "-cap%d" % c.slot_max
    if c.opts.get("deterministic") and c.path not in ("det", "detsorted"):
        s += "-det"
    if c.item_slots is not None:
        s += "-rec%d" % c.item_slots
    return s + "-" + c.table


def table_shape(c):
    """(n_users, n_items): ml-100k fold 1, or tables past twice the batch's
    occurrences on both sides (odd sizes), where the applies scan the
    occurrences for owners instead of visiting every row."""
    if c.table == "small":
        return 943, 1682
    G = c.G if c.model == "gbpr" else 0
    return 2 * B_MAX * (1 + G) + 63, 2 * B_MAX * (1 + c.W) + 31


def case_options(c):
    """The plan_of options of a case (batch size: the first edge batch's)."""
    nu, ni = table_shape(c)
    o = dict(c.opts, phase=c.phase, amf_mode=c.amf_mode, item_slots=c.item_slots, B=BATCH_SIZES[0],
             n_users=nu, n_items=ni)
    return o


def case_plan(c, B=None):
    o = case_options(c)
    if B is not None:
        o["B"] = B
    return plan_of(c.model, c.d, c.W, c.G, o)


def _build_cases():
    out = []

    def add(path, model, W, G, widths, opts, slots=(0, 1), phase=0, amf_mode="reference", slot_max=None,
            large=True):
        for isl in slots:
            for d in widths:
                out.append(Case(path, model, d, W, G, opts, phase, amf_mode, slot_max, isl, "small"))
            if large:
                for d in LARGE_D:
                    if d in widths:
                        out.append(Case(path, model, d, W, G, opts, phase, amf_mode, slot_max, isl, "large"))

    cw, cwe = CORE + WIDE, CORE + WIDE + EDGE_D
    c128 = CORE + tuple(d for d in EDGE_D if d <= 128)
    # generic: grad_path 1
    gen = dict(grad_path=1)
    add("generic", "bpr", 1, 0, cwe, gen)
    for W in (3, 5):
        add("generic", "bpr", W, 0, cw, gen)
    for m in ("amf", "cml"):
        for W in (1, 5):
            add("generic", m, W, 0, cw, gen, phase=1 if m == "amf" else 0)
        # W = 3: the compile-time W = 0 instantiations (W is read at run time)
        add("generic", m, 3, 0, PER_EPL, gen, slots=(0,), phase=1 if m == "amf" else 0, large=False)
    for W, G in ((5, 1), (2, 3), (1, 16)):
        add("generic", "gbpr", W, G, cw, gen)
    # phased: grad_path 2
    ph = dict(grad_path=2)
    add("phased", "bpr", 1, 0, c128, ph)
    add("phased", "bpr", 5, 0, CORE, ph)
    for m in ("amf", "cml"):
        for W in (1, 5):
            add("phased", m, W, 0, CORE, ph, phase=1 if m == "amf" else 0)
    for W, G in ((5, 1), (1, 1)):
        add("phased", "gbpr", W, G, CORE, ph)
    # sorted: pos_sort 1 (needs gradient rows: item_slots 0)
    ps = dict(pos_sort=1)
    add("sorted", "bpr", 1, 0, c128, ps, slots=(0,))
    add("sorted", "bpr", 5, 0, CORE, ps, slots=(0,))
    for W in (1, 5):
        for phase in (0, 1):
            add("sorted", "amf", W, 0, CORE, ps, slots=(0,), phase=phase)
    add("sorted", "cml", 1, 0, CORE, ps, slots=(0,))
    add("sorted", "cml", 5, 0, CORE, dict(pos_sort=1, grad_path=2), slots=(0,))
    # deterministic (pos_sort left on auto: off at these batch sizes)
    det = dict(deterministic=1)
    for m, W, G in (("bpr", 1, 0), ("bpr", 5, 0), ("amf", 5, 0), ("cml", 1, 0), ("cml", 5, 0),
                    ("gbpr", 5, 1), ("gbpr", 2, 3)):
        add("det", m, W, G, cw, det, phase=1 if m == "amf" else 0)
    # deterministic + sorted: the fixed-point form
    dps = dict(deterministic=1, pos_sort=1)
    for m in ("bpr", "amf"):
        for W in (1, 5):
            add("detsorted", m, W, 0, CORE, dps, slots=(0,), phase=1 if m == "amf" else 0)
    # CML's fixed-point form: grad_sort_kernel<CML, ..., FX>
    add("detsorted", "cml", 1, 0, CORE, dps, slots=(0,))
    add("detsorted", "cml", 5, 0, CORE, dict(dps, grad_path=2), slots=(0,))
    # LDS-staged: auto, with gradient rows and with item records (the default at d = 128)
    for m in ("bpr", "amf", "cml"):
        add("lds", m, 5, 0, (128,), {}, phase=1 if m == "amf" else 0)
    add("lds", "gbpr", 5, 1, (64,), {})
    # apr
    add("apr", "amf", 1, 0, CORE + WIDE, {}, slots=(None,), phase=1, amf_mode="apr")
    add("apr", "amf", 5, 0, CORE + (256,), {}, slots=(None,), phase=1, amf_mode="apr")
    add("apr", "amf", 3, 0, PER_EPL, {}, slots=(None,), phase=1, amf_mode="apr", large=False)
    # what apr does not combine with: the engine must say so
    out.append(Case("apr", "amf", 32, 5, 0, dict(deterministic=1), 1, "apr", None, None, "small"))
    out.append(Case("apr", "amf", 32, 5, 0, {}, 1, "apr", None, 1, "small"))
    # tuples
    for m, W in TUPLE_MODELS.items():
        for cap in (32, 2):
            add("tuple", m, W, 0, cwe, {}, slot_max=cap)
    return tuple(out)


CASES = _build_cases()


# ---------------------------------------------------------------------------
# edge batches
# ---------------------------------------------------------------------------
USER_COUNTS = (1, 2, 3, 4, 5, 9, 33)
POS_COUNTS = (1, 2, 7, 8, 9, 16, 17, 128, 129)
NEG_COUNTS = (1, 2, 4, 5, 31, 32, 33, 127, 128, 129)
MIXED_COUNTS = ((1, 1), (3, 3))     # (positive, negative) occurrences of the items that are both
REGION = 64                         # item ids one batch's engineered rows are taken from


def _fill(total, rows_left, allowed):
    """Occurrence counts from ``allowed`` that add up to ``total`` on at most
    ``rows_left`` rows, as many singletons as fit."""
    out = []
    allowed = sorted(allowed)
    while total > 0:
        assert len(out) < rows_left, "not enough rows for the prescribed counts"
        left = max(1, rows_left - len(out) - 8)      # spare rows for the remainder
        fit = [a for a in allowed if a * left >= total]
        c = fit[0] if fit else allowed[-1]
        if c > total:
            c = max(a for a in allowed if a <= total)
        out.append(c)
        total -= c
    return out


def _pad_counts(need):
    """``need`` (< 64) occurrences as negative-only items with listed counts."""
    out = []
    for c in (33, 32, 31, 5, 4, 2, 1):
        while need >= c:
            out.append(c)
            need -= c
    return out


def det_split(keys, n_first):
    """The deterministic apply's view of one sorted key array (users, then
    items offset by n_users): for every row of at least 127 slots its
    (key, ns, global start, head, whole tiles, tail) against 64-position
    tiles, as apply_row splits a row of ns >= 2 * 64 (a shorter row is summed
    slot by slot: tiles is None)."""
    keys = np.sort(np.asarray(keys, np.int64), kind="stable")
    uniq, start, cnt = np.unique(keys, return_index=True, return_counts=True)
    out = []
    for k, gs, ns in zip(uniq.tolist(), start.tolist(), cnt.tolist()):
        if ns < 127:
            continue
        if ns < 2 * kDetTile:
            out.append((k, ns, gs, ns, None, 0))
            continue
        ge = gs + ns
        qa, qb = -(-gs // kDetTile), ge // kDetTile
        out.append((k, ns, gs, qa * kDetTile - gs, qb - qa, ge - qb * kDetTile))
    return out


def psort_blocks(pos_items, n_items):
    """Gradient blocks (16 sorted positions each) every positive item's run spans."""
    cnt = np.bincount(np.asarray(pos_items), minlength=n_items)
    off = np.cumsum(cnt) - cnt
    return np.where(cnt > 0, (off + cnt - 1) // kPsortPPB - off // kPsortPPB + 1, 0)


def _one_batch(rng, s, B, W, G, n_users, n_items, prev_hot_users, prev_hot_items):
    nU = B * (1 + G)
    base = REGION * (2 - s)                     # the engineered ids move down, batch by batch
    pool_lo = 3 * REGION
    # ---- items: the engineered region, in id order --------------------------------
    nxt = [base]

    def new_id():
        nxt[0] += 1
        assert nxt[0] <= base + REGION
        return nxt[0] - 1

    pos, neg = {}, {}                           # item id -> occurrences
    L = new_id(); pos[L] = 128                  # offP = 0: exactly capP blocks; global start nU
    a1 = new_id(); pos[a1] = 1
    a2 = new_id(); pos[a2] = 128                # offP = 129: capP + 1 blocks
    cur = nU + 257
    for c in _pad_counts((kDetTile - 1 - cur) % kDetTile):
        neg[new_id()] = c
    p129 = new_id(); pos[p129] = 129            # starts at 63 mod 64, ends on a tile boundary
    n128 = new_id(); neg[n128] = 128            # starts and ends on one
    n129 = new_id(); neg[n129] = 129            # starts on one
    n127 = new_id(); neg[n127] = 127
    # ---- items: the pool -------------------------------------------------------------
    prev = [i for i in prev_hot_items if i >= base + REGION]
    fresh = [i for i in rng.permutation(np.arange(pool_lo, n_items)).tolist() if i not in set(prev)]
    take = iter(fresh)
    for c in POS_COUNTS:
        if c < 128:
            pos[next(take)] = c
    for c in NEG_COUNTS:
        if c < 127 and c not in neg.values():
            neg[next(take)] = c
    m33, x11, yji = next(take), next(take), next(take)
    pos[m33], neg[m33] = 3, 3                   # three positive and three negative occurrences
    pos[x11], neg[x11] = 1, 1                   # one pair's positive, another's only negative
    pos[yji], neg[yji] = 1, 1                   # a pair with j == i
    zrep = None
    if W >= 2:
        zrep = next(take)
        neg[zrep] = 2                           # one pair repeats this negative
    # what is left: last batch's hot rows as singletons first, then fresh rows
    rest = prev + list(take)
    need_p = B - sum(pos.values())
    assert need_p >= 0
    fill_p = sorted(_fill(need_p, len(rest) // 4, [c for c in POS_COUNTS if c < 128]))
    for c in fill_p:
        pos[rest.pop(0)] = c
    need_n = B * W - sum(neg.values())
    assert need_n >= 0, "batch too small for the prescribed negative counts"
    fill_n = sorted(_fill(need_n, len(rest), [c for c in NEG_COUNTS if c < 127]))
    for c in fill_n:
        neg[rest.pop(0)] = c
    # ---- pairs -----------------------------------------------------------------------
    order = rng.permutation(B)                  # hot occurrences spread over the gradient blocks
    i_col = np.empty(B, np.int64)
    i_col[order] = np.repeat(list(pos.keys()), list(pos.values()))
    j = np.full((B, W), -1, np.int64)
    p_y = int(np.flatnonzero(i_col == yji)[0])
    j[p_y, 0] = yji
    special = {yji: 1}
    if zrep is not None:
        p_z = int(np.flatnonzero(i_col == a1)[0])
        j[p_z, 0] = j[p_z, 1] = zrep
        special[zrep] = 2
    bag = np.repeat(list(neg.keys()), [c - special.get(k, 0) for k, c in neg.items()])
    bag = bag[rng.permutation(bag.shape[0])]
    free = np.flatnonzero(j.reshape(-1) < 0)
    assert free.shape[0] == bag.shape[0]
    jf = j.reshape(-1)
    jf[free] = bag
    # x11's negative occurrence belongs to another pair than its positive one
    px = int(np.flatnonzero(i_col == x11)[0])
    qx = int(np.flatnonzero(jf == x11)[0])
    if qx // W == px:
        other = next(int(q) for q in free if q // W != px and jf[q] not in (x11, yji, zrep))
        jf[qx], jf[other] = jf[other], jf[qx]
    # ---- users -----------------------------------------------------------------------
    uprev = list(prev_hot_users)[:32]
    ufresh = [u for u in rng.permutation(n_users).tolist() if u not in set(uprev)]
    utake = iter(ufresh)
    Uall = np.full((B, 1 + G), -1, np.int64)     # column 0: u; the rest: the pair's group
    counts = {}
    rows = rng.permutation(B).tolist()
    if G >= 1:
        up, ur = next(utake), next(utake)
        r = [rows.pop() for _ in range(4)]
        Uall[r[0], 0] = up                       # u in one pair, a group member in two others
        Uall[r[1], 1] = Uall[r[2], 1] = up
        Uall[r[3], 0] = Uall[r[3], 1] = ur       # a group member equal to the pair's own u
        counts[up], counts[ur] = 3, 2
        if G >= 2:
            uq = next(utake)
            r4 = rows.pop()
            Uall[r4, 1] = Uall[r4, 2] = uq       # one user twice in a group
            counts[uq] = 2
    for c in USER_COUNTS:
        if c not in counts.values():
            counts[next(utake)] = c
    placed = {k: int((Uall == k).sum()) for k in counts}
    urest = uprev + list(utake)
    need_u = nU - sum(counts.values())
    for c in sorted(_fill(need_u, len(urest), USER_COUNTS)):
        counts[urest.pop(0)] = c
    ubag = np.repeat(list(counts.keys()), [c - placed.get(k, 0) for k, c in counts.items()])
    ubag = ubag[rng.permutation(ubag.shape[0])]
    uf = Uall.reshape(-1)
    ufree = np.flatnonzero(uf < 0)
    assert ufree.shape[0] == ubag.shape[0]
    uf[ufree] = ubag
    pairs = np.stack([Uall[:, 0], i_col], 1).astype(np.int32)
    negs = j.astype(np.int32)
    groups = Uall[:, 1:].astype(np.int32) if G >= 1 else None
    keys = np.concatenate([Uall.reshape(-1), n_users + i_col, n_users + jf])
    named = dict(L=L, a1=a1, a2=a2, p129=p129, n128=n128, n129=n129, n127=n127, m33=m33, x11=x11, yji=yji,
                 zrep=zrep)
    # the rows the next batch should meet as singletons, hottest first
    hot_u = sorted((k for k, c in counts.items() if c > 1), key=lambda k: -counts[k])
    tot = {k: pos.get(k, 0) + neg.get(k, 0) for k in set(pos) | set(neg)}
    hot_i = sorted((k for k, c in tot.items() if c > 1), key=lambda k: (-tot[k], k))
    return dict(pairs=pairs, negs=negs, groups=groups, B=B, nU=nU, named=named,
                det=det_split(keys, n_users), hot_users=hot_u, hot_items=hot_i)


@functools.lru_cache(maxsize=None)
def edge_batches(model, W, G, n_users, n_items, seed=0):
    """Three host-fed batches with prescribed occurrence counts per row (see
    USER_COUNTS, POS_COUNTS, NEG_COUNTS, MIXED_COUNTS) whose hot rows move
    between the batches: the rows one batch touches more than once, hottest
    first, are singletons of the next, so whatever a step leaves behind for a
    row -- a count, a slot row, a partial row, an accumulator row -- meets a
    step that treats the row as new.  That reaches as far as the next batch
    has singletons: every engineered and named row and every row of the
    prescribed counts always (tests/test_step_matrix.py asserts the 40 hottest
    items and the 32 hottest users); of the filler rows with two to five
    occurrences that a small table needs at W >= 3 only the first; and no user
    at all on the small table at G >= 3, where 943 users share 2,300 to 10,000
    occurrences and one singleton is all the counts leave room for.  Tuple models
    get ``tuples`` [B, 2 + n_neg] (and CPLR ``coefs``) from the same rows.
    Each batch carries ``det``: det_split of its sorted keys.  The result is
    shared between tests: treat it as read-only."""
    G = G if model == "gbpr" else 0
    rng = np.random.RandomState(1000 * seed + 17 * W + G + 1)
    out, hu, hi = [], [], []
    for s, B in enumerate(BATCH_SIZES):
        b = _one_batch(rng, s, B, W, G, n_users, n_items, hu, hi)
        hu, hi = b["hot_users"], b["hot_items"]
        if model in TUPLE_MODELS:
            b["tuples"] = np.concatenate([b["pairs"], b["negs"]], 1).astype(np.int32)
            # CPLR's confidence coefficients scale every term of a row sum, and the error of
            # acc' = acc + G^2 grows with the square of the terms: kept in [0, 0.5), so that a
            # 129-occurrence bias sum stays inside the band in any float32 summation order
            # (gamma(1, 1) draws up to 8.9 put the float32 oracle itself at 0.85 of it, on
            # acc_bias of the 127-negative item at d = 7; draws up to 2 put the device at 1.27
            # of it on one element, acc_bias of a 129-occurrence item in the third step of
            # cplr d = 64, slot_max 32, records, large tables: 4.05147505 against 4.05142231,
            # G ~ 2 summed from terms of up to 3, the occurrences past slot 32 by float atomics)
            b["coefs"] = rng.uniform(0.0, 0.5, (B, 2)).astype(np.float32) if model == "cplr" else None
        for k in ("pairs", "negs", "groups", "tuples", "coefs"):
            if b.get(k) is not None:
                b[k].setflags(write=False)
        out.append(b)
    return tuple(out)


def occurrence_counts(b, n_users, n_items):
    """(user counts, positive counts, negative counts) per row of one batch."""
    u = b["pairs"][:, 0] if b["groups"] is None else np.concatenate([b["pairs"][:, 0], b["groups"].reshape(-1)])
    return (np.bincount(u, minlength=n_users), np.bincount(b["pairs"][:, 1], minlength=n_items),
            np.bincount(b["negs"].reshape(-1), minlength=n_items))


def tile_edge_ids(n_items):
    """(the ids at the scan tile's edge and the table's end, their neighbours)."""
    edge = sorted(i for i in {0, 2046, 2047, n_items - 1} if i < n_items)
    near = sorted(i for i in {1, 2045, 2048, n_items - 2} if i < n_items and i not in edge)
    return edge, near


def tile_edge_batches(n_users, n_items, W, B=300, seed=0):
    """Two batches for the psort scan's tile edges and the radix sort's key
    width: item ids 0, 2046, 2047 and n_items - 1 each as a duplicated
    positive (three times) and negative (twice) in the first batch and once
    each in the second (and the other way round for their neighbours 1, 2045,
    2048 and n_items - 2 where they exist), the highest user id in both."""
    rng = np.random.RandomState(seed + n_items)
    edge, near = tile_edge_ids(n_items)
    out = []
    for s in range(2):
        dup, single = (edge, near) if s == 0 else (near, edge)
        u = rng.permutation(n_users)[:B].astype(np.int64)
        u[0] = u[1] = n_users - 1
        other = np.setdiff1d(np.arange(n_items), edge + near)      # the fill never meets the placed ids
        i = other[rng.randint(other.shape[0], size=B)].astype(np.int64)
        j = other[rng.randint(other.shape[0], size=(B, W))].astype(np.int64)
        r = iter(rng.permutation(B).tolist())
        for it in dup:
            for _ in range(3):
                i[next(r)] = it
            for _ in range(2):
                j[next(r), rng.randint(W)] = it
        for it in single:
            i[next(r)] = it
        for it in single:
            j[next(r), 0] = it
        out.append((np.stack([u, i], 1).astype(np.int32), j.astype(np.int32)))
    return out


def tiny_csr(n_users, n_items):
    """A CSR with one interaction per user: host-fed steps read none of it."""
    ip = np.arange(n_users + 1, dtype=np.int64)
    ix = (np.arange(n_users, dtype=np.int64) % n_items).astype(np.int32)
    return ip, ix
