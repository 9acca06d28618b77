"""MF / SVD / WRMF step figures on one GPU:

    timeout -k 10 600 python tools/pointwise_ab.py [--out FILE] [--quick]

Measured, each after a warm-up of the same shape, as the median of --reps
windows of a host clock around calls that end in a device synchronise
(take_loss syncs):

  step, driver shapes  ml-100k fold 1 with raw ratings
                       (tests/golden/rating_stream.npz): MF d = 100, B = 1000
                       and SVD d = 32, B = 100 on the exact sampler at negRatio
                       0 (about ten / two users per batch); WRMF d = 100,
                       B = 100 + 100 negatives, weight 2, on the binarised fold;
  step, large batch    B = 65,536, d = 64 on cfg2-like tables (1M users, 100K
                       items), MF and SVD, twice: "runs" gives every user 50
                       consecutive rows as sampler_rating's batches do, "uniform"
                       draws every row's user uniformly.

These are whole-call times (host range check and counting sort, the id copy,
every launch), not kernel times.  The tool does not time single launches (the
C ABI has no hook around a step's launches): the time per launch comes from a separate
``rocprofv3 --kernel-trace --stats -- python tools/pointwise_ab.py --quick``
run.  Beside each figure the tool prints what the algorithm needs, computed
from the shapes: per batch row two gathered rows, per distinct user and item
row one accumulator row read and two rows written (SVD: K and its accumulator
read and written once), so that a figure can be held against HBM bandwidth.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def step_bytes(batches, d, svd):
    """Mean bytes one step must move: 2 gathered rows per batch row, 1 row
    read + 2 written per distinct table row, K and AK read and written."""
    tot = 0.0
    for ui, _ in batches:
        uniq = len(np.unique(ui[:, 0])) + len(np.unique(ui[:, 1]))
        tot += 4.0 * d * (2 * len(ui) + 3 * uniq) + (16.0 * d * d if svd else 0.0)
    return tot / len(batches)


def time_steps(eng, batches, n_steps, reps):
    def window():
        for s in range(n_steps):
            eng.step(*batches[s % len(batches)], return_loss=False)
        eng.take_loss()
    window()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        window()
        out.append((time.perf_counter() - t0) / n_steps)
    return out


def summary(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


def figure(eng, batches, d, svd, n_steps, reps):
    ts = time_steps(eng, batches, n_steps, reps)
    nbytes = step_bytes(batches, d, svd)
    users = float(np.mean([len(np.unique(ui[:, 0])) for ui, _ in batches]))
    return {"ms_per_step": {k: 1e3 * v for k, v in summary(ts).items()}, "bytes_per_step": nbytes,
            "bytes_per_s": nbytes / statistics.median(ts), "rows_per_s": len(batches[0][0]) / statistics.median(ts),
            "distinct_users_per_batch": users}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="one short window per figure (profiler runs)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import scipy.sparse as sp
    from collaborativefilteringusingtensorflow_amd import _native as N
    from collaborativefilteringusingtensorflow_amd._pointwise import PointwiseEngine
    from collaborativefilteringusingtensorflow_amd.sampler_rating import ExactSampler
    if N.device_count() < 1:
        raise SystemExit("pointwise_ab: no HIP device visible")
    reps = 1 if args.quick else args.reps
    res = {}

    # -- the drivers' shapes ---------------------------------------------------------
    g = np.load(os.path.join(ROOT, "tests", "golden", "rating_stream.npz"))
    raw = sp.csr_matrix((g["tra_ratings"].astype(np.float64), g["tra_indices"].astype(np.int32),
                         g["tra_indptr"].astype(np.int64)), shape=(943, 1682))
    z = np.load(os.path.join(ROOT, "tests", "golden", "ml100k_fold1.npz"))
    binar = sp.csr_matrix((np.ones(len(z["train_indices"])), z["train_indices"], z["train_indptr"]),
                          shape=(943, 1682))
    for kind, d, B, neg, tra, weight in (("mf", 100, 1000, .0, raw, 1.0), ("svd", 32, 100, .0, raw, 1.0),
                                         ("wrmf", 100, 100, 1, binar, 2.0)):
        smp = ExactSampler(tra, negRatio=neg, batch_size=B, seed=0)
        batches = [smp._draw() for _ in range(min(256, tra.nnz // B))]
        smp.close()
        eng = PointwiseEngine(943, 1682, d, kind=kind, weight=weight, reg=0.1)
        eng.init_params(0.0, 0.1, seed=1)
        res["step_ml100k_%s_d%d_B%d" % (kind, d, len(batches[0][0]))] = figure(
            eng, batches, d, kind == "svd", 200 if args.quick else 4000, reps)
        eng.close()

    # -- B = 65,536 on cfg2-like tables, d = 64 ----------------------------------------
    nu, ni, d, B = 1000000, 100000, 64, 65536
    rng = np.random.RandomState(3)
    shapes = {}
    for name in ("runs", "uniform"):
        batches = []
        for _ in range(8):
            if name == "runs":   # 50 consecutive rows per user, as sampler_rating's slices
                users = np.repeat(rng.choice(nu, (B + 49) // 50, replace=False), 50)[:B]
            else:
                users = rng.randint(0, nu, B)
            ui = np.stack([users, rng.randint(0, ni, B)], 1).astype(np.int32)
            p = rng.permutation(B)   # shuffled inside the batch, as the sampler leaves it
            batches.append((ui[p], rng.randint(1, 6, B).astype(np.float32)))
        shapes[name] = batches
    for kind in ("mf", "svd"):
        eng = PointwiseEngine(nu, ni, d, kind=kind, reg=0.1)
        eng.init_params(0.0, 0.1, seed=1)
        for name, batches in shapes.items():
            res["step_1M_100K_%s_d64_B65536_%s" % (kind, name)] = figure(
                eng, batches, d, kind == "svd", 20 if args.quick else 200, reps)
        eng.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
