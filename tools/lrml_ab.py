"""LRML step and recommend figures on one GPU:

    timeout -k 10 600 python tools/lrml_ab.py [--out FILE] [--quick]

Measured, each after a warm-up of the same shape, as the median of --reps
windows of a host clock around calls that end in a device synchronise
(take_loss / score_topk sync):

  step, driver shape   ml-100k fold 1 (tests/golden/ml100k_fold1.npz), d = 100,
                       M = 20, B = 100, batches of the exact sampler;
  step, large batch    synth_graph(1M users, 100K items), d = 64, M = 20,
                       B = 65,536: positives drawn from the graph, negatives
                       uniform;
  recommend            both predict modes: every ml-100k user at d = 100,
                       M = 20, and 4,096 users x 100K items at d = 64, M = 20,
                       k = 10, in (user, item) pairs/s and exponentials/s.

These are whole-call times (host range check, the id copy, every launch), not
kernel times: the kernels' own times come from a separate
``rocprofv3 --kernel-trace --stats -- python tools/lrml_ab.py --quick`` run.
Beside each figure the tool prints what the algorithm needs, computed from the
shapes: the step's gather + scatter bytes (4 gathered rows and 4 float-atomic
rows per batch row, 3 rows read and 3 written per distinct table row in the
apply) and the scoring pass's exponentials (reference: M d per pair; train: M
per pair), so that a figure can be held against HBM bandwidth and against the
transcendental issue rate.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def step_bytes(batches, d):
    """Mean bytes one step must move: per batch row 4 gathered + 4 scattered
    rows, per distinct user / item row 3 read + 3 written in the apply."""
    tot = 0.0
    for pos, neg in batches:
        B = len(pos)
        uniq = len(np.unique(np.r_[pos[:, 0], neg[:, 0]])) + len(np.unique(np.r_[pos[:, 1], neg[:, 1]]))
        tot += 4.0 * d * (8 * B + 6 * uniq)
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


def time_recommend(eng, users, k, mode, reps):
    eng.score_topk(users, k, exclude_train=True, predict_mode=mode)
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        eng.score_topk(users, k, exclude_train=True, predict_mode=mode)
        out.append(time.perf_counter() - t0)
    return out


def summary(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="one short window per figure (profiler runs)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import scipy.sparse as sp
    from collaborativefilteringusingtensorflow_amd import _native as N
    from collaborativefilteringusingtensorflow_amd.engine import synth_graph
    from collaborativefilteringusingtensorflow_amd.lrml import LRMLEngine
    from collaborativefilteringusingtensorflow_amd.sampler_lrml_ranking import ExactSampler
    if N.device_count() < 1:
        raise SystemExit("lrml_ab: no HIP device visible")
    reps = 1 if args.quick else args.reps
    res = {}

    # -- the driver's shape ----------------------------------------------------------
    z = np.load(os.path.join(ROOT, "tests", "golden", "ml100k_fold1.npz"))
    ip, ix = z["train_indptr"], z["train_indices"]
    tra = sp.csr_matrix((np.ones(len(ix), np.float32), ix, ip), shape=(943, 1682))
    smp = ExactSampler(tra, batch_size=100, seed=0)
    batches = [smp.next_batch() for _ in range(256)]
    smp.close()
    d, M = 100, 20
    eng = LRMLEngine(943, 1682, d, M)
    eng.init_params(0.0, 0.01, seed=1)
    eng.set_interactions(ip, ix)
    ts = time_steps(eng, batches, 200 if args.quick else 4000, reps)
    nbytes = step_bytes(batches, d)
    res["step_ml100k_d100_M20_B100"] = {"ms_per_step": {k: 1e3 * v for k, v in summary(ts).items()},
                                        "bytes_per_step": nbytes,
                                        "bytes_per_s": nbytes / statistics.median(ts)}
    users = np.arange(943, dtype=np.int32)
    for mode in ("reference", "train"):
        rs = time_recommend(eng, users, 10, mode, reps)
        pairs = 943 * 1682
        exps = pairs * (M * d if mode == "reference" else M)
        res["recommend_ml100k_d100_M20_" + mode] = {"s": summary(rs), "pairs_per_s": pairs / statistics.median(rs),
                                                    "exps_per_s": exps / statistics.median(rs)}
    eng.close()

    # -- B = 65,536 on the 1M x 100K graph, d = 64 -------------------------------------
    nu, ni, d, M, B = 1000000, 100000, 64, 20, 65536
    gp, gx = synth_graph(nu, ni, 50.0, 0.8, 7, n_threads=min(16, os.cpu_count() or 1))
    rows = np.repeat(np.arange(nu, dtype=np.int32), np.diff(gp))
    rng = np.random.RandomState(3)
    batches = []
    for _ in range(8):
        sel = rng.randint(0, len(gx), B)
        batches.append((np.stack([rows[sel], gx[sel]], 1).astype(np.int32),
                        np.stack([rng.randint(0, nu, B), rng.randint(0, ni, B)], 1).astype(np.int32)))
    eng = LRMLEngine(nu, ni, d, M)
    eng.init_params(0.0, 0.01, seed=1)
    eng.set_interactions(gp, gx)
    ts = time_steps(eng, batches, 20 if args.quick else 200, reps)
    nbytes = step_bytes(batches, d)
    res["step_synth1M_100K_d64_M20_B65536"] = {"ms_per_step": {k: 1e3 * v for k, v in summary(ts).items()},
                                               "bytes_per_step": nbytes,
                                               "bytes_per_s": nbytes / statistics.median(ts),
                                               "rows_per_s": B / statistics.median(ts)}
    users = np.arange(0, nu, nu // 4096, dtype=np.int32)[:4096]
    for mode in ("reference", "train"):
        rs = time_recommend(eng, users, 10, mode, reps)
        pairs = len(users) * ni
        exps = pairs * (M * d if mode == "reference" else M)
        res["recommend_4096x100K_d64_M20_" + mode] = {"s": summary(rs), "pairs_per_s": pairs / statistics.median(rs),
                                                      "exps_per_s": exps / statistics.median(rs)}
    eng.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
