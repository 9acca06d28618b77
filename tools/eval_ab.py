"""A/B of one epoch's evaluation, host metrics against device metrics, on one GPU
(DESIGN 3.14, 8):

    timeout -k 10 600 python tools/eval_ab.py [--users 65536] [--items 100000] [--d 128] [--k 10]

A synthetic graph (synth_graph) whose every 10th train item is moved to the
truth; in one process, after one warm-up of each, the median of 5 wall-clock
times (a synchronize before the clock starts and before it stops) of

  (a) host:   Engine.score_topk + PairwiseModel._recommend's list building +
              ranking.evaluateCV over the five CV metrics;
  (b) device: Engine.evaluate at [k]

and the metric kernels' own HIP-event time (profile slot "metrics").  Checks
that both give the same scores (to 1e-9) and prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CV = ["pre", "recall", "ndcg", "map", "mrr"]


def split_truth(indptr, indices):
    """Every 10th train item (in nnz order) moves to the truth; users left
    without a truth item are not evaluated."""
    held = np.zeros(len(indices), bool)
    held[9::10] = True
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))

    def part(sel):
        ip = np.zeros(len(indptr), np.int64)
        np.cumsum(np.bincount(rows[sel], minlength=len(indptr) - 1), out=ip[1:])
        return ip, indices[sel].astype(np.int32)

    return part(~held), part(held)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=65536)
    ap.add_argument("--items", type=int, default=100000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--mean-degree", type=float, default=50.0)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from collaborativefilteringusingtensorflow_amd import ranking
    from collaborativefilteringusingtensorflow_amd._native import KERNELS
    from collaborativefilteringusingtensorflow_amd.engine import Engine, synth_graph
    nu, ni, d, k = args.users, args.items, args.d, args.k
    indptr, indices = synth_graph(nu, ni, args.mean_degree, 0.8, 7, n_threads=min(16, os.cpu_count() or 1))
    (tr_ip, tr_ix), (te_ip, te_ix) = split_truth(indptr, indices)
    users = np.nonzero(np.diff(te_ip))[0].astype(np.int32)
    eng = Engine("bpr", nu, ni, d, n_neg=1)
    eng.set_interactions(tr_ip, tr_ix)
    eng.init_params(0.0, 0.1, truncated=True, seed=1)
    eng.train_steps(4096, 20, return_loss=False)     # tables off their initial values
    eng.set_truth(te_ip, te_ix)
    eng.synchronize()
    yss_true = [set(te_ix[te_ip[u]:te_ip[u + 1]].tolist()) for u in users]

    def host():
        idx = eng.score_topk(users, k, exclude_train=True)
        yss_pred = [[int(x) for x in row if x >= 0] for row in idx]       # _model.py _recommend
        return ranking.evaluateCV(yss_true, yss_pred, CV, k)

    def device():
        sums = eng.evaluate(users, [k], exclude_train=True)
        return ranking.scores_from_sums(sums[0], len(users), CV, "cv")

    def timed(fn):
        eng.synchronize()
        t0 = time.perf_counter()
        out = fn()
        eng.synchronize()
        return time.perf_counter() - t0, out

    res = {}
    for name, fn in (("host", host), ("device", device)):
        fn()                                          # warm-up
        runs = [timed(fn) for _ in range(args.reps)]
        res[name] = {"median_s": statistics.median(t for t, _ in runs), "min_s": min(t for t, _ in runs),
                     "max_s": max(t for t, _ in runs), "scores": runs[-1][1]}
    for a, b in zip(res["host"]["scores"], res["device"]["scores"]):
        assert abs(a - b) <= 1e-9 * max(abs(a), 1e-300), (res["host"]["scores"], res["device"]["scores"])
    # the kernels' own time, in a run of its own (event pairs only around the slots read)
    eng.profile_reset()
    eng.set_option("profile_mask", (1 << KERNELS["metrics"]) | (1 << KERNELS["topk"]))
    eng.profile(True)
    for _ in range(args.reps):
        device()
    eng.profile(False)
    m_ms, m_n = eng.profile_read("metrics")
    t_ms, t_n = eng.profile_read("topk")
    print(json.dumps({"users": int(len(users)), "items": ni, "d": d, "k": k, "truth_nnz": int(len(te_ix)),
                      "host_eval_median_s": res["host"]["median_s"], "host_eval_range_s": [res["host"]["min_s"], res["host"]["max_s"]],
                      "device_eval_median_s": res["device"]["median_s"],
                      "device_eval_range_s": [res["device"]["min_s"], res["device"]["max_s"]],
                      "metrics_kernels_ms": m_ms / max(m_n, 1), "topk_kernel_ms": t_ms / max(t_n, 1),
                      "scores": dict(zip(CV, res["device"]["scores"]))}))
    eng.close()


if __name__ == "__main__":
    main()
