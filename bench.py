#!/usr/bin/env python
"""Benchmark of the pairwise-ranking training hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config cfg2]
                    [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps, writes its outputs when
--dump-outputs is given and prints the result line.  --full adds what else
the benchmark measures, each in a pass of its own after the timed region: the
per-kernel breakdown, SURVEY 8(d)'s batch, one drawn batch's row statistics
(apply roofline, dedup-aware bytes), cfg5's scoring pass, the cfg1 NDCG@10
check and the CPU baselines.

Metric (BASELINE.json): BPR triplets/sec (d=64) + achieved HBM GB/s.
Default workload = configs[1]: BPR-MF on a synthetic implicit-feedback graph,
1,000,000 users x 100,000 items, 50M interactions (degree 1+Poisson(49),
Zipf(0.8) item popularity), d=64, W=1, B=524,288 pairs per GPU per step
(SURVEY 8(d)'s B=65,536 is timed beside it: "batch_65536").
A step = one pass of the hot path over one batch, all on the GPU: device
sampler (epoch bijection + negative rejection) -> gather -> loss ->
gradient scatter -> duplicate-row sum -> Adagrad apply.  Inputs are resident
in HBM before the timed region.

N>1, one rank per GPU: users are sharded by contiguous id ranges (each rank
generates and samples its own shard), item rows are replicated; per step each
rank runs the local phase, the dense fp32 item gradient is exchanged over
RCCL (all-reduce + replicated item Adagrad, or reduce-scatter -> owner
Adagrad -> all-gather: --item-exchange) and every replica holds the identical
item table.  value = triplets of all ranks / max-over-ranks time ("weak").
`bench.py --gpus N` without a launcher starts its own N ranks
(torch.distributed.run as a child process, before anything touches the GPU)
and relays rank 0's line; every rank checks that the process group it formed
has exactly N ranks.

rank 0 prints ONE JSON line; diagnostics go to stderr.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
PROFILE_EVERY = 8
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec

CONFIGS = {
    # configs[1] of BASELINE.json
    # B = 2^19 pairs per GPU per step: the multi-GPU step all-reduces the dense
    # 25.6 MB item gradient once per step whatever B is, so B sets how many
    # triplets each exchanged byte carries; the 2^16 line of earlier
    # profiles is `--batch 65536`
    "cfg2": dict(model="bpr", n_users=1_000_000, n_items=100_000, mean_degree=50.0, zipf=0.8,
                 graph_seed=20261015, d=64, W=1, G=1, B=524288, reg=0.02, truncated=True,
                 desc="BPR-MF synthetic 1M users x 100K items, d=64"),
    # configs[2]: CML on the same graph
    "cfg3": dict(model="cml", n_users=1_000_000, n_items=100_000, mean_degree=50.0, zipf=0.8,
                 graph_seed=20261015, d=128, W=5, G=1, B=65536, reg=0.0, truncated=False,
                 margin=1.0, reg_cov=1.0, clip_norm=1.0,
                 desc="CML synthetic 1M users x 100K items, d=128, W=5"),
    # configs[3]: GBPR, 10M users x 1M items (N > 1: user-sharded with the
    # cross-shard group exchange + RCCL item-gradient all-reduce)
    "cfg4": dict(model="gbpr", n_users=10_000_000, n_items=1_000_000, mean_degree=20.0, zipf=0.8,
                 graph_seed=20261015, d=64, W=5, G=1, B=65536, reg=0.01, truncated=True,
                 rho=0.4, desc="GBPR synthetic 10M users x 1M items, d=64, W=5, G=1",
                 # N > 1: 2^20 pairs per GPU (the 260 MB item exchange
                 # is fixed per step, so at 65,536 pairs it is ~4x the compute
                 # step -- 1.35-1.5x at 8 GPUs -- and at 2^20 ~0.4x of it,
                 # 4.6x); the 65,536 line stays in the line as batch_65536
                 B_multi=1 << 20),
    # configs[4] shape, AMF phase 2 (adversarial) step
    "cfg5": dict(model="amf", n_users=1_000_000, n_items=100_000, mean_degree=50.0, zipf=0.8,
                 graph_seed=20261015, d=128, W=5, G=1, B=65536, reg=0.05, truncated=True,
                 reg_adv=1.0, desc="AMF synthetic 1M users x 100K items, d=128, W=5"),
}


def log(*a):
    print(*a, file=sys.stderr)
    sys.stderr.flush()


def gather_bytes_per_pair(d, W, G=0, bias=False):
    """algorithmic gather bytes per pair = (2+W)*4d + 4(2+W)
    (fp32 rows of U_u, V_i, V_j plus their int32 ids); + G group rows (GBPR)."""
    rows = 2 + W + G
    return rows * 4 * d + 4 * rows + (4 * (1 + W) if bias else 0)


def full_step_bytes_per_pair(d, W, G=0):
    """per row occurrence read var, read acc, write var, write acc
    (16d B) plus the ids: (2+W)*16d + 4(2+W)."""
    rows = 2 + W + G
    return rows * 16 * d + 4 * rows


def draw_bytes_per_pair(W, G, mean_row):
    """Algorithmic bytes of the device draw + count of one pair (prep_body):
    the pair record (8 B), its user's CSR extent (2 x 8 B) and row scan
    (4 B x row length, mean over pairs = sum(deg^2)/sum(deg)), the occurrence
    ids and ranks written (2 x 4 B per occurrence) and one count atomic per
    occurrence (4 B); GBPR adds the item's CSC extent + one user id per group
    member."""
    occ = 2 + W + G
    return 8 + 16 + 4 * mean_row + 12 * occ + ((16 + 4 * G) if G else 0)


def lib_digest():
    """First 12 hex digits of sha1(libcf_engine.so): the build the committed
    counters were collected on."""
    import hashlib
    from collaborativefilteringusingtensorflow_amd import _native
    try:
        with open(_native.LIB_PATH, "rb") as f:
            return hashlib.sha1(f.read()).hexdigest()[:12]
    except OSError:
        return "nolib"


def pmc_key(config, B, world, path_flags, exchange=None):
    """Key of profiles/pmc_traffic.json: workload, batch, ranks, the kernel
    path the step takes (cf_step_path flags) and the engine build -- counters
    collected on another build, path or world size do not apply to this line."""
    k = "%s_b%d_n%d_p%x_%s" % (config, B, world, path_flags, lib_digest())
    return k + ("_" + exchange if exchange else "")


def missing_orders(order_ms, n_in_region, steps, batches_per_epoch):
    """Sorted batches: a timed region of `steps` steps owes
    steps / batches_per_epoch epoch orders; the n_in_region computed inside
    it are on its clock, the rest are charged at order_ms each.  No order
    (sorted batches off at this batch size: order_ms 0) -> nothing owed."""
    if order_ms <= 0 or batches_per_epoch <= 0:
        return 0.0
    return max(0.0, steps / float(batches_per_epoch) - n_in_region)


def load_pmc(key):
    """HBM bytes per launch of the dominant kernel from the committed
    rocprofv3 FETCH_SIZE / WRITE_SIZE passes (tools/pmc_summary.py) for
    exactly this key, else None."""
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    try:
        with open(path) as f:
            rec = json.load(f)
        return rec.get(key, {}).get("step_hbm_bytes_per_launch")
    except Exception:
        return None


def ndcg_cfg1(device):
    """BASELINE configs[0] quality check: BPRMF on ml-100k fold 1 with the
    testbprmf.py settings (d=32, reg=.1, B=100, W=1, 50 epochs), fed the
    reference sampler's exact stream for np.random.seed(11) from the seeded
    tables of tests/golden/make_cfg1_golden.py, scored by the drop-in's own
    recommend + evaluateCV; the oracle's metrics for the same run are the
    committed fixture tests/golden/cfg1_oracle_metrics.json."""
    import scipy.sparse as sp
    from collaborativefilteringusingtensorflow_amd.bprmf import BPRMF
    from collaborativefilteringusingtensorflow_amd.init_util import seeded_table
    from collaborativefilteringusingtensorflow_amd.sampler_ranking import ExactSampler
    gdir = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gdir, "cfg1_oracle_metrics.json")) as f:
        ref = json.load(f)
    c = ref["config"]
    z = np.load(os.path.join(gdir, "ml100k_fold1.npz"))
    shape = (int(z["n_users"]), int(z["n_items"]))
    tra = sp.lil_matrix(sp.csr_matrix((np.ones(len(z["train_indices"]), np.float32),
                                       z["train_indices"], z["train_indptr"]), shape=shape))
    tst = sp.lil_matrix(sp.csr_matrix((np.ones(len(z["test_indices"]), np.float32),
                                       z["test_indices"], z["test_indptr"]), shape=shape))
    rng = np.random.RandomState(c["init_seed"])
    U0 = seeded_table(rng, (shape[0], c["d"]))
    V0 = seeded_table(rng, (shape[1], c["d"]))
    t0 = time.perf_counter()
    m = BPRMF(shape[0], shape[1], c["topN"], 'cv', c["metrics"], c["reg"], c["d"], c["B"],
              max_iter=c["epochs"], device=device, verbose=False)
    m.set_initial_tables(user=U0, item=V0)
    es = ExactSampler(tra, n_neg=c["W"], batch_size=c["B"], seed=c["sampler_seed"])
    got = m.train(1, tra, tst, es)
    es.close()
    m.close()
    dt = time.perf_counter() - t0
    g = dict(zip(c["metrics"], [float(x) for x in got]))
    return {"value": g["ndcg"], "ref_oracle": ref["metrics"]["ndcg"],
            "rel_diff": abs(g["ndcg"] - ref["metrics"]["ndcg"]) / ref["metrics"]["ndcg"],
            "metrics": g, "seconds": dt,
            "config": "cfg1: BPRMF ml-100k fold 1, d=32, reg=.1, B=100, W=1, 50 epochs, "
                      "reference sampler stream (seed 11), NDCG@10 vs the oracle on the same "
                      "batches and init"}


def cpu_threads():
    """Host threads for the all-cores CPU baseline: OMP_NUM_THREADS when set
    (the GPU box sets it to the job's CPU share), else every visible CPU."""
    try:
        n = int(os.environ.get("OMP_NUM_THREADS", "0"))
    except ValueError:
        n = 0
    return n if n > 0 else (os.cpu_count() or 1)


def cpu_baseline(cfg, indptr, indices, budget_s=12.0):
    """The C oracle (oracle/cf_oracle.c): the same sample + step work unit on
    the same graph, timed on this host on a bounded sample -- on all cores
    (oracle_train_mt, BPR / AMF) and on one core (oracle_train)."""
    from oracle.build_oracle import COracle
    from oracle import cf_oracle as O
    rng = np.random.RandomState(1)
    U = O.init_table(rng, (cfg["n_users"], cfg["d"]))
    V = O.init_table(rng, (cfg["n_items"], cfg["d"]))

    def make():
        return COracle(cfg["model"], U, V, W=cfg["W"], reg=cfg["reg"],
                       margin=cfg.get("margin", 1.0), reg_cov=cfg.get("reg_cov", 1.0),
                       clip_norm=cfg.get("clip_norm", 1.0), reg_adv=cfg.get("reg_adv", 1.0),
                       max_batch=cfg["B"])
    users = np.repeat(np.arange(len(indptr) - 1, dtype=np.int32), np.diff(indptr))
    coo = np.stack([users, indices], axis=1)
    del users
    B = cfg["B"]

    def timed(run):
        t0 = time.perf_counter()
        run(1, 12345)
        one = time.perf_counter() - t0
        n = max(1, int(budget_s / max(one, 1e-3)))
        t0 = time.perf_counter()
        run(n, 6789)
        return n, time.perf_counter() - t0

    c1 = make()
    n1, dt1 = timed(lambda n, seed: c1.train(indptr, indices, coo, B, n, seed))
    del c1
    single = {"value": n1 * B * cfg["W"] / dt1, "cores": 1,
              "sample": "%d steps, oracle_train, %.1f s" % (n1, dt1)}
    T = cpu_threads()
    if cfg["model"] in ("bpr", "amf") and T > 1:
        cm = make()
        nm, dtm = timed(lambda n, seed: cm.train_mt(indptr, indices, coo, B, n, seed, T))
        del cm
        return {"value": nm * B * cfg["W"] / dtm, "unit": "triplets/s", "cores": T, "kind": "port",
                "sample": "%d steps x %d pairs (W=%d) of %s: sample+forward+backward+dedup+Adagrad, "
                          "oracle/cf_oracle.c oracle_train_mt on %d threads, %.1f s"
                          % (nm, B, cfg["W"], cfg["desc"], T, dtm),
                "single_thread": single}
    return {"value": single["value"], "unit": "triplets/s", "cores": 1, "kind": "port",
            "sample": "%d steps x %d pairs (W=%d) of %s: sample+forward+backward+dedup+Adagrad, "
                      "oracle/cf_oracle.c single thread, %.1f s" % (n1, B, cfg["W"], cfg["desc"], dt1)}


def launcher_cmd(n_gpus, argv, port, python=None):
    """The torch.distributed.run command bench.py starts for itself when it
    is asked for N > 1 GPUs without a launcher (one rank per GPU, rendezvous
    on 127.0.0.1)."""
    return [python or sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
            "--nproc-per-node", str(int(n_gpus)), "--master-addr", "127.0.0.1",
            "--master-port", str(int(port)), os.path.abspath(__file__)] + list(argv)


def needs_launch(n_gpus, env=None):
    env = os.environ if env is None else env
    return int(n_gpus) > 1 and "WORLD_SIZE" not in env


def check_world(formed, n_gpus):
    """Every rank: the process group must hold exactly --gpus ranks."""
    if int(formed) != int(n_gpus):
        raise SystemExit("bench.py: --gpus %d but the process group has %d ranks" % (n_gpus, formed))


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch(n_gpus, argv):
    """Run the N ranks as a child process (never exec: this process has not
    touched the GPU and stays the parent), relay rank 0's JSON line to stdout
    and everything else to stderr; return the child's exit code."""
    env = dict(os.environ)
    env["CF_BENCH_LAUNCHED"] = "1"
    env.setdefault("MASTER_ADDR", "127.0.0.1")
    cmd = launcher_cmd(n_gpus, argv, free_port())
    log("bench.py: launching %d ranks: %s" % (n_gpus, " ".join(cmd)))
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, env=env, universal_newlines=True)
    line = None
    for raw in proc.stdout:
        t = raw.strip()
        if t.startswith("{") and '"metric"' in t:
            line = t
        elif t:
            log(t)
    rc = proc.wait()
    if line is not None:
        sys.stdout.write(line + "\n")
        sys.stdout.flush()
    return rc


def batch_stats(pairs, negs, groups, d, W):
    """Algorithmic bytes of one drawn batch, from its row multiplicities:
    * apply: every row seen >= 2 times reads its c gradient rows, reads and
      writes its row and accumulator: (c + 4) * 4d;
    * dedup-aware step: every UNIQUE row read + written with its accumulator
      (16d) + the int32 ids of every occurrence -- the bytes a step must move
      at the least (SURVEY 8(d)'s full-step figure without the duplicates)."""
    u = [pairs[:, 0]] + ([groups.reshape(-1)] if groups is not None else [])
    users = np.concatenate(u)
    items = np.concatenate([pairs[:, 1], negs.reshape(-1)])
    out = {}
    apply_b, uniq = 0.0, 0
    for ids in (users[users >= 0], items):
        _, c = np.unique(ids, return_counts=True)
        uniq += len(c)
        dup = c[c >= 2]
        apply_b += float(((dup + 4) * 4 * d).sum())
        out.setdefault("dup_rows", []).append(int(len(dup)))
    occ = len(users) + len(items)
    out["apply_bytes"] = apply_b
    out["dedup_step_bytes"] = float(uniq * 16 * d + 4 * occ)
    out["unique_rows"] = int(uniq)
    return out


DUMP_TABLE_BYTES = 10 << 20   # per table; at most six tables (GBPR) + the loss: under 64 MB
DUMP_SEED = 20261020


def dump_outputs(eng, model, out_dir):
    """What a caller of the timed path holds after its last step: every table
    the step updates (rows and Adagrad accumulators, float32) and the loss it
    accumulated since the start of the run (float64).  A table larger than
    DUMP_TABLE_BYTES is written as a fixed sample of its rows: the row ids
    depend only on the table's shape and DUMP_SEED."""
    os.makedirs(out_dir, exist_ok=True)
    names = ["user", "item", "acc_user", "acc_item"] + (["bias", "acc_bias"] if model == "gbpr" else [])
    for name in names:
        t = np.ascontiguousarray(eng.get_table(name), dtype=np.float32)
        n_rows = t.shape[0]
        keep = max(1, DUMP_TABLE_BYTES // max(1, t.nbytes // max(1, n_rows)))
        if keep < n_rows:
            rows = np.sort(np.random.RandomState(DUMP_SEED).choice(n_rows, size=keep, replace=False))
            t = t[rows]
        np.save(os.path.join(out_dir, name + ".npy"), t)
        del t
    np.save(os.path.join(out_dir, "loss.npy"), np.array([eng.take_loss()], dtype=np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--config", default="cfg2", choices=sorted(CONFIGS))
    ap.add_argument("--batch", type=int, default=0, help="pairs per GPU per step (0 = config)")
    ap.add_argument("--full", action="store_true",
                    help="also run the passes beside the headline figure: per-kernel breakdown, "
                         "--secondary-batch, batch statistics, cfg5's score pass, cfg1 NDCG@10, "
                         "CPU baselines (each can still be switched off by its own flag)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the tables and the loss the timed path left "
                         "after its last step to DIR/<name>.npy (float32 / float64; tables larger "
                         "than their share of 64 MB as a fixed seeded sample of rows)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--no-ndcg", action="store_true", help="skip the cfg1 NDCG@10 check")
    ap.add_argument("--dense-apply", type=int, default=int(os.environ.get("CF_DENSE_APPLY", "-1")),
                    help="cf_set_option dense_apply: 1 item-row apply on the slot / record path (default), 0 owner scan")
    ap.add_argument("--fused-variant", type=int, default=0,
                    help="cf_set_option fused_variant: 0 sequential fused scoring + top-k, 1 software-pipelined")
    ap.add_argument("--score-pass", action="store_true",
                    help="also time one full scoring + top-10 pass over this rank's users")
    ap.add_argument("--grad-path", type=int, default=0,
                    help="cf_set_option grad_path: 0 auto, 1 generic kernel, 2 phased kernel when eligible, 3 LDS-staged negatives when eligible")
    ap.add_argument("--prep-stream", type=int, default=0,
                    help="cf_set_option prep_stream: 0 in-order (default), 1 side stream")
    ap.add_argument("--pipeline", type=int, default=1,
                    help="cf_set_option pipeline: 1 apply(s)+draw(s+1) (default); 0 stepwise")
    ap.add_argument("--slot-max", type=int, default=0,
                    help="cf_set_option slot_max (0 = engine default)")
    ap.add_argument("--item-reduce", type=int, default=-1,
                    help="multi-rank item path (cf_set_option item_reduce 0/1/2; -1 = engine default)")
    ap.add_argument("--neg-check", type=int, default=-1,
                    help="negative rejection (cf_set_option neg_check: 1 Pos(u) set, 0 CSR row scan; -1 default)")
    ap.add_argument("--n-users", type=int, default=0, help="override the config's users (rehearsals)")
    ap.add_argument("--n-items", type=int, default=0, help="override the config's items (rehearsals)")
    ap.add_argument("--hot-replicas", type=int, default=0,
                    help="cf_set_option hot_replicas (0 = engine default)")
    ap.add_argument("--zipf", type=float, default=-1.0,
                    help="override the item popularity exponent (experiments; 0 = uniform)")
    ap.add_argument("--item-exchange", default=os.environ.get("CF_ITEM_EXCHANGE", "auto"),
                    choices=["auto", "allreduce", "rs_ag"],
                    help="multi-GPU item step: RCCL all-reduce + replicated Adagrad, or "
                         "reduce-scatter -> owner Adagrad -> all-gather; auto = rs_ag when "
                         "n_items * d >= 2^24 (DESIGN 5.1)")
    ap.add_argument("--secondary-batch", type=int, default=65536,
                    help="also time this batch size (SURVEY 8(d)'s B); 0 = off")
    ap.add_argument("--item-slots", type=int, default=-1,
                    help="cf_set_option item_slots (duplicated item rows: 1 records, 0 gradient rows; -1 default)")
    ap.add_argument("--bias-slots", type=int, default=-1,
                    help="cf_set_option bias_slots (GBPR item bias: 1 slots, 0 atomics; -1 default)")
    ap.add_argument("--pos-sort", type=int, default=-1,
                    help="cf_set_option pos_sort (gradient pairs in positive-item order; -1 default)")
    ap.add_argument("--item-pieces", type=int, default=-1,
                    help="the multi-rank item reduce + all-reduce in this many pieces of item rows "
                         "(-1 = auto: 4 at N > 1 with the all-reduce exchange, else 1)")
    ap.add_argument("--sorted-batches", type=int, default=-1,
                    help="cf_set_option sorted_batches (each batch's pairs in CSR order; -1 default)")
    ap.add_argument("--spec-neg", type=int, default=-1,
                    help="cf_set_option spec_neg (speculative negative counts in the pos_sort draw)")
    ap.add_argument("--pair-prefetch", type=int, default=-1,
                    help="cf_set_option pair_prefetch (the gradient launch fetches the next draw's pair records)")
    ap.add_argument("--deterministic", type=int, default=0,
                    help="cf_set_option deterministic (sort-based ranks, no float atomics)")
    ap.add_argument("--set-option", action="append", default=[], metavar="NAME=VALUE",
                    help="extra cf_set_option calls (A/B experiments), applied after the flags above")
    ap.add_argument("--amf-mode", default="reference", choices=["reference", "apr"],
                    help="AMF configs: cf_config.amf_mode (apr: Δ from the normalised embedding-loss "
                         "gradient, DESIGN 3.13; not the reference's computation)")
    ap.add_argument("--dry-run", action="store_true",
                    help="form the process group, check it, print a line; no GPU work (tests)")
    args = ap.parse_args()
    if needs_launch(args.gpus):
        sys.exit(launch(args.gpus, sys.argv[1:]))
    # the JSON line is the only thing on stdout: RCCL / HIP print banners
    # there from native code, so fd 1 points at stderr until the end
    json_out = os.fdopen(os.dup(1), "w")
    sys.stdout.flush()
    os.dup2(2, 1)
    cfg = dict(CONFIGS[args.config])
    if args.batch:
        cfg["B"] = args.batch
    if args.n_users or args.n_items:
        cfg["n_users"] = args.n_users or cfg["n_users"]
        cfg["n_items"] = args.n_items or cfg["n_items"]
        cfg["desc"] += " [rehearsal: %d users x %d items]" % (cfg["n_users"], cfg["n_items"])
    if args.zipf >= 0:
        cfg["zipf"] = args.zipf
        cfg["desc"] += " [experiment: zipf %.2f]" % args.zipf

    from collaborativefilteringusingtensorflow_amd.engine import (Engine, synth_degrees, synth_graph,
                                                                  synth_item_users)
    from collaborativefilteringusingtensorflow_amd.distributed import (make_gpu_group_exchange,
                                                                       make_gpu_sharded, shard_users)
    from collaborativefilteringusingtensorflow_amd._native import KERNELS
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    check_world(world, args.gpus)
    if not args.batch and world > 1 and "B_multi" in cfg:
        cfg["B"] = cfg["B_multi"]
        cfg["desc"] += " [%d pairs per GPU at N > 1, DESIGN 5.1]" % cfg["B"]
    if args.item_exchange == "auto":
        # the all-reduce hides under the fused user apply + draw at
        # cfg2/3/5; item-range ownership pays off where the dense item Adagrad
        # itself is large (cfg4: 1M x 64 floats)
        args.item_exchange = "rs_ag" if cfg["n_items"] * cfg["d"] >= (1 << 24) else "allreduce"
    dist = None
    torch = None
    # CF_DIST_BACKEND=gloo + CF_SHARE_DEVICE=1 rehearse the N>1 path with all
    # ranks on device 0 of a one-GPU box (RCCL refuses duplicate devices)
    backend = os.environ.get("CF_DIST_BACKEND", "nccl")
    if os.environ.get("CF_SHARE_DEVICE") == "1":
        local_rank = 0
    # CF_BENCH_SHARDED=1 at N=1: the multi-GPU code path (dense item gradient,
    # all-reduce over a one-rank group) -- the local cost of a sharded step
    sharded = world > 1 or os.environ.get("CF_BENCH_SHARDED") == "1"
    if sharded and world == 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29561")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        cfg["desc"] += " [sharded code path, 1 rank]"
    if args.dry_run:
        backend = os.environ.get("CF_DIST_BACKEND", "gloo")
        if world == 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", str(free_port()))
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
    if sharded or args.dry_run:
        import torch  # noqa: F811
        import torch.distributed as dist  # noqa: F811
        if args.dry_run:
            dist.init_process_group(backend)
        else:
            torch.cuda.set_device(local_rank)
            if backend == "nccl":
                dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
            else:
                dist.init_process_group(backend)
        check_world(dist.get_world_size(), args.gpus)
    if args.dry_run:
        if rank == 0:
            json_out.write(json.dumps({"metric": "dry-run", "value": 0, "n_gpus": dist.get_world_size(),
                                       "backend": dist.get_backend(),
                                       "launched": os.environ.get("CF_BENCH_LAUNCHED") == "1"}) + "\n")
            json_out.flush()
        dist.barrier()
        dist.destroy_process_group()
        return

    # ---- inputs: this rank's user shard of the synthetic graph ----------------
    nu_all, ni, d, W, B = cfg["n_users"], cfg["n_items"], cfg["d"], cfg["W"], cfg["B"]
    t0 = time.perf_counter()
    u0, u1 = shard_users(synth_degrees(nu_all, cfg["mean_degree"], cfg["graph_seed"]), world, rank)
    indptr, indices = synth_graph(nu_all, ni, cfg["mean_degree"], cfg["zipf"], cfg["graph_seed"],
                                  u_begin=u0, u_end=u1, n_threads=min(16, os.cpu_count() or 1))
    log("rank %d: users [%d,%d) nnz %d generated in %.1fs" % (rank, u0, u1, len(indices),
                                                             time.perf_counter() - t0))
    kw = dict(reg=cfg["reg"])
    for k in ("margin", "reg_cov", "clip_norm", "reg_adv", "rho"):
        if k in cfg:
            kw[k] = cfg[k]
    if args.amf_mode != "reference":
        if cfg["model"] != "amf":
            raise SystemExit("--amf-mode applies to AMF configs (cfg5)")
        kw["amf_mode"] = args.amf_mode
        cfg["desc"] += " [amf_mode %s, epsilon 0.5]" % args.amf_mode
    eng = Engine(cfg["model"], u1 - u0, ni, d, n_neg=W, gsize=cfg["G"], device=local_rank,
                 dense_item_apply=sharded, seed=1000 + rank, **kw)
    eng.set_option("grad_path", args.grad_path)
    if args.fused_variant != 0:   # (the engine's default is 0)
        eng.set_option("fused_variant", args.fused_variant)
    eng.set_option("prep_stream", args.prep_stream)
    eng.set_option("pipeline", args.pipeline)
    if args.hot_replicas:
        eng.set_option("hot_replicas", args.hot_replicas)
    if args.neg_check >= 0:
        eng.set_option("neg_check", args.neg_check)
    if args.item_reduce >= 0:
        eng.set_option("item_reduce", args.item_reduce)
    if args.bias_slots >= 0:
        eng.set_option("bias_slots", args.bias_slots)
    if args.item_slots >= 0:
        eng.set_option("item_slots", args.item_slots)
    if args.dense_apply >= 0:
        eng.set_option("dense_apply", args.dense_apply)
    if args.pos_sort >= 0:
        eng.set_option("pos_sort", args.pos_sort)
    if args.pair_prefetch >= 0:
        eng.set_option("pair_prefetch", args.pair_prefetch)
    if args.spec_neg >= 0:
        eng.set_option("spec_neg", args.spec_neg)
    if args.sorted_batches >= 0:
        eng.set_option("sorted_batches", args.sorted_batches)
    if args.deterministic:
        eng.set_option("deterministic", 1)
    if args.slot_max:
        eng.set_option("slot_max", args.slot_max)
    for kv in args.set_option:
        name, val = kv.split("=", 1)
        eng.set_option(name, int(val))
        cfg["desc"] += " [%s=%s]" % (name, val)
    eng.set_interactions(indptr, indices)
    eng.init_params(0.0, 0.1, truncated=cfg["truncated"], seed=1)  # same V on every rank
    if cfg["model"] == "amf":
        eng.begin_phase(1)

    if sharded and cfg["model"] == "gbpr":
        # group members come from every shard: the global item -> user CSR
        # (built natively, cf_synth_item_users) feeds the group draw, the
        # exchange fetches / returns remote rows
        degs = synth_degrees(nu_all, cfg["mean_degree"], cfg["graph_seed"])
        bounds = [shard_users(degs, world, r)[0] for r in range(world)] + [nu_all]
        t1 = time.perf_counter()
        item_csr = synth_item_users(nu_all, ni, cfg["mean_degree"], cfg["zipf"], cfg["graph_seed"],
                                    n_threads=min(16, os.cpu_count() or 1))
        log("rank %d: item -> user CSR built in %.1fs" % (rank, time.perf_counter() - t1))
        step, _items = make_gpu_group_exchange(eng, world, rank, bounds, None, None, ni, d, B,
                                               torch.device("cuda", local_rank),
                                               exchange=args.item_exchange, item_csr=item_csr)
        del item_csr
    elif sharded:
        pieces = args.item_pieces
        if pieces < 0:   # piece q's all-reduce runs while piece q+1 is reduced
            pieces = 4 if (world > 1 and args.item_exchange == "allreduce" and cfg["model"] != "gbpr") else 1
        step, _items = make_gpu_sharded(eng, ni, d, cfg["model"] == "gbpr",
                                        torch.device("cuda", local_rank), exchange=args.item_exchange,
                                        pieces=pieces)
        dist_pieces = pieces
    if sharded:
        def run(k, b=B):
            for _ in range(k):
                step(b)

        def sync():
            torch.cuda.synchronize()
            dist.barrier()
    else:
        def run(k, b=B):
            eng.train_steps(b, k, return_loss=False)

        def sync():
            eng.synchronize()

    run(args.warmup)
    sync()
    # timed region: HIP events around the dominant kernel only (an event pair
    # around every launch would add ~20 us per step to the loop)
    eng.profile_reset()
    # pipeline 2: the gradient launch of step s also carries the draw + count
    # of step s+1 ("grad_prep"); otherwise (pipeline 1, the default) the
    # gradient launch is "step" and the draw rides in the apply launch
    dom = "grad_prep" if (args.pipeline == 2 and not sharded) else "step"
    # the split GBPR exchange step runs its gradient in two launches (pairs
    # with local group members, then the rest): both are timed, summed per step
    split_grad = sharded and cfg["model"] == "gbpr"
    # + the sorted batches' epoch orders computed inside the region (always
    # timed, so their count is exact; see the charge below)
    eng.set_option("profile_mask", (1 << KERNELS[dom]) | ((1 << KERNELS["step_remote"]) if split_grad else 0)
                   | (1 << KERNELS["epoch_order"]))
    # every PROFILE_EVERY-th launch is timed: an event pair on every launch
    # costs the loop ~6 us/step (cfg2), sampled launches ~1/PROFILE_EVERY of it
    eng.set_option("profile_every", PROFILE_EVERY)
    eng.profile(not args.no_profile)
    sync()
    t0 = time.perf_counter()
    run(args.steps)
    sync()
    elapsed = time.perf_counter() - t0
    eng.profile(False)
    eng.set_option("profile_every", 1)
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda:%d" % local_rank)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    step_ms, step_n = eng.profile_read(dom)
    _, eo_in = eng.profile_read("epoch_order")
    if split_grad:
        rem_ms, _ = eng.profile_read("step_remote")
        step_ms += rem_ms

    if args.dump_outputs:   # before any later pass steps the tables again
        if sharded and hasattr(step, "sync_state"):
            step.sync_state()   # item-range ownership: gather the owners' accumulator rows
        if rank == 0:
            dump_outputs(eng, cfg["model"], args.dump_outputs)

    # per-kernel breakdown: a separate, untimed pass with every launch timed
    kernels = {}
    if args.full and not args.no_profile:
        nb = min(args.steps, 50)
        eng.profile_reset()
        eng.set_option("profile_mask", 0xFFFFFFFF)
        eng.profile(True)
        run(nb)
        sync()
        eng.profile(False)
        for kname in ("sample", "slot", "step", "step_remote", "grad_prep", "apply", "apply_prep", "apply_slot",
                      "item_reduce", "apply_dense", "clip", "psort"):
            ms, n = eng.profile_read(kname)
            if n:
                kernels[kname] = {"launches": n, "avg_us": 1e3 * ms / n, "total_ms": ms}
        kernels["note"] = "separate %d-step pass with every launch timed (not the timed region)" % nb
    loss = eng.take_loss()
    log("rank %d: loss accumulated %.4e" % (rank, loss))

    # sorted batches: each epoch's pair order -- a
    # counting sort of the pairs by batch (cf_epoch.hip, round 6) -- is computed once per epoch,
    # ahead, on a low-priority stream.  The orders computed inside the timed
    # region (eo_in) are already on its clock; a region shorter than an epoch
    # may meet fewer than its share (steps / batches per epoch).  The missing
    # share is charged at the order's standalone time (measured here on a
    # forced, uncached epoch): `value` and `ms_per_step` below include it
    def epoch_order_ms(b):
        """Standalone time of one epoch's order at batch b (0 when sorted
        batches are off there): a forced, uncached epoch, then the sampler
        state is restored."""
        ms_ = 0.0
        try:
            st0 = eng.sampler_state()
            eng.profile_reset()
            eng.set_option("profile_mask", 1 << KERNELS["epoch_order"])
            eng.profile(True)
            eng.set_sampler_state(st0[0] + 7, 0)
            run(1, b)
            sync()
            eng.profile(False)
            ms, n = eng.profile_read("epoch_order")
            ms_ = ms / n if n else 0.0
            eng.set_sampler_state(*st0)
            eng.take_loss()
        except Exception as ex:  # diagnostics only
            log("epoch order timing failed: %r" % (ex,))
        if world > 1:
            t = torch.tensor([ms_], dtype=torch.float64, device="cuda:%d" % local_rank)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            ms_ = float(t.item())
        return ms_

    def order_charge(ms_, n_in, steps, per_ep):
        """Orders (of the region's steps / per_ep share) not on the clock."""
        miss = missing_orders(ms_, n_in, steps, per_ep)
        if world > 1:
            t = torch.tensor([miss], dtype=torch.float64, device="cuda:%d" % local_rank)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            miss = float(t.item())
        return miss

    per_epoch = max(1, len(indices) // B)
    eo_ms = epoch_order_ms(B)
    elapsed_timed = elapsed
    eo_missing = order_charge(eo_ms, eo_in, args.steps, per_epoch)
    elapsed = elapsed + 1e-3 * eo_ms * eo_missing

    # SURVEY 8(d)'s batch (65,536 pairs per GPU) on the same engine and graph
    secondary = None
    B2 = args.secondary_batch
    if args.full and B2 and B2 != B and B2 <= len(indices):
        run(max(2, args.warmup // 2), B2)
        sync()
        eng.profile_reset()
        eng.set_option("profile_mask", 1 << KERNELS["epoch_order"])
        eng.profile(True)
        t0 = time.perf_counter()
        run(args.steps, B2)
        sync()
        el2 = time.perf_counter() - t0
        eng.profile(False)
        _, eo2_in = eng.profile_read("epoch_order")
        per_epoch2 = max(1, len(indices) // B2)
        eo2_ms = epoch_order_ms(B2)
        eo2_missing = order_charge(eo2_ms, eo2_in, args.steps, per_epoch2)
        el2 += 1e-3 * eo2_ms * eo2_missing
        if world > 1:
            t = torch.tensor([el2], dtype=torch.float64, device="cuda:%d" % local_rank)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el2 = float(t.item())
        secondary = {"batch_pairs_per_gpu": B2, "steps": args.steps,
                     "value": B2 * W * args.steps * world / el2, "unit": "triplets/s",
                     "ms_per_step": 1e3 * el2 / args.steps,
                     "epoch_order": {"ms_per_epoch": eo2_ms, "batches_per_epoch": per_epoch2,
                                     "in_timed_region": eo2_in, "charged": eo2_missing}}
    # one drawn batch's row multiplicities -> the apply + draw launch's and a
    # dedup-aware step's algorithmic bytes (batch_stats)
    st = None
    if args.full:
        try:
            bp, bn, bg = eng.sample(B)
            st = batch_stats(bp, bn, bg, d, W)
        except Exception as ex:  # diagnostics only
            log("batch stats failed: %r" % (ex,))

    trip_per_step = B * W
    total_trip = trip_per_step * args.steps * world
    value = total_trip / elapsed
    step_avg_s = (1e-3 * step_ms / step_n) if step_n else float("nan")
    Gm = cfg["G"] if cfg["model"] == "gbpr" else 0
    gb = gather_bytes_per_pair(d, W, Gm, bias=cfg["model"] == "gbpr") * B
    deg = np.diff(np.asarray(indptr, dtype=np.int64)).astype(np.float64)
    mean_row = float((deg * deg).sum() / max(deg.sum(), 1.0))
    db = draw_bytes_per_pair(W, Gm, mean_row) * B if dom == "grad_prep" else 0.0
    achieved = (gb + db) / step_avg_s / 1e9 if step_avg_s == step_avg_s and step_avg_s > 0 else None
    path_flags, path = eng.step_path(B)
    key = pmc_key(args.config, B, world, path_flags, args.item_exchange if sharded else None)
    traffic = load_pmc(key)
    if dom == "grad_prep":
        kdesc = ("grad_fast_kernel: gather + loss + grads + singleton-row Adagrad of step s, "
                 "fused with the device draw + count of step s+1")
        bdef = ("SURVEY 8(d) gather bytes B*((2+W)*4d + 4(2+W)) of step s + draw bytes of step s+1 "
                "B*(8 + 16 + 4*E[row] + 12(2+W)), E[row] = sum(deg^2)/nnz = %.1f" % mean_row)
    else:
        kdesc = "grad_kernel (gather + loss + grads + singleton-row Adagrad)"
        bdef = "SURVEY 8(d) gather bytes: B*((2+W)*4d + 4(2+W))"
    roofline = {"kernel": kdesc,
                "bound": "hbm",
                "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                "frac": (achieved / HBM_PEAK_GBPS) if achieved else None,
                "traffic": traffic,
                "pmc_key": key,
                "step_path": path,
                "bytes_per_launch": gb + db,
                "gather_bytes_per_launch": gb,
                "gather_only_GBps": gb / step_avg_s / 1e9 if achieved else None,
                "bytes_def": bdef,
                "avg_launch_us": step_avg_s * 1e6 if step_n else None,
                "timed_launches": step_n,
                "timed_every": PROFILE_EVERY if not args.no_profile else None}
    full_b = full_step_bytes_per_pair(d, W) * B * args.steps * world
    roofline_apply = None
    ap_k = kernels.get("apply_prep")
    if st is not None and ap_k:
        dbp = draw_bytes_per_pair(W, Gm, mean_row) * B
        ab = st["apply_bytes"] + dbp
        roofline_apply = {
            "kernel": "apply_prep_kernel: Adagrad of the duplicated rows of step s (slot sums) "
                      "+ device draw + count of step s+1",
            "bound": "hbm", "achieved": ab / (1e-6 * ap_k["avg_us"]) / 1e9, "peak": HBM_PEAK_GBPS,
            "unit": "GB/s", "frac": ab / (1e-6 * ap_k["avg_us"]) / 1e9 / HBM_PEAK_GBPS,
            "bytes_per_launch": ab, "apply_bytes": st["apply_bytes"], "draw_bytes": dbp,
            "bytes_def": "sum over rows seen c >= 2 times in the batch of (c + 4) * 4d (c gradient "
                         "rows read, row + accumulator read and written) + the draw bytes "
                         "B*(8 + 16 + 4*E[row] + 12(2+W)), E[row] = %.1f" % mean_row,
            "avg_launch_us": ap_k["avg_us"], "dup_rows_user_item": st["dup_rows"]}
    dedup = None
    if st is not None:
        dedup = {"bytes_per_step": st["dedup_step_bytes"], "unique_rows": st["unique_rows"],
                 "GBps": st["dedup_step_bytes"] * args.steps * world / elapsed / 1e9,
                 "def": "unique rows touched x 16d (row + accumulator read and written) + 4 B per "
                        "occurrence id, one drawn batch"}
    dist_info = {}
    if sharded:
        dist_info = {"world_size_formed": dist.get_world_size(), "backend": dist.get_backend(),
                     "item_exchange": args.item_exchange,
                     "item_pieces": locals().get("dist_pieces", 1),
                     "launched_by_bench": os.environ.get("CF_BENCH_LAUNCHED") == "1"}
    out = {
        "metric": "BPR triplets/sec/GPU (d=64) + achieved HBM GB/s; NDCG@10 vs ref",
        "value": value, "unit": "triplets/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps,
        "ms_per_step_timed": 1e3 * elapsed_timed / args.steps,
        "epoch_order": {"ms_per_epoch": eo_ms, "batches_per_epoch": per_epoch,
                        "in_timed_region": eo_in, "charged": eo_missing,
                        "charged_ms_per_step": eo_ms * eo_missing / args.steps,
                        "def": "sorted batches: one epoch's pair order (a counting sort of the pairs by batch, "
                               "cf_epoch.hip) is computed per epoch; those inside the timed region are on its "
                               "clock, the rest of the region's share (steps / batches_per_epoch) is charged "
                               "at the standalone time (DESIGN 3.1)"},
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic (seeded, generated in-repo), random-init tables",
        "config": {"workload": cfg["desc"], "model": cfg["model"], "n_users": nu_all,
                   "n_items": ni, "nnz_rank0": int(len(indices)), "d": d, "W": W,
                   "batch_pairs_per_gpu": B, "global_batch": B * world,
                   "parallelism": ("dp%d user-sharded, RCCL item-grad %s" % (
                                       world, "all-reduce" if args.item_exchange == "allreduce"
                                       else "reduce-scatter + owner Adagrad + all-gather")
                                   + (" + group-member all-to-all" if cfg["model"] == "gbpr" else ""))
                   if world > 1 else "single GPU"},
        "per_gpu_value": value / world,
        "full_step_algorithmic_GBps": full_b / elapsed / 1e9,
        "roofline": roofline,
        "roofline_apply_prep": roofline_apply,
        "dedup_step": dedup,
        "batch_65536": secondary,
        "kernels": kernels,
    }
    out["config"].update(dist_info)
    if args.score_pass or (args.full and args.config == "cfg5"):
        users = np.arange(u1 - u0, dtype=np.int32)
        eng.score_topk(users[:1024], 10)          # warm-up
        sync()
        eng.profile_reset()
        eng.set_option("profile_mask", 1 << KERNELS["topk"])
        eng.profile(True)
        t0 = time.perf_counter()
        eng.score_topk(users, 10, exclude_train=True)
        sync()
        ts = time.perf_counter() - t0
        eng.profile(False)
        tk_ms, tk_n = eng.profile_read("topk")
        if world > 1:
            t = torch.tensor([ts], dtype=torch.float64, device="cuda:%d" % local_rank)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            ts = float(t.item())
        flop = 2.0 * nu_all * ni * d
        out["score_pass"] = {"users": nu_all, "items": ni, "d": d, "k": 10, "seconds": ts,
                             "TFLOPs": flop / ts / 1e12,
                             "frac_fp32_mfma_peak": flop / ts / 1e12 / (157.3 * world),
                             "kernel": ("fused_topk_pipe_kernel" if args.fused_variant == 1 and cfg["model"] != "cml"
                                        else "fused_topk_kernel") +
                                       " (v_mfma_f32_32x32x2_f32 + streaming top-k)",
                             "kernel_ms_hip_events": tk_ms if tk_n else None,
                             "kernel_TFLOPs": (2.0 * (u1 - u0) * ni * d / (1e-3 * tk_ms) / 1e12)
                             if tk_n and tk_ms > 0 else None}
    if args.full and rank == 0 and world == 1 and not args.no_ndcg:
        try:
            out["ndcg10_vs_ref"] = ndcg_cfg1(local_rank)
        except Exception as ex:  # the bench line must still print
            log("cfg1 ndcg run failed: %r" % (ex,))
            out["ndcg10_vs_ref"] = None
    if args.full and rank == 0 and not args.no_cpu_baseline:
        # at N > 1 too (verdict r03): rank 0 times the same bounded sample on
        # its host cores after the timed region, on its own user shard, while
        # the other ranks wait at the closing barrier
        try:
            out["cpu_baseline"] = cpu_baseline(cfg, indptr, indices)
            if world > 1:
                out["cpu_baseline"]["note"] = ("rank 0's host, its user shard's interactions, after the timed "
                                               "region; the GPU value is the %d-GPU aggregate" % world)
        except Exception as ex:  # the bench line must still print
            log("cpu baseline failed: %r" % (ex,))
            out["cpu_baseline"] = None
    eng.close()
    if rank == 0:
        json_out.write(json.dumps(out) + "\n")
        json_out.flush()
    if sharded:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
