"""distributed.reduce_eval over gloo on CPU (world 2 and 3): per-shard metric
sums of disjoint user shards all-reduce to the whole set's sums, the user
counts to the total.

Bound: each shard's sum (numpy, over its rows) and the all-reduce's adds are
fp64 sums of the same n values in some order, so the result is within
n * 2^-52 * sum|x| of math.fsum over all rows (the sum bound of
tests/test_gpu_eval.py with no per-user tolerance: the rows are given)."""
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CUT = 3


def _rows(n):
    rng = np.random.RandomState(77)
    return rng.rand(n, N_CUT, 7) * np.array([1.0, 1e-3, 1e3, 1.0, 1.0, 1.0, 0.5])


def _cuts(n, world):
    return [n * r // world for r in range(world + 1)]


def _worker(rank, world, port, n, q):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from collaborativefilteringusingtensorflow_amd.distributed import reduce_eval
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    cuts = _cuts(n, world)
    mine = _rows(n)[cuts[rank]:cuts[rank + 1]]
    sums, total = reduce_eval(mine.sum(axis=0), mine.shape[0])
    q.put((rank, sums, total))
    dist.barrier()
    dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("world", [2, 3])
def test_reduce_eval_equals_whole_set(world):
    n = 1001
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=180) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    rows = _rows(n)
    for rank, sums, total in res:
        assert total == n and isinstance(total, int)
        assert sums.shape == (N_CUT, 7) and sums.dtype == np.float64
        for c in range(N_CUT):
            for m in range(7):
                x = rows[:, c, m]
                want = math.fsum(x.tolist())
                bound = n * 2.0 ** -52 * math.fsum(np.abs(x).tolist())
                assert abs(sums[c, m] - want) <= bound, (rank, c, m, sums[c, m], want, bound)
    for rank, sums, _ in res[1:]:
        assert np.array_equal(sums, res[0][1])   # every rank holds the same global sums
