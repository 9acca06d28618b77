"""Shared inputs of the LRML tests (tests/test_lrml_model.py,
tests/test_gpu_lrml.py): seeded initial tables, the reference's captured
batch stream, the edge-shape batches, and the float64 / float32 model runs.

INIT_SEEDS: the init seed of every parity shape, picked on the CPU so that the
float64 model's min |h| over all rows of the ten golden-stream steps exceeds
1e-4 (the tests assert it): no row's hinge can take the other branch in fp32.
"""
import os

import numpy as np

import lrml_model as LM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NU, NI = 943, 1682
HP = dict(margin=0.2, clip_norm=1.0, lr=0.01)
H_MIN = 1e-4

# (d, M, stddev) -> init seed (the first that pick_seed below accepts)
INIT_SEEDS = {(50, 20, 0.01): 1, (50, 20, 0.3): 2, (100, 20, 0.01): 1, (100, 20, 0.3): 1,
              (20, 1, 0.01): 1, (20, 1, 0.3): 1, (128, 64, 0.01): 1, (128, 64, 0.3): 1}
# edge shapes (50 x 80 tables, stddev 0.3, six steps): d -> M, (B, d) -> seed,
# chosen the same way (min |h| > 2 * H_MIN in float64)
EDGE_NU, EDGE_NI = 50, 80
EDGE_M = {1: 5, 17: 33, 33: 20, 128: 64}
EDGE_SEEDS = {(1, 1): 1, (1, 17): 1, (1, 33): 1, (1, 128): 1, (63, 1): 1, (63, 17): 1, (63, 33): 2,
              (63, 128): 2, (257, 1): 1, (257, 17): 1, (257, 33): 2, (257, 128): 4}


def stream():
    with np.load(os.path.join(GOLDEN, "lrml_stream.npz")) as z:
        return z["pos"], z["neg"]


def init_tables(seed, nu, ni, d, M, stddev):
    """float32 U, V, Key, Mem ~ N(0, stddev^2), untruncated (lrml.py:30-41)."""
    rng = np.random.RandomState(seed)
    return [(rng.randn(*s) * stddev).astype(np.float32) for s in ((nu, d), (ni, d), (d, M), (M, d))]


def run_model(tabs, batches, dtype, hp=HP):
    """The model from float32 tables cast to dtype.  Returns the tables
    dict, the per-step losses and the per-step h vectors."""
    U, V, Key, Mem = (t.astype(dtype) for t in tabs)
    AU, AV = np.full_like(U, 0.1), np.full_like(V, 0.1)
    losses, hs = [], []
    for pos, neg in batches:
        lo, h = LM.step(U, V, AU, AV, Key, Mem, pos, neg, **hp)
        losses.append(lo)
        hs.append(h)
    return dict(user=U, item=V, acc_user=AU, acc_item=AV, key=Key, memory=Mem), losses, hs


def min_abs_h(hs):
    return min(float(np.abs(h).min()) for h in hs)


def pick_seed(d, M, stddev, n_steps=10, start=1, tries=200):
    """The first init seed whose float64 run keeps min |h| > 2 * H_MIN."""
    pos, neg = stream()
    batches = list(zip(pos[:n_steps], neg[:n_steps]))
    for seed in range(start, start + tries):
        _, _, hs = run_model(init_tables(seed, NU, NI, d, M, stddev), batches, np.float64)
        if min_abs_h(hs) > 2 * H_MIN:
            return seed, min_abs_h(hs)
    raise RuntimeError("no seed found")


def edge_batch(rng, nu, ni, B):
    """B rows with a hot user in a third of them, users in both roles,
    i = i' rows and one row whose negative pair equals its positive pair."""
    pos = np.stack([rng.randint(0, nu, B), rng.randint(0, ni, B)], 1)
    neg = np.stack([rng.randint(0, nu, B), rng.randint(0, ni, B)], 1)
    pos[: (B + 2) // 3, 0] = 3                 # a hot user
    neg[B // 2:, 0] = pos[: B - B // 2, 0]     # users in both roles
    neg[::4, 1] = pos[::4, 1]                  # i == i'
    neg[B - 1] = pos[B - 1]                    # neg == pos
    return pos.astype(np.int64), neg.astype(np.int64)


def edge_case(B, d, n_steps=6):
    """Initial tables and the batches of one edge shape."""
    seed = EDGE_SEEDS[(B, d)]
    rng = np.random.RandomState(1000 * B + d + 7919 * seed)
    batches = [edge_batch(rng, EDGE_NU, EDGE_NI, B) for _ in range(n_steps)]
    return init_tables(seed, EDGE_NU, EDGE_NI, d, EDGE_M[d], 0.3), batches


def band_ratio(got, ref, rtol=1e-5, atol=1e-6):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref) / (atol + rtol * np.abs(ref))))
