"""Shared inputs of the pointwise tests (tests/test_pointwise_model.py,
tests/test_rating_sampler.py, tests/test_gpu_pointwise.py): the reference's
captured sampler_rating streams, fold 1 with raw ratings, seeded initial
tables, the edge-shape batches and the float64 / float32 model runs."""
import os

import numpy as np
import scipy.sparse as sp

import pointwise_model as PM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NU, NI = 943, 1682
EDGE_NU, EDGE_NI = 50, 80
REG, LR = 0.1, 0.1
WEIGHT = {"mf": 1.0, "svd": 1.0, "wrmf": 2.0}
RATOL, AATOL = 1e-5, 1e-6     # conftest's RTOL, ATOL


def golden():
    with np.load(os.path.join(GOLDEN, "rating_stream.npz")) as z:
        return {k: z[k] for k in z.files}


def stream(kind):
    """The captured batches: MF / SVD read raw ratings, WRMF binarised + negatives."""
    g = golden()
    p = "wrmf" if kind == "wrmf" else "mf"
    return g[p + "_ui"].astype(np.int32), g[p + "_r"].astype(np.float32)


def raw_train():
    g = golden()
    return sp.csr_matrix((g["tra_ratings"].astype(np.float64), g["tra_indices"].astype(np.int32),
                          g["tra_indptr"].astype(np.int64)), shape=(NU, NI))


def tst_tuples():
    """Every tenth test tuple of fold 1 (about 2,000)."""
    g = golden()
    return g["tst_ui"].astype(np.int32), g["tst_r"].astype(np.float32)


def tables_names(kind):
    t = ("user", "item", "acc_user", "acc_item")
    return t + ("kernel", "acc_kernel") if kind == "svd" else t


def init_tables(kind, seed, nu, ni, d, stddev=0.1):
    """float32 U, V (svd: K) ~ truncated normal(0, stddev^2) at two sigma, the
    accumulators at 0.1 (mf.py:26-31; tf.train.AdagradOptimizer)."""
    rng = np.random.RandomState(seed)

    def tn(shape):
        x = rng.randn(*shape)
        bad = np.abs(x) > 2
        while bad.any():
            x[bad] = rng.randn(int(bad.sum()))
            bad = np.abs(x) > 2
        return (x * stddev).astype(np.float32)

    T = dict(user=tn((nu, d)), item=tn((ni, d)))
    if kind == "svd":
        T["kernel"] = tn((d, d))
    for n in list(T):
        T["acc_" + n] = np.full_like(T[n], 0.1)
    return T


def cast(T, dtype):
    return {n: t.astype(dtype) for n, t in T.items()}


def run_model(kind, T0, batches, dtype):
    T = cast(T0, dtype)
    losses = [PM.step(kind, T, ui, r, REG, LR, WEIGHT[kind]) for ui, r in batches]
    return T, losses


def band_ratio(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref) / (AATOL + RATOL * np.abs(ref))))


def fp32_ratio(kind, T0, batches):
    """Worst |float32 model - float64 model| / default band over the tables
    after the batches: how far float32 arithmetic alone leaves the band."""
    T64, _ = run_model(kind, T0, batches, np.float64)
    T32, _ = run_model(kind, T0, batches, np.float32)
    return max(band_ratio(T32[n], T64[n]) for n in tables_names(kind))


def edge_batch(rng, nu, ni, B, single_user=False):
    """B rows (u, i, r): one user in a third of the rows, an item repeated under
    different users, one exact duplicate row; single_user: one user throughout."""
    ui = np.stack([rng.randint(0, nu, B), rng.randint(0, ni, B)], 1)
    r = rng.randint(1, 6, B).astype(np.float32)
    ui[: (B + 2) // 3, 0] = 3                  # a hot user
    if single_user:
        ui[:, 0] = 7
    if B >= 4:
        ui[::4, 1] = ui[0, 1]                  # one item under different users
    if B >= 2:
        ui[B - 1] = ui[B // 2]                 # an exact duplicate (u, i, r)
        r[B - 1] = r[B // 2]
    return ui.astype(np.int32), r


def edge_case(kind, B, d, n_steps=6):
    rng = np.random.RandomState(1000 * B + d)
    batches = [edge_batch(rng, EDGE_NU, EDGE_NI, B, single_user=(s == 2)) for s in range(n_steps)]
    return init_tables(kind, 1 + d, EDGE_NU, EDGE_NI, d), batches
