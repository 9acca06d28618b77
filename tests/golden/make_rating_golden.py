"""Generate ``rating_stream.npz`` and ``rating_cases.json`` from the
*reference itself*.

Test infrastructure only, as ``make_golden.py``: it runs where the read-only
reference checkout lives and imports it; the GPU box only reads the files.

``rating_stream.npz``, all on ml-100k fold 1 with ``np.random.seed(17)`` set
right before the sampler is built, taken on the CONSUMER side of
``next_batch()`` of ``src/samplers/sampler_rating.py:22-39``:

* ``mf_ui`` [40, 100, 2], ``mf_r`` [40, 100]: the first 40 batches at
  ``negRatio=0``, ``batch_size=100``, raw ratings (the MF / SVD stream);
* ``wrmf_ui`` [40, 200, 2], ``wrmf_r`` [40, 200]: the first 40 batches at
  ``negRatio=1``, ``batch_size=100``, binarised > 3 (the WRMF stream);
* ``tra_indptr / tra_indices / tra_ratings``: the raw-rating train matrix the
  first stream was drawn from (``IOUtil.loadSparseR``), as CSR;
* ``tst_ui`` [n, 2], ``tst_r`` [n]: every tenth of the fold's test tuples in
  ``nonzero()`` order (about 2,000).

Ratings of ml-100k are the integers 1..5, so they are stored as int8.  40
batches stay inside the first epoch.  Each capture runs in a child process
because the reference sampler starts a non-daemon ``while True`` thread; the
child ends with ``os._exit``.

``rating_cases.json``: known answers of ``src/metrics/rating.py`` (the
``__main__`` demo case at :33 and seeded random cases with float32
predictions), computed by calling the reference functions.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEED, BATCH, N_BATCHES = 17, 100, 40


def _raw_fold():
    sys.path.insert(0, HERE)
    import make_golden as G
    G._ref_paths()
    from IOUtil import loadSparseR
    return (loadSparseR(943, 1682, G.DATA + "ratings__1_tra.txt"),
            loadSparseR(943, 1682, G.DATA + "ratings__1_tst.txt"), G)


def capture_child(which, out_path):
    tra, _, G = _raw_fold()
    if which == "wrmf":
        tra, _ = G.load_fold(1)
    np.random.seed(SEED)
    sampler = __import__("sampler_rating").Sampler(tra, negRatio=1 if which == "wrmf" else .0, batch_size=BATCH)
    batches = np.stack([np.asarray(sampler.next_batch()) for _ in range(N_BATCHES)])
    np.save(out_path, batches)
    sys.stdout.flush()
    os._exit(0)


def _capture(which):
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, which + ".npy")
        subprocess.check_call([sys.executable, __file__, "--capture", which, path], timeout=600)
        b = np.load(path)
    assert np.array_equal(b, np.rint(b))
    return b[:, :, :2].astype(np.int32), b[:, :, 2].astype(np.int8)


def make_stream():
    import scipy.sparse as sp
    tra, tst, _ = _raw_fold()
    out = {}
    out["mf_ui"], out["mf_r"] = _capture("mf")
    out["wrmf_ui"], out["wrmf_r"] = _capture("wrmf")
    assert out["mf_ui"].shape == (N_BATCHES, BATCH, 2) and out["wrmf_ui"].shape == (N_BATCHES, 2 * BATCH, 2)
    csr = sp.csr_matrix(tra)
    csr.sort_indices()
    assert np.array_equal(csr.data, np.rint(csr.data))
    out["tra_indptr"] = csr.indptr.astype(np.int32)
    out["tra_indices"] = csr.indices.astype(np.int16)
    out["tra_ratings"] = csr.data.astype(np.int8)
    t = np.array([(u, i, tst[u, i]) for u, i in np.asarray(tst.nonzero()).T])[::10]
    out["tst_ui"] = t[:, :2].astype(np.int16)
    out["tst_r"] = t[:, 2].astype(np.int8)
    np.savez_compressed(os.path.join(HERE, "rating_stream.npz"), seed=np.int64(SEED),
                        batch_size=np.int64(BATCH), **out)


def make_cases():
    sys.path.insert(0, HERE)
    import make_golden as G
    G._ref_paths()
    import rating as R
    cases = [dict(name="demo", ys_true=[2.5, 1.5, 0.0], ys_pred=[1.0, 2.0, 1.0], pred_dtype="float64")]
    rng = np.random.RandomState(5)
    for k, n in enumerate((1, 7, 100, 2001)):
        true = rng.randint(1, 11, n) / 2.0
        pred = np.clip(true + rng.randn(n), 0.5, 5.0).astype(np.float32)
        cases.append(dict(name="random%d" % k, ys_true=true.tolist(), ys_pred=[float(x) for x in pred],
                          pred_dtype="float32"))
    for c in cases:
        yt, yp = np.array(c["ys_true"]), np.array(c["ys_pred"], dtype=c["pred_dtype"])
        c["metrics"] = ["mae", "mse", "rmse", "nope"]
        c["scores"] = [None if s is None else float(s) for s in R.evaluate(yt, yp, c["metrics"])]
    with open(os.path.join(HERE, "rating_cases.json"), "w") as f:
        json.dump(cases, f)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--capture":
        capture_child(sys.argv[2], sys.argv[3])
    make_stream()
    make_cases()
    print("rating_stream.npz, rating_cases.json written to", HERE)
