"""Generate ``lrml_stream.npz`` from the *reference itself*.

Test infrastructure only, as ``make_golden.py``: it runs where the read-only
reference checkout lives and imports it; the GPU box only reads the file.

Captured: the first 40 ``(pos, neg)`` batches of
``src/samplers/sampler_lrml_ranking.py:20-35`` on ml-100k fold 1 at
``batch_size=100``, with ``np.random.seed(17)`` set right before the sampler
is built, taken on the CONSUMER side of ``next_batch()``.  40 batches stay
inside the first epoch (442 batches), so the queue's last-batch race never
appears in the fixture.  The capture runs in a child process because the
reference sampler starts a non-daemon ``while True`` thread; the child ends
with ``os._exit``.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEED, BATCH, N_BATCHES = 17, 100, 40


def capture_child(out_path):
    sys.path.insert(0, HERE)
    import make_golden as G
    tra, _ = G.load_fold(1)
    np.random.seed(SEED)
    sampler = __import__("sampler_lrml_ranking").Sampler(tra, batch_size=BATCH)
    batches = [sampler.next_batch() for _ in range(N_BATCHES)]
    np.savez(out_path,
             pos=np.stack([np.asarray(b[0]) for b in batches]).astype(np.int32),
             neg=np.stack([np.asarray(b[1]) for b in batches]).astype(np.int32))
    sys.stdout.flush()
    os._exit(0)


def make_stream():
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "lrml.npz")
        subprocess.check_call([sys.executable, __file__, "--capture", path], timeout=300)
        with np.load(path) as z:
            pos, neg = z["pos"], z["neg"]
    assert pos.shape == neg.shape == (N_BATCHES, BATCH, 2)
    np.savez_compressed(os.path.join(HERE, "lrml_stream.npz"), pos=pos, neg=neg,
                        seed=np.int64(SEED), batch_size=np.int64(BATCH))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--capture":
        capture_child(sys.argv[2])
    make_stream()
    print("lrml_stream.npz written to", HERE)
