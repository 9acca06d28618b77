"""What the rating drivers (testmf.py, testsvd.py) share: the fold's raw
rating matrices and their (user, item, rating) tuples (testmf.py:27-37)."""
import numpy as np
import scipy.sparse as sp


def tuples_of(sR):
    """np.array([(u, i, sR[u, i]) for u, i in nonzero()]) without the Python loop."""
    csr = sp.csr_matrix(sR, dtype=np.float64)
    csr.sum_duplicates()
    csr.eliminate_zeros()
    csr.sort_indices()
    users = np.repeat(np.arange(csr.shape[0]), np.diff(csr.indptr))
    return np.stack([users.astype(np.float64), csr.indices.astype(np.float64), csr.data], 1)


def load_rating_fold(dataset_dir, fold, n_users, n_items):
    from ..io_util import loadSparseR
    tra = loadSparseR(n_users, n_items, dataset_dir + 'ratings__' + str(fold + 1) + '_tra.txt')
    tst = loadSparseR(n_users, n_items, dataset_dir + 'ratings__' + str(fold + 1) + '_tst.txt')
    return tra, tst
