"""MF driver (src/models/basic/testmf.py): same globals and worker, fed by the
sampler_rating drop-in.  ``max_iter`` is the model's default made a global, so
that a short run needs no edit of the worker."""
import os

from ..mf import MF
from ..sampler_rating import Sampler
from ._common import args, run_folds
from ._rating_common import load_rating_fold, tuples_of

cv_folds = 5
eval_metrics = ['rmse', 'mae', 'mse']

reg = .1

range_of_ratings = (1, 5)
n_factors = 100
batch_size = 1000
max_iter = 50


def worker(fold, n_users, n_items, dataset_dir):
    trasR, tstsR = load_rating_fold(dataset_dir, fold, n_users, n_items)
    print(dataset_dir.split('/')[-2] + ':', trasR.shape, trasR.nnz, '%.2f' % (trasR.nnz / float(trasR.shape[0])))
    tra_tuple, tst_tuple = tuples_of(trasR), tuples_of(tstsR)
    device = int(os.environ.get("CF_DEVICE", "0"))
    sampler = Sampler(trasR=trasR, negRatio=.0, batch_size=batch_size)
    mf = MF(n_users, n_items, eval_metrics, range_of_ratings, reg, n_factors, batch_size, max_iter=max_iter,
            device=device)
    scores = mf.train(fold + 1, tra_tuple, tst_tuple, sampler)
    print('fold=%d:' % fold, ','.join(['%s' % m for m in eval_metrics]), '=',
          ','.join(['%.6f' % s for s in scores]))
    mf.close()
    sampler.close()
    return scores


if __name__ == '__main__':
    print('reg=', reg)
    dataset_dir, nfolds, parallel = args(cv_folds)
    run_folds(worker, 943, 1682, dataset_dir, nfolds, '', eval_metrics, parallel)
