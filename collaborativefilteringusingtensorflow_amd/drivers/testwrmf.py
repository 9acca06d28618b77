"""WRMF driver (src/models/basic/testwrmf.py): same globals and worker, fed by
the sampler_rating drop-in with negRatio 1.  ``max_iter`` is the model's
default made a global, so that a short run needs no edit of the worker."""
import os

from ..sampler_rating import Sampler
from ..wrmf import WRMF
from ._common import args, load_fold, run_folds

folds = 5
binarize_threshold = 3

weight = 2.
reg = .1

topN = 10
split_method = 'cv'
eval_metrics = ['pre', 'recall', 'map', 'mrr', 'ndcg']
negRatio = 1
n_factors = 100
batch_size = 100
max_iter = 50


def worker(fold, n_users, n_items, dataset_dir):
    trasR, tstsR = load_fold(dataset_dir, fold, n_users, n_items, binarize_threshold)
    print(dataset_dir.split('/')[-2] + '@%d:' % (fold + 1), trasR.shape, trasR.nnz,
          '%.2f' % (trasR.nnz / float(trasR.shape[0])))
    device = int(os.environ.get("CF_DEVICE", "0"))
    sampler = Sampler(trasR, negRatio, batch_size)
    wrmf = WRMF(n_users, n_items, topN, split_method, eval_metrics, weight, reg, n_factors, batch_size,
                max_iter=max_iter, device=device)
    scores = wrmf.train(fold + 1, trasR, tstsR, sampler)
    print(dataset_dir.split('/')[-2] + '@%d:' % (fold + 1), 'weight=', weight, 'reg=', reg)
    print('fold=%d:' % (fold + 1), ','.join(['%s' % m for m in eval_metrics]), '=',
          ','.join(['%.6f' % s for s in scores]))
    wrmf.close()
    sampler.close()
    return scores


if __name__ == '__main__':
    print('weight=', weight, 'reg=', reg)
    dataset_dir, nfolds, parallel = args(3)
    run_folds(worker, 943, 1682, dataset_dir, nfolds, topN, eval_metrics, parallel)
