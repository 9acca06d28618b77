"""LRML driver (src/models/others/testlrml.py): same globals and worker, fed
by the sampler_lrml_ranking drop-in.  ``max_iter`` is the model's default
made a global, so that a short run needs no edit of the worker."""
import os

from ..lrml import LRML
from ..sampler_lrml_ranking import Sampler
from ._common import args, load_fold, run_folds

folds = 5
binarize_threshold = 3

n_memory = 20
margin = .2

topN = 10
split_method = 'cv'
eval_metrics = ['pre', 'recall', 'map', 'mrr', 'ndcg']
clip_norm = 1.0
n_factors = 100
batch_size = 100
max_iter = 50


def worker(fold, n_users, n_items, dataset_dir):
    trasR, tstsR = load_fold(dataset_dir, fold, n_users, n_items, binarize_threshold)
    print(dataset_dir.split('/')[-2] + '@%d:' % (fold + 1), trasR.shape, trasR.nnz,
          '%.2f' % (trasR.nnz / float(trasR.shape[0])))
    device = int(os.environ.get("CF_DEVICE", "0"))
    sampler = Sampler(trasR, batch_size=batch_size)
    lrml = LRML(n_users, n_items, topN, split_method, eval_metrics, n_memory, margin, clip_norm,
                n_factors, batch_size, max_iter=max_iter, device=device)
    scores = lrml.train(fold + 1, trasR, tstsR, sampler)
    print(dataset_dir.split('/')[-2] + '@%d:' % (fold + 1),
          ','.join(['%s' % m for m in eval_metrics]) + '@%d=' % topN +
          ','.join(['%.6f' % s for s in scores]))
    lrml.close()
    sampler.close()
    return scores


if __name__ == '__main__':
    print('n_memory=', n_memory, 'margin=', margin)
    dataset_dir, nfolds, parallel = args(1)
    run_folds(worker, 943, 1682, dataset_dir, nfolds, topN, eval_metrics, parallel)
