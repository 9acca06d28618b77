"""UserCF driver (src/models/basic/testucf.py:14-114): same globals and worker."""
import os

from ..usercf import UserCF
from ._common import args, load_fold, run_folds

folds = 5
binarize_threshold = 3

topK = 200

topN = 100
split_method = 'cv'
eval_metrics = ['pre', 'recall', 'map', 'mrr', 'ndcg']


def worker(fold, n_users, n_items, dataset_dir):
    trasR, tstsR = load_fold(dataset_dir, fold, n_users, n_items, binarize_threshold)
    print(dataset_dir.split('/')[-2] + '@%d:' % (fold + 1), trasR.shape, trasR.nnz,
          '%.2f' % (trasR.nnz / float(trasR.shape[0])))
    ucf = UserCF(n_users, n_items, topK, topN, split_method, eval_metrics,
                 device=int(os.environ.get("CF_DEVICE", "0")))
    scores = ucf.train(fold + 1, trasR, tstsR)
    print(dataset_dir.split('/')[-2] + '@%d:' % (fold + 1),
          ','.join(['%s' % m for m in eval_metrics]) + '@%d=' % topN +
          ','.join(['%.6f' % s for s in scores]))
    ucf.close()
    return scores


if __name__ == '__main__':
    print('topK=', topK)
    dataset_dir, nfolds, parallel = args(5)
    run_folds(worker, 943, 1682, dataset_dir, nfolds, topN, eval_metrics, parallel)
