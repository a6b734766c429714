"""A linear probe of the latent space: the parametric companion of report_knn_on_latent.  A softmax regression is fitted to the
posterior means of the reference split and scored on those of the query split -- are the classes linearly separable, where the
kNN vote says whether they are locally pure.  The probe is evae/linear.py (fp64 on the device), the confusion matrix
evae.ops.cluster_contingency; nothing leaves the device until it is saved.  No plotting."""
import json
import os

import numpy as np
import torch

from evae import ops
from evae.linear import LogisticRegression
from utils.knn_on_latent import _posterior_means, extract_full_data


def report_linear_probe_on_latent(train_loader, val_loader, test_loader, model, dir, args, val=True):
    """Splits and posterior means as report_knn_on_latent takes them: val=True fits on the training split and scores the
    validation split; val=False fits on training + validation and scores the test split (a trailing partial batch of either is
    dropped).  Read from args when present: probe_C (default 1.0), probe_max_iter (default 100), probe_tol (default 1e-4).
    Writes under `dir` linear_probe.json (train_accuracy, test_accuracy, test_log_loss (mean, natural logarithm), n_iter,
    converged, loss, C, classes, n_train, n_test, confusion [true class x predicted class]), linear_probe_coef.npy (float64
    [K x (zd + 1)], the intercept last) and linear_probe_test_predictions.npy (int64 [n_test], the predicted labels).  Prints
    one line and returns the fitted probe."""
    splits = [extract_full_data(loader) for loader in (train_loader, val_loader, test_loader)]
    (ref_x, _, ref_y), (val_x, _, val_y), (test_x, _, test_y) = splits
    ref_x, val_x = ref_x.to(args.device), val_x.to(args.device)
    if val is True:
        query_x, query_y = val_x, val_y
    else:
        ref_x, ref_y = torch.cat((ref_x, val_x), dim=0), torch.cat((ref_y, val_y), dim=0)
        query_x, query_y = test_x.to(args.device), test_y
    with torch.no_grad():
        z_ref = _posterior_means(model, ref_x, args.batch_size)
        z_query = _posterior_means(model, query_x, args.batch_size)
    ref_y, query_y = ref_y[:len(z_ref)].cpu().numpy(), query_y[:len(z_query)].cpu().numpy()
    clf = LogisticRegression(C=float(getattr(args, 'probe_C', 1.0)), max_iter=int(getattr(args, 'probe_max_iter', 100)),
                             tol=float(getattr(args, 'probe_tol', 1e-4))).fit(z_ref, ref_y)
    K = len(clf.classes_)
    log_proba = clf.predict_log_proba(z_query)
    predicted = clf.predict_index(z_query)
    known = np.isin(query_y, clf.classes_)                       # a query label the fit never saw has no row of its own
    true_index = torch.as_tensor(np.searchsorted(clf.classes_, query_y[known]).astype(np.int32), device=predicted.device)
    known_dev = torch.as_tensor(known, device=predicted.device)
    confusion = ops.cluster_contingency(true_index, K, predicted[known_dev].contiguous(), K) if known.any() \
        else torch.zeros((K, K), dtype=torch.int64)
    log_loss = float(-log_proba[known_dev].gather(1, true_index.long()[:, None]).mean().item()) if known.any() else float('nan')
    labels = clf.classes_[predicted.cpu().numpy()]
    result = {'train_accuracy': clf.score(z_ref, ref_y), 'test_accuracy': float((labels == query_y).mean()),
              'test_log_loss': log_loss, 'n_iter': clf.n_iter_, 'converged': clf.converged_, 'loss': clf.loss_, 'C': clf.C,
              'classes': [int(c) for c in clf.classes_], 'n_train': int(len(z_ref)), 'n_test': int(len(z_query)),
              'confusion': confusion.cpu().tolist()}
    os.makedirs(dir, exist_ok=True)
    np.save(os.path.join(dir, 'linear_probe_coef.npy'), clf._W.cpu().numpy())
    np.save(os.path.join(dir, 'linear_probe_test_predictions.npy'), labels.astype(np.int64))
    with open(os.path.join(dir, 'linear_probe.json'), 'w') as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print('linear probe on', tuple(z_ref.shape), 'latents,', K, 'classes:', clf.n_iter_,
          'iterations, converged' if clf.converged_ else 'iterations, not converged', '| accuracy train',
          round(100 * result['train_accuracy'], 2), 'test', round(100 * result['test_accuracy'], 2), '| test log-loss',
          round(log_loss, 4))
    return clf
