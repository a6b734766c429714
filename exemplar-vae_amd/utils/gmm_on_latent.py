"""A Gaussian mixture of the latent space: the density companion of report_kmeans_on_latent, fitted to the posterior means of
the training split, scored on those of the test split and optionally decoded from.  The mixture is evae/mixture.py and the
scores of its test labels evae/cluster.py (fp64 on the device); nothing leaves the device until it is saved.  No plotting."""
import json
import os

import numpy as np
import torch

from evae.cluster import clustering_quality
from evae.mixture import GaussianMixture
from utils.knn_on_latent import _posterior_means, extract_full_data


def report_gmm_on_latent(train_loader, test_loader, model, dir, args):
    """Posterior means q(z|x) of the full batches of both splits -> a mixture fitted on the training ones.  Read from args when
    present: gmm_components (default: the number of distinct test labels), gmm_covariance_type (default 'full'), gmm_n_init
    (default 1), gmm_max_iter (default 100), seed, gmm_decode (default 0).  Writes gmm_weights.npy [K], gmm_means.npy [K x zd],
    gmm_covariances.npy (all float64), gmm_test_labels.npy [N] int32 and gmm_quality.json (lower_bound, n_iter, converged, bic,
    aic, train_mean_log_density, test_mean_log_density, nmi, ari, purity, n_components, n_train, n_test) under `dir`; with
    gmm_decode = n also gmm_samples.npy, model.generate_x_from_z of n draws.  Prints one line and returns the fitted mixture."""
    train_x, _, _ = extract_full_data(train_loader)
    test_x, _, test_y = extract_full_data(test_loader)
    with torch.no_grad():
        z_train = _posterior_means(model, train_x.to(args.device), args.batch_size)
        z_test = _posterior_means(model, test_x.to(args.device), args.batch_size)
    labels_true = test_y[:len(z_test)]
    components = getattr(args, 'gmm_components', None)
    if components is None:
        components = int(torch.unique(labels_true).numel())
    gm = GaussianMixture(n_components=int(components), covariance_type=getattr(args, 'gmm_covariance_type', 'full'),
                         n_init=int(getattr(args, 'gmm_n_init', 1)), max_iter=int(getattr(args, 'gmm_max_iter', 100)),
                         random_state=getattr(args, 'seed', None)).fit(z_train)
    test_labels = gm.predict(z_test)
    scores = clustering_quality(z_test, test_labels, labels_true=labels_true, silhouette=False)
    quality = {'lower_bound': gm.lower_bound_, 'n_iter': gm.n_iter_, 'converged': gm.converged_, 'bic': gm.bic(z_train),
               'aic': gm.aic(z_train), 'train_mean_log_density': gm.score(z_train), 'test_mean_log_density': gm.score(z_test),
               'nmi': scores['nmi'], 'ari': scores['ari'], 'purity': scores['purity'], 'n_components': gm.n_components,
               'n_train': int(len(z_train)), 'n_test': int(len(z_test))}
    os.makedirs(dir, exist_ok=True)
    np.save(os.path.join(dir, 'gmm_weights.npy'), gm.weights_.cpu().numpy())
    np.save(os.path.join(dir, 'gmm_means.npy'), gm.means_.cpu().numpy())
    np.save(os.path.join(dir, 'gmm_covariances.npy'), gm.covariances_.cpu().numpy())
    np.save(os.path.join(dir, 'gmm_test_labels.npy'), test_labels.cpu().numpy())
    with open(os.path.join(dir, 'gmm_quality.json'), 'w') as f:
        json.dump(quality, f, indent=1, sort_keys=True)
    decode = int(getattr(args, 'gmm_decode', 0) or 0)
    if decode > 0:
        with torch.no_grad():
            z, _ = gm.sample(decode)
            x = model.generate_x_from_z(z, with_reparameterize=False)
        np.save(os.path.join(dir, 'gmm_samples.npy'), x.detach().cpu().numpy())
    print('mixture of', gm.n_components, gm.covariance_type, 'Gaussians on', tuple(z_train.shape), 'latents:', gm.n_iter_,
          'iterations, converged' if gm.converged_ else 'iterations, not converged', '| mean log-density train',
          round(quality['train_mean_log_density'], 4), 'test', round(quality['test_mean_log_density'], 4), '| nmi',
          round(quality['nmi'], 4), 'ari', round(quality['ari'], 4), 'purity', round(quality['purity'], 4))
    return gm
