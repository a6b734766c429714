"""PCA picture of the latent space: the linear companion of utils/tsne_on_latent.py::report_tsne_on_latent, on the same posterior
means.  The decomposition is evae/pca.py (fp64 on the device); nothing leaves the device until it is saved.  No plotting."""
import os

import numpy as np
import torch

from evae import ops
from evae.pca import PCA
from utils.knn_on_latent import _posterior_means, extract_full_data


def report_pca_on_latent(test_loader, model, dir, args):
    """Posterior means q(z|x) of the full batches of the test split (as report_tsne_on_latent takes them) -> their projection on
    the first two principal components.  Writes pca.npy [N x 2], pca_labels.npy [N] and pca_explained_variance_ratio.npy [zd]
    under `dir`, prints how many components hold 95 % of the variance -- a finer count than the active units of
    compute_mean_variance_per_dimension -- and returns the projection (on the device)."""
    test_x, _, test_y = extract_full_data(test_loader)
    with torch.no_grad():
        z = _posterior_means(model, test_x.to(args.device), args.batch_size)
    pca = PCA().fit(z)
    with torch.no_grad():
        projection = ops.pca_project(z, pca.mean_, pca.components_[:2].contiguous())
    ratio = pca.explained_variance_ratio_.cpu().numpy()
    labels = test_y[:len(projection)]
    os.makedirs(dir, exist_ok=True)
    np.save(os.path.join(dir, 'pca.npy'), projection.cpu().numpy())
    np.save(os.path.join(dir, 'pca_labels.npy'), labels.cpu().numpy())
    np.save(os.path.join(dir, 'pca_explained_variance_ratio.npy'), ratio)
    if not ratio.sum() > 0.0:                                 # PCA gives zeros, not 0 / 0, for latents that are all equal
        print('PCA of', tuple(z.shape), 'latents: no variance, no component count')
        return projection
    needed = int(np.searchsorted(np.cumsum(ratio), 0.95) + 1)
    print('PCA of', tuple(z.shape), 'latents:', min(needed, len(ratio)), 'of', len(ratio), 'components hold 95 % of the variance;',
          'the first two hold', round(float(ratio[:2].sum()), 4))
    return projection
