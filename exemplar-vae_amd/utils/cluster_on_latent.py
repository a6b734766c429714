"""k-means of the latent space, scored against the labels: the unsupervised companion of report_knn_on_latent, on the same
posterior means as utils/tsne_on_latent.py and utils/pca_on_latent.py.  The clustering and its scores are evae/cluster.py (fp64 on
the device); nothing leaves the device until it is saved.  No plotting."""
import json
import os

import numpy as np
import torch

from evae.cluster import KMeans, clustering_quality
from utils.knn_on_latent import _posterior_means, extract_full_data


def report_kmeans_on_latent(test_loader, model, dir, args):
    """Posterior means q(z|x) of the full batches of the test split (as report_tsne_on_latent takes them) -> their k-means
    clustering.  Read from args when present: kmeans_clusters (default: the number of distinct labels), kmeans_n_init (default
    'auto'), kmeans_max_iter (default 300), seed, kmeans_silhouette (default on).  Writes kmeans_labels.npy [N] int32,
    kmeans_centres.npy [K x zd] float64 and kmeans_quality.json (inertia, n_iter, n_clusters, n_samples, nmi, ari, purity,
    silhouette -- null when switched off) under `dir`, prints one line and returns the labels (on the device)."""
    test_x, _, test_y = extract_full_data(test_loader)
    with torch.no_grad():
        z = _posterior_means(model, test_x.to(args.device), args.batch_size)
    labels_true = test_y[:len(z)]
    clusters = getattr(args, 'kmeans_clusters', None)
    if clusters is None:
        clusters = int(torch.unique(labels_true).numel())
    km = KMeans(n_clusters=int(clusters), n_init=getattr(args, 'kmeans_n_init', 'auto'),
                max_iter=int(getattr(args, 'kmeans_max_iter', 300)), random_state=getattr(args, 'seed', None)).fit(z)
    scores = clustering_quality(z, km.labels_, labels_true=labels_true, silhouette=bool(getattr(args, 'kmeans_silhouette', True)))
    quality = {'inertia': km.inertia_, 'n_iter': km.n_iter_, 'n_clusters': km.n_clusters, 'n_samples': int(len(z)),
               'nmi': scores['nmi'], 'ari': scores['ari'], 'purity': scores['purity'], 'silhouette': scores.get('silhouette')}
    os.makedirs(dir, exist_ok=True)
    np.save(os.path.join(dir, 'kmeans_labels.npy'), km.labels_.cpu().numpy())
    np.save(os.path.join(dir, 'kmeans_centres.npy'), km.cluster_centers_.cpu().numpy())
    with open(os.path.join(dir, 'kmeans_quality.json'), 'w') as f:
        json.dump(quality, f, indent=1, sort_keys=True)
    print('k-means of', tuple(z.shape), 'latents:', km.n_clusters, 'clusters in', km.n_iter_, 'iterations, inertia',
          round(km.inertia_, 4), '| nmi', round(quality['nmi'], 4), 'ari', round(quality['ari'], 4), 'purity',
          round(quality['purity'], 4), 'silhouette', None if quality['silhouette'] is None else round(quality['silhouette'], 4))
    return km.labels_
