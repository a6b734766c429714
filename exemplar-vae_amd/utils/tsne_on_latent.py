"""t-SNE picture of the latent space (reference analysis.py --tsne_visualization: posterior means of the test set handed to
scikit-learn on the host).  Here the embedding is the exact t-SNE of evae/tsne.py and never leaves the device until it is
saved; the sibling of utils/knn_on_latent.py::report_knn_on_latent.  No plotting."""
import json
import os

import numpy as np
import torch

from evae.tsne import TSNE, embedding_quality
from utils.knn_on_latent import _posterior_means, extract_full_data


def report_tsne_on_latent(test_loader, model, dir, args):
    """Posterior means q(z|x) of the full batches of the test split (batches of args.batch_size; a trailing partial batch is
    dropped, as in report_knn_on_latent) -> their 2-D embedding.  Writes tsne.npy [N x 2] and tsne_labels.npy [N] under `dir`
    and returns the embedding (on the device).  Read from args when present: tsne_perplexity (30), tsne_n_iter (1000), tsne_method ('exact';
    'neighbours' for more than evae.ops.tsne_max_points() latents), tsne_init ('random'; 'pca' starts from the latents' first two
    principal components and does not depend on seed), seed, tsne_quality_neighbours (0: off; k > 0 additionally writes
    tsne_quality.json -- evae.tsne.embedding_quality of latents and embedding at k neighbours with the labels' vote, plus
    kl_divergence and method -- and prints one more line)."""
    test_x, _, test_y = extract_full_data(test_loader)
    with torch.no_grad():
        z = _posterior_means(model, test_x.to(args.device), args.batch_size)
    tsne = TSNE(perplexity=float(getattr(args, 'tsne_perplexity', 30.0)), n_iter=int(getattr(args, 'tsne_n_iter', 1000)),
                random_state=getattr(args, 'seed', None), method=getattr(args, 'tsne_method', 'exact'),
                init=getattr(args, 'tsne_init', 'random'))
    embedding = tsne.fit_transform(z)
    labels = test_y[:len(embedding)]
    os.makedirs(dir, exist_ok=True)
    np.save(os.path.join(dir, 'tsne.npy'), embedding.cpu().numpy())
    np.save(os.path.join(dir, 'tsne_labels.npy'), labels.cpu().numpy())
    print('t-SNE of', tuple(z.shape), 'latents: KL', round(tsne.kl_divergence_, 4))
    k = int(getattr(args, 'tsne_quality_neighbours', 0) or 0)
    if k > 0:
        quality = embedding_quality(z, embedding, n_neighbors=k, labels=labels)
        quality.update(kl_divergence=tsne.kl_divergence_, method=tsne.method)
        with open(os.path.join(dir, 'tsne_quality.json'), 'w') as f:
            json.dump(quality, f, indent=1, sort_keys=True)
        print('t-SNE quality at', k, 'neighbours: trustworthiness', round(quality['trustworthiness'], 4), 'continuity',
              round(quality['continuity'], 4), 'neighbourhood preservation', round(quality['neighbourhood_preservation'], 4),
              'label accuracy', round(quality['label_accuracy'], 4))
    return embedding
