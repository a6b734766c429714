"""t-SNE picture of the latent space (reference analysis.py --tsne_visualization: posterior means of the test set handed to
scikit-learn on the host).  Here the embedding is the exact t-SNE of evae/tsne.py and never leaves the device until it is
saved; the sibling of utils/knn_on_latent.py::report_knn_on_latent.  No plotting."""
import os

import numpy as np
import torch

from evae.tsne import TSNE
from utils.knn_on_latent import _posterior_means, extract_full_data


def report_tsne_on_latent(test_loader, model, dir, args):
    """Posterior means q(z|x) of the full batches of the test split (batches of args.batch_size; a trailing partial batch is
    dropped, as in report_knn_on_latent) -> their 2-D embedding.  Writes tsne.npy [N x 2] and tsne_labels.npy [N] under `dir`
    and returns the embedding (on the device).  Read from args when present: tsne_perplexity (30), tsne_n_iter (1000), tsne_method ('exact';
    'neighbours' for more than evae.ops.tsne_max_points() latents), seed."""
    test_x, _, test_y = extract_full_data(test_loader)
    with torch.no_grad():
        z = _posterior_means(model, test_x.to(args.device), args.batch_size)
    tsne = TSNE(perplexity=float(getattr(args, 'tsne_perplexity', 30.0)), n_iter=int(getattr(args, 'tsne_n_iter', 1000)),
                random_state=getattr(args, 'seed', None), method=getattr(args, 'tsne_method', 'exact'))
    embedding = tsne.fit_transform(z)
    labels = test_y[:len(embedding)]
    os.makedirs(dir, exist_ok=True)
    np.save(os.path.join(dir, 'tsne.npy'), embedding.cpu().numpy())
    np.save(os.path.join(dir, 'tsne_labels.npy'), labels.cpu().numpy())
    print('t-SNE of', tuple(z.shape), 'latents: KL', round(tsne.kl_divergence_, 4))
    return embedding
