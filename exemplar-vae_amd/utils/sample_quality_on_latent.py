"""Quality of the model's own samples: the companion of report_gmm_on_latent that looks at what the decoder produces.  Samples
of model.generate_x are scored against the test split -- precision, recall, density, coverage -- and against the training split
-- authenticity: for an exemplar model, whose prior is centred on the training images, the number that tells good samples from
copies.  The scores are evae/sample_quality.py (exact integers from the device); nothing leaves the device until it is saved.
No plotting."""
import json
import os

import numpy as np
import torch

from evae.sample_quality import nearest_real, sample_quality
from utils.knn_on_latent import _posterior_means, extract_full_data

_SPACES = {'latent': ('latent',), 'pixel': ('pixel',), 'both': ('latent', 'pixel')}


def _full_batches(x, batch_size):
    return x[:(len(x) // batch_size) * batch_size]


def report_sample_quality(train_loader, test_loader, model, dir, args):
    """model.generate_x draws of the prior, in batches of args.batch_size, scored against the full batches of the test split and
    (authenticity, nearest training image) of the training split.  Read from args when present: sample_quality_samples (default:
    as many as test rows; rounded down to full batches like the splits), sample_quality_space ('latent', the default: posterior
    means q(z|x) of all three sets; 'pixel': flattened images; 'both'), sample_quality_k (default 5), sample_quality_save
    (default 0).  Writes sample_quality.json under `dir`: one object per space with precision, recall, density, coverage,
    authenticity, nearest_distance_median, nearest_k, n_real, n_fake, n_train.  With sample_quality_save also
    sample_quality_nearest.npy, int32 [samples]: the training row nearest to every sample in the (first) space scored.  With
    sample_quality_distances (default False) every space also gets frechet_distance, kid (against the test split) and kid_train
    (against the training split), each where the device kernels take the space's width: the 784 pixels are wider than both
    caps (256), so the pixel space keeps its ball counts only; the latent space gets all three.  Prints
    one line and returns the dict that was written."""
    spaces = _SPACES.get(getattr(args, 'sample_quality_space', None) or 'latent')
    if spaces is None:
        raise ValueError("sample_quality_space=%r: 'latent', 'pixel' or 'both' expected" % (args.sample_quality_space,))
    B = int(args.batch_size)
    k = int(getattr(args, 'sample_quality_k', None) or 5)
    distances = bool(getattr(args, 'sample_quality_distances', False))
    train_x = _full_batches(extract_full_data(train_loader)[0], B).to(args.device)
    test_x = _full_batches(extract_full_data(test_loader)[0], B).to(args.device)
    count = getattr(args, 'sample_quality_samples', None)
    count = len(test_x) if count is None else (int(count) // B) * B
    if count < B:
        raise ValueError("report_sample_quality: %d samples asked for, at least one batch of %d expected" % (count, B))
    was_training = model.training
    model.eval()
    report = {}
    with torch.no_grad():
        draws = [model.generate_x(N=B, dataset=train_loader.dataset).detach() for _ in range(count // B)]
        fake_x = _full_batches(torch.cat([x.reshape(len(x), -1) for x in draws], dim=0), B)     # a vampprior draws at most its components
        if len(fake_x) == 0:
            raise ValueError("report_sample_quality: generate_x gave fewer than one batch of %d" % B)
        count = len(fake_x)
        sets = {}
        if 'latent' in spaces:
            sets['latent'] = tuple(_posterior_means(model, x, B) for x in (train_x, test_x, fake_x))
        if 'pixel' in spaces:
            sets['pixel'] = tuple(x.reshape(len(x), -1).float() for x in (train_x, test_x, fake_x))
        for space in spaces:
            train, test, fake = sets[space]
            report[space] = dict(sample_quality(test, fake, nearest_k=k, train=train, distances=distances), n_train=int(len(train)))
        nearest = nearest_real(sets[spaces[0]][0], sets[spaces[0]][2])[0] if getattr(args, 'sample_quality_save', 0) else None
    model.train(was_training)
    os.makedirs(dir, exist_ok=True)
    with open(os.path.join(dir, 'sample_quality.json'), 'w') as f:
        json.dump(report, f, indent=1, sort_keys=True)
    if nearest is not None:
        np.save(os.path.join(dir, 'sample_quality_nearest.npy'), nearest.cpu().numpy())
    print('sample quality of', count, 'draws, k =', k, '|', ' | '.join(
        '%s: precision %.4f recall %.4f density %.4f coverage %.4f authenticity %.4f' % (
            s, q['precision'], q['recall'], q['density'], q['coverage'], q['authenticity']) for s, q in report.items()))
    return report
