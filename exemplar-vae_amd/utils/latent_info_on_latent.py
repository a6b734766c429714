"""How much the latent code says about the data: the companion of report_gmm_on_latent that uses the posterior VARIANCES.  The
posteriors q(z|x) of a split give the aggregate posterior q(z); one draw per data point is scored under it, under its marginals
and under the model's prior: mutual information I(x; z), total correlation, the per-dimension KL and the split of the ELBO's
average KL term, kl = mutual_information + marginal_kl (how far the prior is from the aggregate posterior).  The numbers are
evae/latent_info.py (float64 from the device, over every component); nothing leaves the device until it is saved.  No plotting."""
import json
import os

import numpy as np
import torch

from evae.latent_info import draw_posterior_samples, latent_information
from utils.evaluation import load_all_pseudo_input
from utils.knn_on_latent import extract_full_data

_SCALARS = ('mutual_information', 'total_correlation', 'dimension_wise_kl', 'entropy_aggregate', 'log_n', 'active_units',
            'active_units_by_information', 'kl', 'marginal_kl')


def _posteriors(model, data, batch_size):
    """q(z|x) means and log-variances (the encoder's own: prior=False) of the full batches of `data`; a trailing partial batch
    is dropped, as _posterior_means drops it"""
    n = (len(data) // batch_size) * batch_size
    pairs = [model.q_z(data[s:s + batch_size], prior=False) for s in range(0, n, batch_size)]
    if not pairs:
        raise ValueError("report_latent_information: %d rows, fewer than one batch of %d" % (len(data), batch_size))
    return torch.cat([p[0] for p in pairs], dim=0).float().contiguous(), torch.cat([p[1] for p in pairs], dim=0).float().contiguous()


def report_latent_information(train_loader, test_loader, model, dir, args):
    """Posteriors of the full batches of args.latent_info_split ('test', the default, or 'train') -> one draw z_i per data
    point from a CPU generator seeded with args.seed -> evae.latent_info.latent_information, with log p(z_i) from
    model.log_p_z on utils.evaluation.load_all_pseudo_input's embedding of the training set.  That one term is the model's own
    fp32 path (the exemplar or mixture prior kernels the ELBO uses), not fp64: kl and marginal_kl carry its rounding, the
    identity kl = mutual_information + marginal_kl does not (the term cancels).  Writes latent_information.json (the scalars
    plus n, z_size, split) and latent_information_per_dimension.npy (float64 [2 x z_size]: mutual information, KL) under `dir`.
    Prints one line and returns the dict that was written."""
    split = getattr(args, 'latent_info_split', None) or 'test'
    if split not in ('train', 'test'):
        raise ValueError("latent_info_split=%r: 'train' or 'test' expected" % (split,))
    B = int(args.batch_size)
    data = extract_full_data(train_loader if split == 'train' else test_loader)[0].to(args.device)
    was_training = model.training
    model.eval()
    with torch.no_grad():
        mean, log_var = _posteriors(model, data, B)
        z, rows = draw_posterior_samples(mean, log_var, random_state=getattr(args, 'seed', None))
        embedding = load_all_pseudo_input(args, model, train_loader.dataset)
        log_prior = torch.cat([model.log_p_z((z[s:s + B], None), embedding, test=True).reshape(-1) for s in range(0, len(z), B)])
        info = latent_information(mean, log_var, z=z, rows=rows, log_prior=log_prior)
    model.train(was_training)
    report = {k: info[k] for k in _SCALARS}
    report.update(n=info['n'], z_size=info['z_size'], split=split)
    per_dimension = torch.stack((info['mutual_information_per_dimension'], info['kl_per_dimension'])).cpu().numpy()
    os.makedirs(dir, exist_ok=True)
    with open(os.path.join(dir, 'latent_information.json'), 'w') as f:
        json.dump(report, f, indent=1, sort_keys=True)
    np.save(os.path.join(dir, 'latent_information_per_dimension.npy'), per_dimension)
    print('latent information of', report['n'], split, 'posteriors, z =', report['z_size'], '| I(x;z) %.4f of log n %.4f'
          % (report['mutual_information'], report['log_n']), '| KL(q(z)||p(z)) %.4f' % report['marginal_kl'],
          '| total correlation %.4f' % report['total_correlation'], '| dimension-wise KL %.4f' % report['dimension_wise_kl'],
          '| active units', report['active_units'], '(variance),', report['active_units_by_information'], '(information)')
    return report
