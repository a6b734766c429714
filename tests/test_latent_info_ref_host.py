"""CPU-only: tests/latent_info_ref.py, the yardstick of tests/test_gpu_latent_info.py, held to independent float64 formulations
-- torch.distributions.Normal(...).log_prob with torch.logsumexp, and scipy.special.logsumexp -- on the very inputs the device
is tested on, within the very bound the device is held to (ref.error_bounds); to closed forms; and its draws to their rules.

The bound has to do two things at once: hold a correct float64 evaluation (this file: torch's is one, with another expression
for the term -- sigma = exp(lv / 2), (z - mu)^2 / (2 sigma^2), log sigma), and stay small enough to catch a wrong one: it may
not exceed 1e-10 at any parity shape, where a component left out or counted twice moves a value by about 1 / N >= 1e-3."""
import math

import numpy as np
import pytest
import torch

import latent_info_ref as ref


def torch_form(z, mean, log_var, rows, chunk=8):
    """float64 torch on the host: (log_q, log_qd, log_cond)"""
    z, mean, log_var = (torch.from_numpy(np.array(a)).double() for a in (z, mean, log_var))      # (a copy: the case is read-only)
    N = mean.shape[0]
    comp = torch.distributions.Normal(mean, torch.exp(0.5 * log_var))
    log_q, log_qd, log_cond = [], [], []
    for s in range(0, len(z), chunk):
        lp = comp.log_prob(z[s:s + chunk, None, :])                       # [chunk x N x d]
        log_q.append(torch.logsumexp(lp.sum(dim=2), dim=1) - math.log(N))
        log_qd.append(torch.logsumexp(lp, dim=1) - math.log(N))
        r = torch.from_numpy(np.array(rows[s:s + chunk])).long()
        log_cond.append(lp[torch.arange(len(r)), r])
    return tuple(torch.cat(a).numpy() for a in (log_q, log_qd, log_cond))


def fraction(got, want, bound):
    return float(np.max(np.abs(got - want) / bound))


@pytest.mark.parametrize("B,N,d", ref.SHAPES, ids=lambda v: str(v))
def test_restatement_is_float64_torch_within_the_device_bound(B, N, d):
    c = ref.case(B, N, d)
    assert max(c['bq'].max(), c['bqd'].max(), c['bc'].max()) <= 1e-10
    got = torch_form(c['z'], c['mean'], c['log_var'], c['rows'])
    fr = [fraction(g, c[k], c[b]) for g, k, b in zip(got, ('log_q', 'log_qd', 'log_cond'), ('bq', 'bqd', 'bc'))]
    print("B=%d N=%d d=%d: bound <= %.3g; torch float64 at %.3f / %.3f / %.3f of it (log_q / log_qd / log_cond)"
          % (B, N, d, max(c['bq'].max(), c['bqd'].max()), *fr))
    assert max(fr) <= 1.0
    for k in ('log_q', 'log_qd', 'log_cond'):
        assert np.isfinite(c[k]).all()
    if B >= N:
        assert set(c['rows'].tolist()) == set(range(N))                   # every component was drawn from


def test_restatement_is_scipy_logsumexp():
    from scipy.special import logsumexp
    c = ref.case(65, 257, 65)
    z, mu, lv = (c[k].astype(np.float64) for k in ('z', 'mean', 'log_var'))
    t = -0.5 * (lv + math.log(2 * math.pi))[None] - 0.5 * (z[:, None, :] - mu[None]) ** 2 * np.exp(-lv)[None]
    assert fraction(logsumexp(t.sum(axis=2), axis=1) - math.log(257), c['log_q'], c['bq']) <= 1.0
    assert fraction(logsumexp(t, axis=1) - math.log(257), c['log_qd'], c['bqd']) <= 1.0
    assert fraction(t[np.arange(65), c['rows']], c['log_cond'], c['bc']) <= 1.0


def test_equal_standard_components_carry_nothing():
    N, d = 37, 5
    mean, log_var = np.zeros((N, d), np.float32), np.zeros((N, d), np.float32)
    z, rows = ref.draws(mean, log_var, random_state=3)
    info = ref.latent_information(mean, log_var, z, rows)
    assert info['mutual_information'] == 0.0 and info['total_correlation'] == 0.0
    assert info['dimension_wise_kl'] == 0.0                              # the Monte-Carlo mean of terms that are each zero
    assert not info['mutual_information_per_dimension'].any() and not info['kl_per_dimension'].any()
    assert info['active_units'] == 0 and info['active_units_by_information'] == 0 and info['log_n'] == math.log(N)


def test_two_components_far_apart_carry_log_two():
    d = 4
    mean = np.zeros((2, d), np.float32)
    mean[1, 0] = 40.0                                                     # 40 sigma apart
    log_var = np.zeros((2, d), np.float32)
    rows = np.arange(200) % 2
    z, _ = ref.draws(mean, log_var, rows=rows, random_state=1)
    info = ref.latent_information(mean, log_var, z, rows)
    assert abs(info['mutual_information'] - math.log(2.0)) <= 1e-12
    assert abs(info['mutual_information_per_dimension'][0] - math.log(2.0)) <= 1e-12
    assert np.abs(info['mutual_information_per_dimension'][1:]).max() <= 1e-15
    assert info['active_units'] == 1 and info['active_units_by_information'] == 1
    lp = ref.agg_lse(z, mean, np.log(np.full((2, d), 1.5, np.float32)))[0]          # some other density as the prior
    both = ref.latent_information(mean, log_var, z, rows, log_prior=lp)
    assert abs(both['kl'] - (both['mutual_information'] + both['marginal_kl'])) <= 4 * ref.U * max(abs(both['kl']), 1.0)


def test_one_dimension_has_no_total_correlation():
    c = ref.case(5, 2, 1)
    info = ref.latent_information(c['mean'], c['log_var'], c['z'], c['rows'])
    assert info['total_correlation'] == 0.0
    c = ref.case(17, 63, 40)
    assert ref.latent_information(c['mean'], c['log_var'], c['z'], c['rows'])['total_correlation'] > 0.1


def test_draws():
    c = ref.case(17, 63, 40)
    z1, r1 = ref.draws(c['mean'], c['log_var'], n_samples=30, random_state=7)
    z2, r2 = ref.draws(c['mean'], c['log_var'], n_samples=30, random_state=7)
    z3, r3 = ref.draws(c['mean'], c['log_var'], n_samples=30, random_state=8)
    assert z1.dtype == np.float32 and z1.shape == (30, 40)
    assert np.array_equal(z1, z2) and np.array_equal(r1, r2)
    assert not np.array_equal(z1, z3) and not np.array_equal(r1, r3)
    assert len(set(r1.tolist())) == 30 and 0 <= r1.min() and r1.max() < 63    # without replacement
    z_all, r_all = ref.draws(c['mean'], c['log_var'], random_state=7)
    assert np.array_equal(r_all, np.arange(63)) and z_all.shape == (63, 40)       # the default: every row once, in order
    # the draws are draws of the posteriors: standardised, they are standard normals
    e = (z_all - c['mean']) * np.exp(-0.5 * c['log_var'].astype(np.float64))
    assert abs(e.mean()) < 0.08 and abs(e.std() - 1.0) < 0.06
