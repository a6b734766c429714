"""fp64 numpy restatement of the VampPrior mixture density (reference models/BaseModel.py:84-96,124-128) and of what
autograd derives from it -- the yardstick of tests/test_gpu_vampprior.py, itself pinned to the real reference by golden G24
(tests/test_vampprior_host.py) -- plus the input families those tests and tools/gen_goldens.py::g24 share.

    p_ij   = -1/2 sum_d [ lv_jd + log 2pi + (z_id - mu_jd)^2 exp(-lv_jd) ] - log(n_components)
    logp_i = logsumexp_j p_ij
"""
import numpy as np

import golden_inputs as gi

LOG_2PI = np.log(2.0 * np.pi)


def matrix(z, mu, lv, n_components):
    """p [B x C], fp64, in row blocks so that the [B x C x zdim] difference tensor stays small"""
    z, mu, lv = (np.asarray(a, np.float64) for a in (z, mu, lv))
    w = np.exp(-lv)
    cst = -0.5 * (lv + LOG_2PI).sum(axis=1) - np.log(float(n_components))
    out = np.empty((z.shape[0], mu.shape[0]))
    step = max(1, (1 << 22) // max(mu.size, 1))
    for s in range(0, z.shape[0], step):
        d = z[s:s + step, None, :] - mu[None, :, :]
        out[s:s + step] = cst[None, :] - 0.5 * (d * d * w[None]).sum(axis=2)
    return out


def logp_of(p):
    m = p.max(axis=1)
    return m + np.log(np.exp(p - m[:, None]).sum(axis=1))


def forward(z, mu, lv, n_components):
    """logp [B], fp64"""
    return logp_of(matrix(z, mu, lv, n_components))


def grads(z, mu, lv, n_components, gout):
    """(dz, dmu, dlv) of sum_i gout_i logp_i, fp64"""
    z, mu, lv, gout = (np.asarray(a, np.float64) for a in (z, mu, lv, gout))
    p = matrix(z, mu, lv, n_components)
    r = gout[:, None] * np.exp(p - logp_of(p)[:, None])          # [B x C]
    w = np.exp(-lv)
    dz = np.empty_like(z)
    dmu = np.zeros_like(mu)
    dlv = np.zeros_like(lv)
    step = max(1, (1 << 22) // max(mu.size, 1))
    for s in range(0, z.shape[0], step):
        d = z[s:s + step, None, :] - mu[None, :, :]              # [b x C x zdim]
        rb = r[s:s + step, :, None]
        dz[s:s + step] = -(rb * d * w[None]).sum(axis=1)
        dmu += (rb * d * w[None]).sum(axis=0)
        dlv += (rb * 0.5 * (d * d * w[None] - 1.0)).sum(axis=0)
    return dz, dmu, dlv


def inputs(seed, B, C, zdim):
    """(z [B x zdim], mu [C x zdim], lv [C x zdim], gout [B]) fp32: clustered latents, per-component log-variances uniform on
    [-6, 2] (the range of the model's hardtanh) with some entries exactly at either end."""
    z, mu = gi.clustered_latents(seed, B, C, zdim)
    rs = np.random.RandomState(seed + 1000)
    lv = rs.uniform(-6.0, 2.0, size=(C, zdim)).astype(np.float32)
    flat = lv.reshape(-1)
    n_end = max(1, flat.size // 16)
    flat[rs.choice(flat.size, size=n_end, replace=False)] = -6.0
    flat[rs.choice(flat.size, size=n_end, replace=False)] = 2.0
    if flat.size >= 2:
        flat[0], flat[-1] = -6.0, 2.0
    gout = rs.standard_normal(B).astype(np.float32)
    return z, mu, lv, gout
