"""fp64 restatement of one standard-normal-prior `vae` step (reference models/BaseModel.py:65-77 over AbsModel.py:13-49 with
log_p_z = log_normal_standard, utils/distributions.py:36-41) -- the yardstick of tests/test_gpu_standard_prior.py: the latent
block's forward and backward as the two kernels of csrc/evae_latent_std.hip see them (numpy, composed from oracle/evae_oracle.py's
functions), and the whole step -- loss, RE, KL and every parameter gradient -- through float64 torch autograd on the CPU.

    logp_i = sum_d (-z_id^2 / 2 - log(2 pi) / 2)          KL_i = logq_i - logp_i          loss_i = -RE_i + beta KL_i
"""
import numpy as np

import evae_oracle as orc

LO, HI = -6.0, 2.0


def heads_forward(x, wm, bm, wl, bl, eps, lo=LO, hi=HI):
    """-> dict(mean, pre, lv, z [M x Z], logq, logp [M]), fp64"""
    x, wm, bm, wl, bl, eps = (np.asarray(a, np.float64) for a in (x, wm, bm, wl, bl, eps))
    mean = orc.linear(x, wm, bm)
    pre = orc.linear(x, wl, bl)
    lv = orc.hardtanh(pre, lo, hi)
    z = mean + eps * np.exp(0.5 * lv)
    return dict(mean=mean, pre=pre, lv=lv, z=z, logq=orc.log_normal_diag(z, mean, lv), logp=orc.log_normal_standard(z))


def heads_backward(lv, pre, eps, z, dz, cKL, wm, wl, out_prev, s_prev, lo=LO, hi=HI):
    """Backward of the same block for the upstream gradients dz (decoder) and cKL = d loss / d KL per row (KL = logq - logp):
    -> (dmu, dlv_pre [M x Z], dh, dg [M x K]) fp64, (dh, dg) the gradient of the two pre-activations of the gated layer below."""
    lv, pre, eps, z, dz, cKL, wm, wl, out_prev, s_prev = (np.asarray(a, np.float64) for a in
                                                          (lv, pre, eps, z, dz, cKL, wm, wl, out_prev, s_prev))
    ck = cKL[:, None]
    dz_tot = dz + ck * z                                   # -d logp / dz = z
    dmu = dz_tot
    dlv = 0.5 * dz_tot * np.exp(0.5 * lv) * eps - 0.5 * ck      # d logq / d lv = -1/2 (the eps^2 term carries no gradient)
    dlv_pre = np.where((pre > lo) & (pre < hi), dlv, 0.0)
    dA = dmu @ wm + dlv_pre @ wl
    return dmu, dlv_pre, dA * s_prev, dA * out_prev * (1.0 - s_prev)


def step(sd, x, eps, beta, average=True, upstream=None):
    """One step of the model whose state dict (numpy) is `sd`.  -> (loss, RE, KL) -- [B] each, or the batch means -- and the
    gradient of sum(upstream * loss) (per-row outputs; default 1/B: the mean loss) or of the mean loss (average) for every
    parameter, fp64."""
    import torch
    p = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in sd.items()}
    xt = torch.tensor(np.asarray(x, np.float64))
    et = torch.tensor(np.asarray(eps, np.float64))

    def gated(h, pre):
        a = h @ p[pre + ".h.weight"].T + p[pre + ".h.bias"]
        g = h @ p[pre + ".g.weight"].T + p[pre + ".g.bias"]
        return a * torch.sigmoid(g)
    h2 = gated(gated(xt, "q_z_layers.0"), "q_z_layers.1")
    mean = h2 @ p["q_z_mean.weight"].T + p["q_z_mean.bias"]
    lv = torch.clamp(h2 @ p["q_z_logvar.linear.weight"].T + p["q_z_logvar.linear.bias"], LO, HI)
    z = mean + et * torch.exp(0.5 * lv)
    log2pi = float(np.log(2.0 * np.pi))
    logq = (-0.5 * (lv + log2pi + (z - mean) ** 2 / torch.exp(lv))).sum(1)
    logp = (-0.5 * z * z - 0.5 * log2pi).sum(1)
    d2 = gated(gated(z, "p_x_layers.0"), "p_x_layers.1")
    xm = torch.sigmoid(d2 @ p["p_x_mean.linear.weight"].T + p["p_x_mean.linear.bias"])
    pr = torch.clamp(xm, 1e-5, 1.0 - 1e-5)
    RE = (xt * torch.log(pr) + (1.0 - xt) * torch.log(1.0 - pr)).sum(1)
    KL = logq - logp
    loss = -RE + float(beta) * KL
    B = xt.shape[0]
    if average or upstream is None:
        loss.mean().backward()
    else:
        (loss * torch.tensor(np.asarray(upstream, np.float64))).sum().backward()
    grads = {k: v.grad.numpy() for k, v in p.items()}
    out = tuple(t.detach().numpy() for t in (loss, RE, KL))
    if average:
        out = tuple(t.mean() for t in out)
    return out, grads
