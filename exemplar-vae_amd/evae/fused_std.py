"""One-node autograd implementation of the `vae` training loss under the standard-normal prior (--prior standard; the body of
reference models/BaseModel.py:65-77 + AbsModel.py:13-19,44-49 with log_p_z = log_normal_standard, utils/distributions.py:36-41).

A standard-prior step IS the batch rows' chain of evae/fused_vae.py and nothing else: encoder -> heads -> sample -> decoder ->
reconstruction term -> backward for the B rows.  Here that chain is a first-class node on ONE stream -- the caller's; no second
stream, no cross-branch edge in the captured graph -- with the latent block as one launch each way (csrc/evae_latent_std.hip):

    forward    2 gated encoder layers, evae_heads_reparam_std_fwd (heads + sample + log q + log p), 2 gated decoder layers, the
               sigmoid head, the reconstruction term, the ELBO's assembly                                        -- 8 launches
    backward   3 decoder data gradients, evae_heads_std_bwd (reparameterisation + Hardtanh + prior + the heads' data gradient with
               encoder layer 2's gate derivative), encoder layer 2's data gradient, ONE grouped launch for the six weight
               gradients                                                                                        -- 6 launches

(+ evae_elbo_bwd and the sigmoid head's gradient when the step's runner has not promised loss.backward(ones) on the batch means.)
Sizes the one-launch latent kernels do not take (evae_heads_std_applies) run the launches they replace; a layer the thin kernels
do not take runs on the tiled GEMMs behind the same entry points.  The same arithmetic as the modular path.

decoder_fwd, decoder_dgrads and upstream_coefs are the same launches with the same arguments in the exemplar step and serve
evae/fused_vae.py too; the rest of its chain writes into tail rows of shared buffers and into image rows.  evae/launch.py: invariants."""
from types import SimpleNamespace

import torch

from . import _lib, handoff, ops
from .launch import Launcher, beta_args, vp, wgrad_jobs

ACT_NONE, ACT_SIGMOID = ops.ACT_NONE, ops.ACT_SIGMOID
LV_LO, LV_HI = -6.0, 2.0           # the Hardtanh of q_z_logvar (models/VAE.py)

PARAM_ORDER = [
    "p_x_mean.linear.weight", "p_x_mean.linear.bias",
    "q_z_layers.0.h.weight", "q_z_layers.0.h.bias", "q_z_layers.0.g.weight", "q_z_layers.0.g.bias",
    "q_z_layers.1.h.weight", "q_z_layers.1.h.bias", "q_z_layers.1.g.weight", "q_z_layers.1.g.bias",
    "q_z_mean.weight", "q_z_mean.bias",
    "q_z_logvar.linear.weight", "q_z_logvar.linear.bias",
    "p_x_layers.0.h.weight", "p_x_layers.0.h.bias", "p_x_layers.0.g.weight", "p_x_layers.0.g.bias",
    "p_x_layers.1.h.weight", "p_x_layers.1.h.bias", "p_x_layers.1.g.weight", "p_x_layers.1.g.bias",
]
_NAMES = "wp bp w1h b1h w1g b1g w2h b2h w2g b2g wm bm wl bl d1h e1h d1g e1g d2h e2h d2g e2g".split()


def named(names, params):
    return SimpleNamespace(**dict(zip(names, params)))


# ------------------------------------------------------------------------------------------------ shared with evae/fused_vae.py
def decoder_fwd(k, st, p):
    """z -> two gated layers -> the sigmoid head, B rows, on k's stream"""
    B, D, H, Z = st.B, st.D, st.H, st.Z
    k.gated_fwd(st.z, None, B, Z, Z, p.d1h, p.e1h, p.d1g, p.e1g, H, st.D1, None, st.sd1)
    k.gated_fwd(st.D1, None, B, H, H, p.d2h, p.e2h, p.d2g, p.e2g, H, st.D2, None, st.sd2)
    k.linear_fwd(st.D2, B, H, H, p.wp, p.bp, D, ACT_SIGMOID, 0.0, 0.0, st.xmean, None)


def decoder_dgrads(k, st, p):
    """dpx -> [dh | dg] of decoder layers 2 and 1 -> dz: every gated layer's backward uses the merged [dh | dg] buffer (one
    weight-gradient job per layer) and the gate derivative of the layer below is applied in the data gradient's epilogue"""
    B, D, H, Z, t = st.B, st.D, st.H, st.Z, st.bwd
    k.bwd_data(t.dpx, p.wp, None, None, B, D, D, H, st.D2, st.sd2, t.dp2, t.dp2.data_ptr() + 4 * H, 2 * H)
    k.bwd_data(t.dp2, p.d2h, t.dp2.data_ptr() + 4 * H, p.d2g, B, H, 2 * H, H, st.D1, st.sd1, t.dp1, t.dp1.data_ptr() + 4 * H, 2 * H)
    k.bwd_data(t.dp1, p.d1h, t.dp1.data_ptr() + 4 * H, p.d1g, B, H, 2 * H, Z, None, None, t.dz, None, Z)


def upstream_coefs(k, st, dloss, dRE, dKL):
    """(cRE, cKL, -cKL) per row on st.bwd: the forward pass's when the caller kept its unit-upstream promise (-> True), else from
    the upstream gradients -- per-row vectors (average=False) or scalars of the batch means -- by evae_elbo_bwd (-> False)"""
    t, B = st.bwd, st.B
    if st.coef is not None and dRE is None and dKL is None and dloss is not None and dloss.numel() == 1:
        t.cRE, t.cKL, t.neg_cKL = st.coef
        return True
    f32 = dict(device=st.dev, dtype=torch.float32)
    t.cRE = torch.empty(B, **f32); t.cKL = torch.empty(B, **f32); t.neg_cKL = torch.empty(B, **f32)
    t.gl, t.gr, t.gk = (None if g_ is None else ops._f32(g_) for g_ in (dloss, dRE, dKL))
    beta_dev, beta_host = beta_args(st.beta)
    _lib.check(k.lib.evae_elbo_bwd(vp(t.gl), 0 if t.gl is None else t.gl.numel(), vp(t.gr), 0 if t.gr is None else t.gr.numel(),
                                   vp(t.gk), 0 if t.gk is None else t.gk.numel(), vp(beta_dev), beta_host, B, vp(t.cRE), vp(t.cKL),
                                   vp(t.neg_cKL), k.st), "elbo_bwd")
    return False


# ------------------------------------------------------------------------------------------------ the stages of this step
# (Its launches go through ops.probed like the exemplar step's; the probe records nothing below min_flops = 2 GFLOP and this step's
#  launches at B = 100 are about 0.1 GFLOP, so none of them is labelled with a matrix pipe: pipes=False)
def _launcher(dev):
    return Launcher(dev, prefix="std_", pipes=False)


def _fwd_encode(k, st, p):
    """encoder, heads, sample, both densities"""
    B, D, H, Z, lib = st.B, st.D, st.H, st.Z, k.lib
    f32 = dict(device=st.dev, dtype=torch.float32)
    # a gated layer keeps its output and its gate s for the backward (dg = dout * out * (1 - s)); h is never stored
    st.A1 = torch.empty((B, H), **f32); st.s1 = torch.empty_like(st.A1)
    st.A2 = torch.empty((B, H), **f32); st.s2 = torch.empty_like(st.A2)
    st.z_mean = torch.empty((B, Z), **f32); st.lv_pre = torch.empty_like(st.z_mean); st.logvar = torch.empty_like(st.z_mean)
    st.z = torch.empty_like(st.z_mean)
    t = st.fwd
    t.logq = torch.empty(B, **f32); t.logp = torch.empty(B, **f32)
    st.D1 = torch.empty((B, H), **f32); st.sd1 = torch.empty_like(st.D1)
    st.D2 = torch.empty((B, H), **f32); st.sd2 = torch.empty_like(st.D2)
    st.xmean = torch.empty((B, D), **f32)
    t.RE = torch.empty(B, **f32)
    k.gated_fwd(st.x, None, B, D, st.x.stride(0), p.w1h, p.b1h, p.w1g, p.b1g, H, st.A1, None, st.s1)
    k.gated_fwd(st.A1, None, B, H, H, p.w2h, p.b2h, p.w2g, p.b2g, H, st.A2, None, st.s2)
    st.one_launch = bool(lib.evae_heads_std_applies(B, H, Z, H))
    if st.one_launch:
        _lib.check(lib.evae_heads_reparam_std_fwd(vp(st.A2), B, H, H, vp(p.wm), vp(p.bm), vp(p.wl), vp(p.bl), Z, LV_LO, LV_HI, vp(st.eps),
                                                  vp(st.z_mean), vp(st.lv_pre), vp(st.logvar), vp(st.z), vp(t.logq), vp(t.logp), k.st),
                   "heads_reparam_std_fwd")
    else:
        w = k.ws("heads", lib.evae_heads_reparam_fwd_workspace_bytes(B, H, Z))
        _lib.check(lib.evae_heads_reparam_fwd(vp(st.A2), B, H, H, vp(p.wm), vp(p.bm), vp(p.wl), vp(p.bl), Z, LV_LO, LV_HI, vp(st.eps),
                                              vp(st.z_mean), vp(st.lv_pre), vp(st.logvar), vp(st.z), vp(t.logq), vp(w), w.numel(), k.st),
                   "heads_reparam_fwd")
        _lib.check(lib.evae_log_normal_std_fwd(vp(st.z), B, Z, vp(t.logp), k.st), "log_normal_std_fwd")


def _fwd_reconstruct(k, st, ho, average):
    """the reconstruction term and the ELBO's assembly -> (loss, RE, KL, means)"""
    B, D, lib, t = st.B, st.D, k.lib, st.fwd
    f32 = dict(device=st.dev, dtype=torch.float32)
    beta_dev, beta_host = beta_args(st.beta)
    if ho.unit_upstream and average:
        # the caller (evae/graph.py) promises loss.backward(ones) on the batch mean and nothing else: RE, the backward's
        # coefficient vectors (-1/B, beta/B, -beta/B) and the sigmoid head's gradient are one launch
        st.coef = (torch.empty(B, **f32), torch.empty(B, **f32), torch.empty(B, **f32))
        st.dpx = torch.empty((B, D), **f32)
        _lib.check(lib.evae_bernoulli_unit_step(vp(st.x), vp(st.xmean), B, D, vp(beta_dev), beta_host, vp(t.RE), vp(st.coef[0]),
                                                vp(st.coef[1]), vp(st.coef[2]), vp(st.dpx), k.st), "bernoulli_unit_step")
    else:
        _lib.check(lib.evae_bernoulli_ll_fwd(vp(st.x), vp(st.xmean), B, D, vp(t.RE), k.st), "bernoulli_ll_fwd")
    t.loss = torch.empty(B, **f32); t.KL = torch.empty(B, **f32)
    t.means = torch.empty(3, **f32) if average else None
    _lib.check(lib.evae_elbo_assemble(vp(t.logp), vp(t.RE), vp(t.logq), vp(beta_dev), beta_host, B, vp(t.loss), vp(t.KL), vp(t.means),
                                      k.st), "elbo_assemble")


def _bwd_buffers(st):
    B, D, H, Z, t = st.B, st.D, st.H, st.Z, st.bwd
    f32 = dict(device=st.dev, dtype=torch.float32)
    t.dp2 = torch.empty((B, 2 * H), **f32); t.dp1 = torch.empty((B, 2 * H), **f32)
    t.dz = torch.empty((B, Z), **f32)
    t.dq2 = torch.empty((B, 2 * H), **f32); t.dq1 = torch.empty((B, 2 * H), **f32)
    t.g_wp = torch.empty((D, H), **f32); t.g_bp = torch.empty(D, **f32)
    t.g_d2 = torch.empty((2 * H, H), **f32); t.g_e2 = torch.empty(2 * H, **f32)
    t.g_d1 = torch.empty((2 * H, Z), **f32); t.g_e1 = torch.empty(2 * H, **f32)
    t.g_hd = torch.empty((2 * Z, H), **f32); t.g_hb = torch.empty(2 * Z, **f32)         # [mean head | log-variance head]
    t.g_w2 = torch.empty((2 * H, H), **f32); t.g_b2 = torch.empty(2 * H, **f32)
    t.g_w1 = torch.empty((2 * H, D), **f32); t.g_b1 = torch.empty(2 * H, **f32)


def _bwd_latent(k, st, p):
    """reparameterisation + log q + Hardtanh + the prior's share of dz, and the heads' data gradient -> the heads' weight-gradient jobs"""
    B, H, Z, lib, t = st.B, st.H, st.Z, k.lib, st.bwd
    f32 = dict(device=st.dev, dtype=torch.float32)
    if st.one_launch:
        t.dhd = torch.empty((B, 2 * Z), **f32)                                         # [dmu | dlv_pre]
        _lib.check(lib.evae_heads_std_bwd(vp(st.z_mean), vp(st.logvar), vp(st.lv_pre), vp(st.eps), vp(st.z), vp(t.dz), vp(t.cKL), vp(t.neg_cKL),
                                          LV_LO, LV_HI, B, Z, vp(p.wm), vp(p.wl), H, vp(st.A2), vp(st.s2), vp(t.dhd),
                                          vp(t.dhd.data_ptr() + 4 * Z), 2 * Z, vp(t.dq2), vp(t.dq2.data_ptr() + 4 * H), 2 * H, k.st),
                   "heads_std_bwd")
        return [(t.dhd, B, 2 * Z, 2 * Z, st.A2, H, H, t.g_hd, t.g_hb)]
    t.dzp = torch.empty((B, Z), **f32); t.dmu = torch.empty((B, Z), **f32); t.dlvp = torch.empty((B, Z), **f32)
    _lib.check(lib.evae_log_normal_std_bwd(vp(st.z), vp(t.neg_cKL), B, Z, vp(t.dzp), k.st), "log_normal_std_bwd")
    _lib.check(lib.evae_reparam_logq_bwd_hardtanh(vp(st.z_mean), vp(st.logvar), vp(st.eps), vp(st.z), vp(t.dz), vp(t.dzp), vp(t.cKL),
                                                  vp(st.lv_pre), LV_LO, LV_HI, B, Z, vp(t.dmu), vp(t.dlvp), k.st), "reparam_logq_bwd")
    k.bwd_data(t.dmu, p.wm, t.dlvp, p.wl, B, Z, Z, H, st.A2, st.s2, t.dq2, t.dq2.data_ptr() + 4 * H, 2 * H)
    return [(t.dmu, B, Z, Z, st.A2, H, H, t.g_hd[:Z], t.g_hb[:Z]), (t.dlvp, B, Z, Z, st.A2, H, H, t.g_hd[Z:], t.g_hb[Z:])]


def _bwd_weights(k, jobs):
    """jobs: (dy, M, N, ldy, x, K, ldx, dw, db).  Those the grouped kernel takes (a contraction over <= 128 rows, widths in
    fours) go out six to a launch; the rest one by one."""
    fits = [j[1] <= 128 and all(v % 4 == 0 for v in (j[2], j[3], j[5], j[6])) and all(vp(t).value % 16 == 0 for t in (j[0], j[4], j[7]))
            for j in jobs]
    grouped = [j for j, ok in zip(jobs, fits) if ok]
    for i in range(0, len(grouped), 6):
        arr, n, _keep = wgrad_jobs(grouped[i:i + 6])
        _lib.check(k.lib.evae_dense_bwd_weight_group(arr, n, k.st), "dense_bwd_weight_group")
    for dy, M, N, ldy, x, K, ldx, dw, db in (j for j, ok in zip(jobs, fits) if not ok):
        k.bwd_weight(dy, M, N, ldy, x, None, K, ldx, dw, db)


class VaeStandardLoss(torch.autograd.Function):
    """forward(x [B x D] binarised batch, eps [B x z], beta (float or device scalar), average, *params (PARAM_ORDER))
    -> (loss, RE, KL): [B] each, or the three batch means when `average`."""

    @staticmethod
    def forward(ctx, x, eps, beta, average, *params):
        p = named(_NAMES, params)
        k = _launcher(x.device)
        ho = handoff.current() or handoff.StepHandoff()       # what the step's runner says about this step; nothing without one
        st = ctx.step = SimpleNamespace(dev=x.device, x=ops._f32(x), eps=ops._f32(eps), beta=beta, H=p.w1h.shape[0], Z=p.wm.shape[0],
                                        coef=None, dpx=None, fwd=SimpleNamespace(), bwd=None)
        st.B, st.D = st.x.shape
        _fwd_encode(k, st, p)
        decoder_fwd(k, st, p)
        _fwd_reconstruct(k, st, ho, average)
        ctx.set_materialize_grads(False)       # unused outputs (RE, KL) then arrive as None, not as zero-filled tensors
        ctx.save_for_backward(*params)
        t, st.fwd = st.fwd, None
        if average:
            l, r, kl = t.means.unbind(0)
            return l, r, kl
        return t.loss, t.RE, t.KL

    @staticmethod
    def backward(ctx, dloss, dRE, dKL):
        p = named(_NAMES, ctx.saved_tensors)
        st = ctx.step
        k = _launcher(st.dev)
        B, D, H, Z = st.B, st.D, st.H, st.Z
        t = st.bwd = SimpleNamespace()
        if upstream_coefs(k, st, dloss, dRE, dKL):
            t.dpx = st.dpx
        else:
            # through the Bernoulli log-likelihood and the sigmoid head at once
            t.dpx = torch.empty((B, D), device=st.dev, dtype=torch.float32)
            _lib.check(k.lib.evae_bernoulli_sigmoid_bwd(vp(st.x), vp(st.xmean), vp(t.cRE), B, D, vp(t.dpx), k.st), "bernoulli_sigmoid_bwd")
        _bwd_buffers(st)
        decoder_dgrads(k, st, p)
        head_jobs = _bwd_latent(k, st, p)
        # ---- encoder layer 2's data gradient (layer 1's gate derivative in its epilogue), then every weight gradient: leaves
        k.bwd_data(t.dq2, p.w2h, t.dq2.data_ptr() + 4 * H, p.w2g, B, H, 2 * H, H, st.A1, st.s1, t.dq1, t.dq1.data_ptr() + 4 * H, 2 * H)
        _bwd_weights(k, [(t.dpx, B, D, D, st.D2, H, H, t.g_wp, t.g_bp), (t.dp2, B, 2 * H, 2 * H, st.D1, H, H, t.g_d2, t.g_e2),
                         (t.dp1, B, 2 * H, 2 * H, st.z, Z, Z, t.g_d1, t.g_e1)] + head_jobs +
                     [(t.dq2, B, 2 * H, 2 * H, st.A1, H, H, t.g_w2, t.g_b2), (t.dq1, B, 2 * H, 2 * H, st.x, D, st.x.stride(0), t.g_w1, t.g_b1)])
        ctx.step = SimpleNamespace(coef=st.coef, dpx=st.dpx)      # (the activations go here; these two with the node, as they always did)
        grads = (t.g_wp, t.g_bp, t.g_w1[:H], t.g_b1[:H], t.g_w1[H:], t.g_b1[H:], t.g_w2[:H], t.g_b2[:H], t.g_w2[H:], t.g_b2[H:],
                 t.g_hd[:Z], t.g_hb[:Z], t.g_hd[Z:], t.g_hb[Z:], t.g_d1[:H], t.g_e1[:H], t.g_d1[H:], t.g_e1[H:], t.g_d2[:H], t.g_e2[:H],
                 t.g_d2[H:], t.g_e2[H:])
        return (None, None, None, None) + grads
