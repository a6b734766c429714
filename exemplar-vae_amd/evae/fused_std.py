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
do not take runs on the tiled GEMMs behind the same entry points.  The same arithmetic as the modular path."""
import ctypes as C

import torch

from . import _lib, handoff, ops

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


def _vp(v):
    if v is None:
        return None
    return C.c_void_p(v if isinstance(v, int) else v.data_ptr())


class _Launch:
    """raw launchers over the C ABI on the caller's stream (no autograd, caller-owned outputs)"""

    def __init__(self, device):
        self.lib = _lib.load()
        self.dev = device
        self.st = ops._stream()

    def ws(self, name, nbytes):
        return ops._workspace("std_" + name, nbytes, self.dev)

    def gated_fwd(self, x, M, K, ldx, wh, bh, wg, bg, N, out, s):
        w = self.ws("fwd", self.lib.evae_dense_fwd_workspace_bytes(M, K, N, 1))
        _lib.check(self.lib.evae_gated_dense_fwd(_vp(x), None, M, K, ldx, _vp(wh), _vp(bh), _vp(wg), _vp(bg), N, _vp(out), None,
                                                 _vp(s), _vp(w), w.numel(), self.st), "gated_dense_fwd")

    def linear_fwd(self, x, M, K, ldx, w_, b, N, act, y):
        w = self.ws("fwd", self.lib.evae_dense_fwd_workspace_bytes(M, K, N, 0))
        _lib.check(self.lib.evae_linear_fwd(_vp(x), None, M, K, ldx, _vp(w_), _vp(b), N, act, 0.0, 0.0, _vp(y), None, _vp(w),
                                            w.numel(), self.st), "linear_fwd")

    def bwd_data(self, dy1, w1, dy2, w2, M, N, ldy, K, out_prev, s_prev, out, dg, ldo):
        w = self.ws("dgrad", self.lib.evae_dense_bwd_data_workspace_bytes(M, N, K, 2 if dy2 is not None else 1))
        _lib.check(self.lib.evae_dense_bwd_data(_vp(dy1), _vp(w1), _vp(dy2), _vp(w2), M, N, ldy, K, _vp(out_prev), _vp(s_prev),
                                                _vp(out), _vp(dg), ldo, _vp(w), w.numel(), self.st), "dense_bwd_data")

    def bwd_weights(self, jobs):
        """jobs: (dy, M, N, ldy, x, K, ldx, dw, db).  Those the grouped kernel takes (a contraction over <= 128 rows, widths in
        fours) go out six to a launch; the rest one by one."""
        def ptr(t):
            return t if isinstance(t, int) else t.data_ptr()
        fits = [j[1] <= 128 and all(v % 4 == 0 for v in (j[2], j[3], j[5], j[6])) and all(ptr(t) % 16 == 0 for t in (j[0], j[4], j[7]))
                for j in jobs]
        grouped = [j for j, ok in zip(jobs, fits) if ok]
        rest = [j for j, ok in zip(jobs, fits) if not ok]
        for i in range(0, len(grouped), 6):
            part = grouped[i:i + 6]
            arr = (_lib.WgradJob * len(part))()
            for a, (dy, M, N, ldy, x, K, ldx, dw, db) in zip(arr, part):
                a.dy, a.x, a.dw, a.db = ptr(dy), ptr(x), ptr(dw), ptr(db)
                a.M, a.N, a.K, a.ldy, a.ldx = M, N, K, ldy, ldx
            _lib.check(self.lib.evae_dense_bwd_weight_group(C.cast(arr, C.c_void_p), len(part), self.st), "dense_bwd_weight_group")
        for dy, M, N, ldy, x, K, ldx, dw, db in rest:
            w = self.ws("wgrad", self.lib.evae_dense_bwd_weight_workspace_bytes(M, N, K))
            _lib.check(self.lib.evae_dense_bwd_weight(_vp(dy), M, N, ldy, _vp(x), None, K, ldx, _vp(dw), _vp(db), 0, _vp(w), w.numel(),
                                                      self.st), "dense_bwd_weight")


class VaeStandardLoss(torch.autograd.Function):
    """forward(x [B x D] binarised batch, eps [B x z], beta (float or device scalar), average, *params (PARAM_ORDER))
    -> (loss, RE, KL): [B] each, or the three batch means when `average`."""

    @staticmethod
    def forward(ctx, x, eps, beta, average, *params):
        (wp, bp, w1h, b1h, w1g, b1g, w2h, b2h, w2g, b2g, wm, bm, wl, bl, d1h, e1h, d1g, e1g, d2h, e2h, d2g, e2g) = params
        dev = x.device
        k = _Launch(dev)
        lib = k.lib
        ho = handoff.current() or handoff.StepHandoff()       # what the step's runner says about this step; nothing without one
        x = ops._f32(x)
        eps = ops._f32(eps)
        B, D = x.shape
        H, Z = w1h.shape[0], wm.shape[0]
        f32 = dict(device=dev, dtype=torch.float32)
        beta_dev = beta if torch.is_tensor(beta) else None
        beta_host = 0.0 if beta_dev is not None else float(beta)
        # a gated layer keeps its output and its gate s for the backward (dg = dout * out * (1 - s)); h is never stored
        A1 = torch.empty((B, H), **f32); s1 = torch.empty_like(A1)
        A2 = torch.empty((B, H), **f32); s2 = torch.empty_like(A2)
        z_mean = torch.empty((B, Z), **f32); lv_pre = torch.empty_like(z_mean); logvar = torch.empty_like(z_mean)
        z = torch.empty_like(z_mean)
        logq = torch.empty(B, **f32); logp = torch.empty(B, **f32)
        D1 = torch.empty((B, H), **f32); sd1 = torch.empty_like(D1)
        D2 = torch.empty((B, H), **f32); sd2 = torch.empty_like(D2)
        xmean = torch.empty((B, D), **f32)
        RE = torch.empty(B, **f32)
        # ---- encoder, heads, sample, both densities
        k.gated_fwd(x, B, D, x.stride(0), w1h, b1h, w1g, b1g, H, A1, s1)
        k.gated_fwd(A1, B, H, H, w2h, b2h, w2g, b2g, H, A2, s2)
        one_launch = bool(lib.evae_heads_std_applies(B, H, Z, H))
        if one_launch:
            _lib.check(lib.evae_heads_reparam_std_fwd(_vp(A2), B, H, H, _vp(wm), _vp(bm), _vp(wl), _vp(bl), Z, LV_LO, LV_HI, _vp(eps),
                                                      _vp(z_mean), _vp(lv_pre), _vp(logvar), _vp(z), _vp(logq), _vp(logp), k.st),
                       "heads_reparam_std_fwd")
        else:
            w = k.ws("heads", lib.evae_heads_reparam_fwd_workspace_bytes(B, H, Z))
            _lib.check(lib.evae_heads_reparam_fwd(_vp(A2), B, H, H, _vp(wm), _vp(bm), _vp(wl), _vp(bl), Z, LV_LO, LV_HI, _vp(eps),
                                                  _vp(z_mean), _vp(lv_pre), _vp(logvar), _vp(z), _vp(logq), _vp(w), w.numel(), k.st),
                       "heads_reparam_fwd")
            _lib.check(lib.evae_log_normal_std_fwd(_vp(z), B, Z, _vp(logp), k.st), "log_normal_std_fwd")
        # ---- decode, reconstruct
        k.gated_fwd(z, B, Z, Z, d1h, e1h, d1g, e1g, H, D1, sd1)
        k.gated_fwd(D1, B, H, H, d2h, e2h, d2g, e2g, H, D2, sd2)
        k.linear_fwd(D2, B, H, H, wp, bp, D, ACT_SIGMOID, xmean)
        coef = dpx = None
        if ho.unit_upstream and average:
            # the caller (evae/graph.py) promises loss.backward(ones) on the batch mean and nothing else: RE, the backward's
            # coefficient vectors (-1/B, beta/B, -beta/B) and the sigmoid head's gradient are one launch
            coef = (torch.empty(B, **f32), torch.empty(B, **f32), torch.empty(B, **f32))
            dpx = torch.empty((B, D), **f32)
            _lib.check(lib.evae_bernoulli_unit_step(_vp(x), _vp(xmean), B, D, _vp(beta_dev), beta_host, _vp(RE), _vp(coef[0]),
                                                    _vp(coef[1]), _vp(coef[2]), _vp(dpx), k.st), "bernoulli_unit_step")
        else:
            _lib.check(lib.evae_bernoulli_ll_fwd(_vp(x), _vp(xmean), B, D, _vp(RE), k.st), "bernoulli_ll_fwd")
        loss = torch.empty(B, **f32); KL = torch.empty(B, **f32)
        means = torch.empty(3, **f32) if average else None
        _lib.check(lib.evae_elbo_assemble(_vp(logp), _vp(RE), _vp(logq), _vp(beta_dev), beta_host, B, _vp(loss), _vp(KL), _vp(means),
                                          k.st), "elbo_assemble")
        ctx.coef, ctx.dpx = coef, dpx
        ctx.one_launch = one_launch
        ctx.beta = beta
        ctx.k_dev = dev
        ctx.bufs = (x, eps, A1, s1, A2, s2, z_mean, lv_pre, logvar, z, D1, sd1, D2, sd2, xmean)
        ctx.set_materialize_grads(False)       # unused outputs (RE, KL) then arrive as None, not as zero-filled tensors
        ctx.save_for_backward(*params)
        if average:
            l, r, kl = means.unbind(0)
            return l, r, kl
        return loss, RE, KL

    @staticmethod
    def backward(ctx, dloss, dRE, dKL):
        params = ctx.saved_tensors
        (wp, bp, w1h, b1h, w1g, b1g, w2h, b2h, w2g, b2g, wm, bm, wl, bl, d1h, e1h, d1g, e1g, d2h, e2h, d2g, e2g) = params
        (x, eps, A1, s1, A2, s2, z_mean, lv_pre, logvar, z, D1, sd1, D2, sd2, xmean) = ctx.bufs
        dev = ctx.k_dev
        k = _Launch(dev)
        lib = k.lib
        B, D = x.shape
        H, Z = w1h.shape[0], wm.shape[0]
        f32 = dict(device=dev, dtype=torch.float32)
        beta = ctx.beta
        beta_dev = beta if torch.is_tensor(beta) else None
        # upstream gradients are per-row vectors (average=False) or scalars of the batch means (average=True)
        if ctx.coef is not None and dRE is None and dKL is None and dloss is not None and dloss.numel() == 1:
            cRE, cKL, neg_cKL = ctx.coef          # written by the forward pass under the caller's unit-upstream promise
            dpx = ctx.dpx
        else:
            cRE = torch.empty(B, **f32); cKL = torch.empty(B, **f32); neg_cKL = torch.empty(B, **f32)
            gl = None if dloss is None else ops._f32(dloss)
            gr = None if dRE is None else ops._f32(dRE)
            gk = None if dKL is None else ops._f32(dKL)
            _lib.check(lib.evae_elbo_bwd(_vp(gl), 0 if gl is None else gl.numel(), _vp(gr), 0 if gr is None else gr.numel(),
                                         _vp(gk), 0 if gk is None else gk.numel(), _vp(beta_dev),
                                         0.0 if beta_dev is not None else float(beta), B, _vp(cRE), _vp(cKL), _vp(neg_cKL), k.st),
                       "elbo_bwd")
            # through the Bernoulli log-likelihood and the sigmoid head at once
            dpx = torch.empty((B, D), **f32)
            _lib.check(lib.evae_bernoulli_sigmoid_bwd(_vp(x), _vp(xmean), _vp(cRE), B, D, _vp(dpx), k.st), "bernoulli_sigmoid_bwd")
        # every gated layer's backward uses the merged [dh | dg] buffer: one weight-gradient job per layer, and the gate derivative of
        # the layer below is applied in the epilogue of the data gradient
        dp2 = torch.empty((B, 2 * H), **f32)
        dp1 = torch.empty((B, 2 * H), **f32)
        dz = torch.empty((B, Z), **f32)
        dq2 = torch.empty((B, 2 * H), **f32)
        dq1 = torch.empty((B, 2 * H), **f32)
        g_wp = torch.empty((D, H), **f32); g_bp = torch.empty(D, **f32)
        g_d2 = torch.empty((2 * H, H), **f32); g_e2 = torch.empty(2 * H, **f32)
        g_d1 = torch.empty((2 * H, Z), **f32); g_e1 = torch.empty(2 * H, **f32)
        g_hd = torch.empty((2 * Z, H), **f32); g_hb = torch.empty(2 * Z, **f32)         # [mean head | log-variance head]
        g_w2 = torch.empty((2 * H, H), **f32); g_b2 = torch.empty(2 * H, **f32)
        g_w1 = torch.empty((2 * H, D), **f32); g_b1 = torch.empty(2 * H, **f32)
        # ---- down the decoder
        k.bwd_data(dpx, wp, None, None, B, D, D, H, D2, sd2, dp2, dp2.data_ptr() + 4 * H, 2 * H)
        k.bwd_data(dp2, d2h, dp2.data_ptr() + 4 * H, d2g, B, H, 2 * H, H, D1, sd1, dp1, dp1.data_ptr() + 4 * H, 2 * H)
        k.bwd_data(dp1, d1h, dp1.data_ptr() + 4 * H, d1g, B, H, 2 * H, Z, None, None, dz, None, Z)
        # ---- the latent block: reparameterisation + log q + Hardtanh + the prior's share of dz, and the heads' data gradient
        if ctx.one_launch:
            dhd = torch.empty((B, 2 * Z), **f32)                                         # [dmu | dlv_pre]
            _lib.check(lib.evae_heads_std_bwd(_vp(z_mean), _vp(logvar), _vp(lv_pre), _vp(eps), _vp(z), _vp(dz), _vp(cKL), _vp(neg_cKL),
                                              LV_LO, LV_HI, B, Z, _vp(wm), _vp(wl), H, _vp(A2), _vp(s2), _vp(dhd),
                                              _vp(dhd.data_ptr() + 4 * Z), 2 * Z, _vp(dq2), _vp(dq2.data_ptr() + 4 * H), 2 * H, k.st),
                       "heads_std_bwd")
            head_jobs = [(dhd, B, 2 * Z, 2 * Z, A2, H, H, g_hd, g_hb)]
        else:
            dzp = torch.empty((B, Z), **f32); dmu = torch.empty((B, Z), **f32); dlvp = torch.empty((B, Z), **f32)
            _lib.check(lib.evae_log_normal_std_bwd(_vp(z), _vp(neg_cKL), B, Z, _vp(dzp), k.st), "log_normal_std_bwd")
            _lib.check(lib.evae_reparam_logq_bwd_hardtanh(_vp(z_mean), _vp(logvar), _vp(eps), _vp(z), _vp(dz), _vp(dzp), _vp(cKL),
                                                          _vp(lv_pre), LV_LO, LV_HI, B, Z, _vp(dmu), _vp(dlvp), k.st), "reparam_logq_bwd")
            k.bwd_data(dmu, wm, dlvp, wl, B, Z, Z, H, A2, s2, dq2, dq2.data_ptr() + 4 * H, 2 * H)
            head_jobs = [(dmu, B, Z, Z, A2, H, H, g_hd[:Z], g_hb[:Z]), (dlvp, B, Z, Z, A2, H, H, g_hd[Z:], g_hb[Z:])]
        # ---- encoder layer 2's data gradient (layer 1's gate derivative in its epilogue), then every weight gradient: leaves
        k.bwd_data(dq2, w2h, dq2.data_ptr() + 4 * H, w2g, B, H, 2 * H, H, A1, s1, dq1, dq1.data_ptr() + 4 * H, 2 * H)
        k.bwd_weights([(dpx, B, D, D, D2, H, H, g_wp, g_bp), (dp2, B, 2 * H, 2 * H, D1, H, H, g_d2, g_e2),
                       (dp1, B, 2 * H, 2 * H, z, Z, Z, g_d1, g_e1)] + head_jobs +
                      [(dq2, B, 2 * H, 2 * H, A1, H, H, g_w2, g_b2), (dq1, B, 2 * H, 2 * H, x, D, x.stride(0), g_w1, g_b1)])
        ctx.bufs = None
        grads = (g_wp, g_bp, g_w1[:H], g_b1[:H], g_w1[H:], g_b1[H:], g_w2[:H], g_b2[:H], g_w2[H:], g_b2[H:],
                 g_hd[:Z], g_hb[:Z], g_hd[Z:], g_hb[Z:], g_d1[:H], g_e1[:H], g_d1[H:], g_e1[H:], g_d2[:H], g_e2[:H], g_d2[H:], g_e2[H:])
        return (None, None, None, None) + grads
