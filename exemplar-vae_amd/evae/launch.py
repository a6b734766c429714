"""The raw-launch layer of the fused training steps (evae/fused_vae.py, evae/fused_std.py) and of the dense autograd operators
of evae/ops.py: the launcher over the dense entry points of the C ABI, the two job-table fillers, the beta pair (the one pointer
conversion, vp, is evae/_lib.py's).  No autograd, caller-owned outputs.  The same Launcher also carries the launchers of the
latent-analysis entry points (tsne_*, nn_rank, pca_*, kmeans_*, cluster_*, silhouette_samples, gmm_*, agg_lse, kernel_row_sums, ordered_sum, sym_congruence, logreg_*), one method per entry.

The fused steps are stage functions over one per-step state object; the modular operators (GatedDenseFn, LinearFn, the heads'
backward, the deferred weight gradients) are torch.autograd.Functions that build a Launcher where they run.  Every change to
either keeps four invariants; they are held by tests/test_gpu_step_trace.py (what a step or an operator issues, record for record,
against the recorded goldens g28 and g29), not by a reader's eye:

* ISSUE ORDER IS BEHAVIOUR.  The order launches, event records and stream waits are issued in is the order the captured hipGraph
  starts them in: the leaves of fused_vae's backward pass issued elsewhere replayed at 0.82-1.2 ms against 0.66.  Stages are
  called in that order; a stage that is interleaved with another stays interleaved.
* THE STREAM CURRENT AT EACH ALLOCATION IS BEHAVIOUR.  The caching allocator pools per stream: an allocation-order change once
  handed a live scratch buffer of the prior's launch to the other stream.  Every torch.empty keeps its place relative to the
  `with torch.cuda.stream(side)` blocks and to its neighbours.
* LIFETIMES DO NOT GET SHORTER.  Launches on the other stream read buffers through raw pointers, with no record_stream.  A stage
  keeps no tensor of its own: what it allocates goes on the step state -- a pass's temporaries on st.fwd / st.bwd, cleared where
  that pass returns; what the backward pass needs on the state itself, dropped where the backward pass returns.
* MODULE-LEVEL SWITCHES KEEP THEIR NAMES AND THEIR READ TIME: import-time constants stay import-time, per-call reads
  (node_merge(), the os.environ reads inside the passes) stay per-call.  evae/graph.py and tools/ read them by name.

In evae/ops.py the same four bind the dense operators: the order of an operator's launches, size queries and allocations, the
stream current at each, the tensors a backward keeps until it returns, and the module attributes tests and bench.py assign to
(ops.PROBE, ops._DEFER, ops._ws, ...: they stay on evae.ops and are read there at call time).  Two more come with them: WHICH
launches ops.probed brackets, and under which name, is behaviour (bench.py builds its roofline from those records) -- hence the
*_call methods below, the launch without the bracket; and no entry point is kept bound across calls (`self.lib.evae_x` is looked
up at each launch): the recorder and _lib.count_calls patch the names on the loaded library object."""
import ctypes as C
import os

import torch

from . import _lib, ops
from ._lib import vp


def beta_args(beta):
    """(beta_dev, beta_host) as the kernels take them: the device scalar and 0.0, or None and the float"""
    if torch.is_tensor(beta):
        return beta, 0.0
    return None, float(beta)


def wgrad_jobs(jobs):
    """(dy, M, N, ldy, x, K, ldx, dw, db[, accumulate]) per job -> (evae_wgrad_job_t array as c_void_p, count, the array: keep it
    until the launch is issued).  accumulate = 1: dw += the product, db += its column sums (default 0).  Which jobs share a
    launch is the caller's rule."""
    arr = (_lib.WgradJob * len(jobs))()
    for a, (dy, M, N, ldy, x, K, ldx, dw, db, *acc) in zip(arr, jobs):
        a.dy, a.x, a.dw, a.db = vp(dy), vp(x), vp(dw), vp(db)
        a.M, a.N, a.K, a.ldy, a.ldx = M, N, K, ldy, ldx
        a.accumulate = acc[0] if acc else 0
    return C.cast(arr, C.c_void_p), len(jobs), arr


def wgrad_finish_jobs(jobs):
    """(byte_rows, M, N, K, ldy, ldx, x_scale, dw, db, workspace) per job -> the same for evae_wgrad_finish_job_t"""
    arr = (_lib.WgradFinishJob * len(jobs))()
    for a, (byte_rows, M, N, K, ldy, ldx, x_scale, dw, db, ws) in zip(arr, jobs):
        a.byte_rows, a.M, a.N, a.K, a.ldy, a.ldx = byte_rows, M, N, K, ldy, ldx
        a.x_scale, a.dw, a.db, a.ws, a.ws_bytes = x_scale, vp(dw), vp(db), vp(ws), ws.numel()
    return C.cast(arr, C.c_void_p), len(jobs), arr


class Launcher:
    """Thin raw launchers over the C ABI (no autograd, caller-owned outputs)."""

    def __init__(self, device, stream=None, prefix="", suffix="", pipes=True):
        """Launches go to `stream` (default: the current one) and take their split-K workspaces from buffers named
        prefix + name + suffix, so that two launchers never share scratch memory.  The names are behaviour: a captured graph has
        the addresses baked in and ops._workspace keys on the name.  pipes=False: no evae_gemm_x6_applies query per launch for
        the roofline probe's pipe label -- for steps whose launches the probe never records."""
        self.lib = _lib.load()
        self.dev = device
        self.st = ops._stream() if stream is None else C.c_void_p(stream.cuda_stream)
        self.pfx, self.sfx, self.pipes = prefix, suffix, pipes

    def ws(self, name, nbytes):
        return ops._workspace(self.pfx + name + self.sfx, nbytes, self.dev)

    _side = {}

    def side_stream(self, one_stream=False):
        """Second stream for the decoder chain of the batch rows: it only meets the exemplar-prior chain at the ELBO (forward)
        and at dz (backward), so the two chains of small launches run side by side, captured as parallel branches of the
        step's hipGraph.  Collectives of the sharded prior stay on the main stream.  one_stream: the caller's own stream."""
        if one_stream:
            return torch.cuda.current_stream(self.dev)
        key = self.dev.index if self.dev.index is not None else torch.cuda.current_device()
        st = Launcher._side.get(key)
        if st is None:
            st = Launcher._side[key] = torch.cuda.Stream(device=self.dev, priority=int(os.environ.get("EVAE_SIDE_PRIORITY", "-1")))
        return st

    def _pipe(self, M, N, gated, flops, fits=True):
        return ops.gemm_pipe(M, N, gated, flops) if (fits and self.pipes) else (None, "fp32-mfma")

    # <name>_call: the launch, its workspace taken now, as a closure -- for the callers whose launch ops.probed does not bracket
    # (the operators of evae/ops.py outside GatedDenseFn.forward); <name>: the same launch inside its bracket

    def gated_fwd_call(self, x, rows, M, K, ldx, wh, bh, wg, bg, N, out, h, s):
        w = self.ws("fwd", self.lib.evae_dense_fwd_workspace_bytes(M, K, N, 1))
        return lambda: _lib.check(self.lib.evae_gated_dense_fwd(vp(x), vp(rows), M, K, ldx, vp(wh), vp(bh), vp(wg), vp(bg), N, vp(out),
                                                                vp(h), vp(s), vp(w), w.numel(), self.st), "gated_fwd")

    def gated_fwd(self, x, rows, M, K, ldx, wh, bh, wg, bg, N, out, h, s):
        call = self.gated_fwd_call(x, rows, M, K, ldx, wh, bh, wg, bg, N, out, h, s)
        ex_, pipe_ = self._pipe(M, N, True, 2.0 * M * K * 2 * N, rows is None)
        ops.probed("gated_dense_fwd M=%d K=%d N=%d%s" % (M, K, N, " (row gather)" if rows is not None else ""), 2.0 * M * K * 2 * N,
                   call, executed=ex_, pipe=pipe_)

    def linear_fwd(self, x, M, K, ldx, w_, b, N, act, lo, hi, y, pre, rows=None):
        w = self.ws("fwd", self.lib.evae_dense_fwd_workspace_bytes(M, K, N, 0))
        _lib.check(self.lib.evae_linear_fwd(vp(x), vp(rows), M, K, ldx, vp(w_), vp(b), N, act, lo, hi, vp(y), vp(pre),
                                            vp(w), w.numel(), self.st), "linear_fwd")

    def bwd_data_call(self, dy1, w1, dy2, w2, M, N, ldy, K, out_prev, s_prev, out, dg, ldo, wT=None):
        """dx [M x K] = dy1 W1 (+ dy2 W2); with out_prev / s_prev (forward output and gate of the layer below) the gate derivative
        of that layer is applied in the epilogue and (dh, dg) are written instead.  wT: the transposed weights prepared by the
        step's head launch, or None (then evae_dense_bwd_data_wt IS evae_dense_bwd_data: both are dense_bwd_data_core,
        csrc/evae_dense.hip)"""
        w = self.ws("dgrad", self.lib.evae_dense_bwd_data_workspace_bytes(M, N, K, 2 if dy2 is not None else 1))
        return lambda: _lib.check(self.lib.evae_dense_bwd_data_wt(vp(dy1), vp(w1), vp(dy2), vp(w2), M, N, ldy, K, vp(out_prev),
                                                                  vp(s_prev), vp(out), vp(dg), ldo, vp(wT), vp(w), w.numel(),
                                                                  self.st), "bwd_data")

    def bwd_data(self, dy1, w1, dy2, w2, M, N, ldy, K, out_prev, s_prev, out, dg, ldo, wT=None):
        call = self.bwd_data_call(dy1, w1, dy2, w2, M, N, ldy, K, out_prev, s_prev, out, dg, ldo, wT)
        fl_ = 2.0 * M * N * K * (2 if dy2 is not None else 1)
        ex_, pipe_ = self._pipe(M, K, False, fl_, N % 4 == 0 and ldy % 4 == 0)
        ops.probed("dense_bwd_data M=%d N=%d%s K=%d%s" % (M, N, "+%d" % N if dy2 is not None else "", K,
                                                          " (gate-backward epilogue)" if out_prev is not None else ""), fl_,
                   call, executed=ex_, pipe=pipe_)

    def gated_bwd(self, dout, ldd, gout, s, M, N, wh, wg, K, dpre, dx):
        """a gated layer's gate derivative and data gradient as one entry point (one launch for batch-sized row counts): fills
        dpre = [dh | dg] [M x 2N] and dx = dh Wh + dg Wg [M x K]"""
        w = self.ws("dgrad", self.lib.evae_dense_bwd_data_workspace_bytes(M, N, K, 2))
        _lib.check(self.lib.evae_gated_dense_bwd(vp(dout), ldd, vp(gout), vp(s), M, N, vp(wh), vp(wg), K, vp(dpre), 2 * N,
                                                 vp(dx), K, vp(w), w.numel(), self.st), "gated_bwd")

    def bwd_weight_call(self, dy, M, N, ldy, x, rows, K, ldx, dw, db, ws_name="wgrad"):
        """dw [N x K] = dy^T x(rows), db [N] = column sums of dy: the split-K GEMM and its finish"""
        w = self.ws(ws_name, self.lib.evae_dense_bwd_weight_workspace_bytes(M, N, K))
        return lambda: _lib.check(self.lib.evae_dense_bwd_weight(vp(dy), M, N, ldy, vp(x), vp(rows), K, ldx, vp(dw), vp(db), 0,
                                                                 vp(w), w.numel(), self.st), "bwd_weight")

    def bwd_weight(self, dy, M, N, ldy, x, rows, K, ldx, dw, db, phase=0, ws_name="wgrad", finish_on=None):
        """phase 1 / 2: the split-K GEMM and its finish as separate calls (finish_on = the launcher whose stream runs it)"""
        if phase == 0:
            # (a narrow output over many rows -- the heads' [40 x 300] over all C + B rows -- streams its operands once: an HBM entry)
            ops.probed("dense_bwd_weight M=%d N=%d K=%d (+db, split-K GEMM + finish)" % (M, N, K), 2.0 * M * N * K,
                       hbm_bytes=(4.0 * M * (N + K)) if (N <= 64 and M >= 2048 and rows is None) else None,
                       fn=self.bwd_weight_call(dy, M, N, ldy, x, rows, K, ldx, dw, db, ws_name))
        else:
            w = self.ws(ws_name, self.lib.evae_dense_bwd_weight_workspace_bytes(M, N, K))
            st = self.st if finish_on is None else finish_on.st
            call = lambda: _lib.check(self.lib.evae_dense_bwd_weight_phased(vp(dy), M, N, ldy, vp(x), vp(rows), K, ldx, vp(dw),
                                                                            vp(db), 0, vp(w), w.numel(), phase, st), "bwd_weight_phased")
            if phase == 1:
                ops.probed("dense_bwd_weight M=%d N=%d K=%d (+db, split-K GEMM; its planes are summed by the step's last grouped launch)"
                           % (M, N, K), 2.0 * M * N * K, call)
            else:
                call()

    # exact t-SNE (csrc/evae_tsne.hip): no workspaces, every buffer is the caller's

    def tsne_affinities(self, d2, N, perplexity, steps, beta, P):
        """d2 [N x N] squared distances -> beta [N], joint P [N x N] (P may be d2): the row search and the symmetrising launch"""
        _lib.check(self.lib.evae_tsne_affinities(vp(d2), N, float(perplexity), int(steps), vp(beta), vp(P), self.st), "tsne_affinities")

    def tsne_forces(self, P, Y, N, exaggeration, want_kl, part):
        _lib.check(self.lib.evae_tsne_forces(vp(P), vp(Y), N, float(exaggeration), int(bool(want_kl)), vp(part), self.st), "tsne_forces")

    def tsne_update(self, part, N, want_kl, momentum, lr, Y, velocity, gains, grad, stats):
        _lib.check(self.lib.evae_tsne_update(vp(part), N, int(bool(want_kl)), float(momentum), float(lr), vp(Y), vp(velocity),
                                             vp(gains), vp(grad), vp(stats), self.st), "tsne_update")

    def tsne_stats(self, part, N, want_kl, stats):
        _lib.check(self.lib.evae_tsne_stats(vp(part), N, int(bool(want_kl)), vp(stats), self.st), "tsne_stats")

    # t-SNE on sparse affinities (csrc/evae_tsne_nn.hip): the two workspaces are the caller's too
    def tsne_knn(self, z, N, zd, k, strip_rows, idx, d2, ws):
        _lib.check(self.lib.evae_tsne_knn(vp(z), N, zd, int(k), int(strip_rows), vp(idx), vp(d2), vp(ws), ws.numel(), self.st), "tsne_knn")

    def nn_rank(self, z, N, zd, nbr, k, strip_rows, rank, row_sums, ws):
        """csrc/evae_nn_rank.hip: the strip workspace is the caller's, as tsne_knn's"""
        _lib.check(self.lib.evae_nn_rank(vp(z), N, zd, vp(nbr), int(k), int(strip_rows), vp(rank), vp(row_sums), vp(ws), ws.numel(),
                                         self.st), "nn_rank")

    def ball_count(self, q, B, c, N, d, col_radius, row_radius, strip_rows, col_hits, row_hits, nn_idx, nn_d2, ws):
        """csrc/evae_ball_count.hip: None switches a radius and its count, or a half of the nearest pair, off"""
        _lib.check(self.lib.evae_ball_count(vp(q), B, vp(c), N, d, vp(col_radius), vp(row_radius), int(strip_rows), vp(col_hits),
                                            vp(row_hits), vp(nn_idx), vp(nn_d2), vp(ws), ws.numel(), self.st), "ball_count")

    def tsne_nn_conditionals(self, d2, N, k, perplexity, steps, beta, cond):
        _lib.check(self.lib.evae_tsne_nn_conditionals(vp(d2), N, int(k), float(perplexity), int(steps), vp(beta), vp(cond), self.st),
                   "tsne_nn_conditionals")

    def tsne_nn_joint(self, cond, ia, ib, nnz, N, val):
        _lib.check(self.lib.evae_tsne_nn_joint(vp(cond), cond.numel(), vp(ia), vp(ib), int(nnz), N, vp(val), self.st), "tsne_nn_joint")

    def tsne_nn_forces(self, row_ptr, col, val, Y, N, exaggeration, want_kl, part, ws):
        _lib.check(self.lib.evae_tsne_nn_forces(vp(row_ptr), vp(col), vp(val), vp(Y), N, float(exaggeration), int(bool(want_kl)),
                                                vp(part), vp(ws), ws.numel(), self.st), "tsne_nn_forces")

    # PCA in fp64 (csrc/evae_pca.hip): the workspaces are the caller's
    def pca_moments(self, x, N, d, mean, cov, ws):
        _lib.check(self.lib.evae_pca_moments(vp(x), N, d, vp(mean), vp(cov), vp(ws), ws.numel(), self.st), "pca_moments")

    def pca_eigh(self, cov, d, evals, evecs, info, ws):
        """ws: None where evae_pca_eigh_workspace_bytes(d) is 0 (the matrices sit in LDS)"""
        _lib.check(self.lib.evae_pca_eigh(vp(cov), d, vp(evals), vp(evecs), vp(info), vp(ws), 0 if ws is None else ws.numel(),
                                          self.st), "pca_eigh")

    def pca_project(self, x, N, d, mean, W, k, scale, out):
        _lib.check(self.lib.evae_pca_project(vp(x), N, d, vp(mean), vp(W), int(k), float(scale), vp(out), self.st), "pca_project")

    def pca_reconstruct(self, y, N, k, mean, W, d, out):
        _lib.check(self.lib.evae_pca_reconstruct(vp(y), N, int(k), vp(mean), vp(W), d, vp(out), self.st), "pca_reconstruct")

    # k-means and clustering scores in fp64 (csrc/evae_kmeans.hip): every buffer and workspace is the caller's
    def kmeans_assign(self, x, N, d, centres, K, labels, d2):
        _lib.check(self.lib.evae_kmeans_assign(vp(x), N, d, vp(centres), int(K), vp(labels), vp(d2), self.st), "kmeans_assign")

    def kmeans_transform(self, x, N, d, centres, K, out):
        _lib.check(self.lib.evae_kmeans_transform(vp(x), N, d, vp(centres), int(K), vp(out), self.st), "kmeans_transform")

    def kmeans_update(self, x, N, d, labels, K, order, start, sums, ws):
        _lib.check(self.lib.evae_kmeans_update(vp(x), N, d, vp(labels), int(K), vp(order), vp(start), vp(sums), vp(ws), ws.numel(),
                                               self.st), "kmeans_update")

    def kmeans_step(self, x, N, d, K, centres, labels, d2, order, start, tol_abs, state, ws):
        _lib.check(self.lib.evae_kmeans_step(vp(x), N, d, int(K), vp(centres), vp(labels), vp(d2), vp(order), vp(start),
                                             float(tol_abs), vp(state), vp(ws), ws.numel(), self.st), "kmeans_step")

    def kmeans_seed(self, x, N, d, K, u, idx, centres, ws):
        _lib.check(self.lib.evae_kmeans_seed(vp(x), N, d, int(K), vp(u), vp(idx), vp(centres), vp(ws), ws.numel(), self.st),
                   "kmeans_seed")

    def kmeans_inertia(self, d2, N, out, ws):
        _lib.check(self.lib.evae_kmeans_inertia(vp(d2), N, vp(out), vp(ws), ws.numel(), self.st), "kmeans_inertia")

    # Gaussian mixture in fp64 (csrc/evae_gmm.hip): every buffer and workspace is the caller's
    def gmm_estep(self, x, N, d, K, ctype, params, log_resp, logp, mean_logp, ws):
        _lib.check(self.lib.evae_gmm_estep(vp(x), N, d, int(K), int(ctype), vp(params), vp(log_resp), vp(logp), vp(mean_logp),
                                           vp(ws), ws.numel(), self.st), "gmm_estep")

    def gmm_mstep(self, x, N, d, K, ctype, log_resp, labels, reg_covar, params, state, ws):
        _lib.check(self.lib.evae_gmm_mstep(vp(x), N, d, int(K), int(ctype), vp(log_resp), vp(labels), float(reg_covar), vp(params),
                                           vp(state), vp(ws), ws.numel(), self.st), "gmm_mstep")

    def gmm_step(self, x, N, d, K, ctype, params, log_resp, logp, reg_covar, tol, state, ws):
        _lib.check(self.lib.evae_gmm_step(vp(x), N, d, int(K), int(ctype), vp(params), vp(log_resp), vp(logp), float(reg_covar),
                                          float(tol), vp(state), vp(ws), ws.numel(), self.st), "gmm_step")

    def gmm_prepare(self, params, d, K, ctype):
        _lib.check(self.lib.evae_gmm_prepare(vp(params), d, int(K), int(ctype), self.st), "gmm_prepare")

    def gmm_argmax(self, log_resp, N, K, labels):
        _lib.check(self.lib.evae_gmm_argmax(vp(log_resp), N, int(K), vp(labels), self.st), "gmm_argmax")

    def gmm_sample(self, params, d, K, ctype, comp, eps, n, z):
        _lib.check(self.lib.evae_gmm_sample(vp(params), d, int(K), int(ctype), vp(comp), vp(eps), n, vp(z), self.st), "gmm_sample")

    def agg_lse(self, z, B, mean, log_var, N, d, rows, log_q, log_qd, log_cond, ws):
        """csrc/evae_agg_lse.hip: None switches an output off (rows may be None when log_cond is); the workspace is the caller's"""
        _lib.check(self.lib.evae_agg_lse(vp(z), B, vp(mean), vp(log_var), N, d, vp(rows), vp(log_q), vp(log_qd), vp(log_cond),
                                         vp(ws), ws.numel(), self.st), "agg_lse")

    # kernel sums in fp64 (csrc/evae_kernel_sum.hip): outputs and the workspace are the caller's
    def kernel_row_sums(self, q, B, c, N, d, kind, gamma, coef0, degree, skip_self, row_sum):
        _lib.check(self.lib.evae_kernel_row_sums(vp(q), B, vp(c), N, d, int(kind), float(gamma), float(coef0), int(degree),
                                                 int(bool(skip_self)), vp(row_sum), self.st), "kernel_row_sums")

    def ordered_sum(self, x, n, out):
        _lib.check(self.lib.evae_ordered_sum(vp(x), n, vp(out), self.st), "ordered_sum")

    def sym_congruence(self, A, S, out, d, ws):
        _lib.check(self.lib.evae_sym_congruence(vp(A), vp(S), vp(out), d, vp(ws), ws.numel(), self.st), "sym_congruence")

    # linear probe in fp64 (csrc/evae_logreg.hip): every buffer and workspace is the caller's
    def logreg_logits(self, x, N, d, W, K, fit_intercept, out):
        _lib.check(self.lib.evae_logreg_logits(vp(x), N, d, vp(W), int(K), int(fit_intercept), vp(out), self.st), "logreg_logits")

    def logreg_line(self, Z, ZD, y, N, d, K, fit_intercept, W, solver, history, lam, line_steps, state, ring, ws):
        _lib.check(self.lib.evae_logreg_line(vp(Z), vp(ZD), vp(y), N, d, int(K), int(fit_intercept), vp(W), vp(solver), int(history),
                                             float(lam), int(line_steps), vp(state), vp(ring), 0 if ring is None else ring.numel(),
                                             vp(ws), ws.numel(), self.st), "logreg_line")

    def logreg_grad(self, x, y, N, d, K, fit_intercept, line_steps, Z, ZD, state, ws):
        _lib.check(self.lib.evae_logreg_grad(vp(x), vp(y), N, d, int(K), int(fit_intercept), int(line_steps), vp(Z), vp(ZD), vp(state),
                                             vp(ws), ws.numel(), self.st), "logreg_grad")

    def logreg_finish(self, N, d, K, fit_intercept, line_steps, W, solver, history, lam, tol, state, ws):
        _lib.check(self.lib.evae_logreg_finish(N, d, int(K), int(fit_intercept), int(line_steps), vp(W), vp(solver), int(history),
                                               float(lam), float(tol), vp(state), vp(ws), ws.numel(), self.st), "logreg_finish")

    def logreg_direction(self, solver, d, K, fit_intercept, history, state):
        _lib.check(self.lib.evae_logreg_direction(vp(solver), d, int(K), int(fit_intercept), int(history), vp(state), self.st),
                   "logreg_direction")

    def logreg_begin(self, x, y, N, d, K, fit_intercept, W, Z, ZD, solver, history, lam, tol, line_steps, state, ws):
        _lib.check(self.lib.evae_logreg_begin(vp(x), vp(y), N, d, int(K), int(fit_intercept), vp(W), vp(Z), vp(ZD), vp(solver),
                                              int(history), float(lam), float(tol), int(line_steps), vp(state), vp(ws), ws.numel(),
                                              self.st), "logreg_begin")

    def logreg_step(self, x, y, N, d, K, fit_intercept, W, Z, ZD, solver, history, lam, tol, line_steps, state, ring, ws):
        _lib.check(self.lib.evae_logreg_step(vp(x), vp(y), N, d, int(K), int(fit_intercept), vp(W), vp(Z), vp(ZD), vp(solver),
                                             int(history), float(lam), float(tol), int(line_steps), vp(state), vp(ring),
                                             0 if ring is None else ring.numel(), vp(ws), ws.numel(), self.st), "logreg_step")

    def logreg_softmax(self, Z, N, K, logp, labels):
        _lib.check(self.lib.evae_logreg_softmax(vp(Z), N, int(K), vp(logp), vp(labels), self.st), "logreg_softmax")

    def cluster_contingency(self, a, Ka, b, Kb, N, table):
        _lib.check(self.lib.evae_cluster_contingency(vp(a), int(Ka), vp(b), int(Kb), N, vp(table), self.st), "cluster_contingency")

    def cluster_scores(self, table, Ka, Kb, out):
        _lib.check(self.lib.evae_cluster_scores(vp(table), int(Ka), int(Kb), vp(out), self.st), "cluster_scores")

    def silhouette_samples(self, x, N, d, order, start, K, out, ws, strip_rows):
        _lib.check(self.lib.evae_silhouette_samples(vp(x), N, d, vp(order), vp(start), int(K), vp(out), vp(ws), ws.numel(),
                                                    int(strip_rows), self.st), "silhouette_samples")

    def bwd_weight_group(self, jobs):
        """ONE launch for up to six thin weight gradients (evae_dense_bwd_weight_group; jobs as wgrad_jobs takes them)"""
        arr, n, _keep = wgrad_jobs(jobs)
        _lib.check(self.lib.evae_dense_bwd_weight_group(arr, n, self.st), "bwd_weight_group")
