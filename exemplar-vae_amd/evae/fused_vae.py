"""One-node autograd implementation of the `vae` exact-prior training loss (the body of
models/BaseModel.py:65-77 + AbsModel.py:13-19,44-49 + BaseModel.py:243-248 in the reference).

Same arithmetic as the modular path (utils.nn.GatedDense, evae.ops.PriorLogP, ...), arranged for the
hardware:

* the B batch rows ride along the C exemplar rows through the encoder: the binarised batch sits in staging
  rows behind the HBM-resident dataset (the captured step gathers it there itself, evae/graph.py) and ONE
  row-gathered GEMM per encoder layer serves all C + B rows (forward and weight gradient), so the 100-row batch
  path costs three thin decoder layers instead of a second pass over every encoder layer;
* every GatedDense backward uses the merged [dh | dg] buffer (one weight-gradient GEMM per layer) and
  the gate derivative of the layer below is applied in the epilogue of the data-gradient GEMM;
* one autograd node instead of ~25: 61 kernel launches per step and no per-op autograd bookkeeping;
* two streams scheduled by hand: the exemplar-prior chain (with its collectives when sharded) and the big
  GEMMs on the main stream, the decoder chain of the batch rows and every weight gradient nobody waits for on
  the side stream (DESIGN.md section 4 for what was measured to arrive at this order of issue).

With torch.distributed active and shard=True the exemplar rows are this rank's shard: the per-row
partials (max, sumexp, nmask) are all-gathered and merged, dz / dlogvar are sum-all-reduced and
dcentres is scaled by the world size (see evae/shard.py for why).

Both passes are a sequence of stage functions over one per-step state object (ctx.step); evae/launch.py states the four
invariants every change to them has to keep (issue order, the stream current at each allocation, lifetimes, the switches)."""
import ctypes as C
import math
import os
from types import SimpleNamespace

import torch
import torch.distributed as dist

from . import _lib, handoff, ops, shard
from .fused_std import decoder_dgrads, decoder_fwd, named, upstream_coefs
from .launch import Launcher, beta_args, vp, wgrad_finish_jobs

ACT_NONE, ACT_SIGMOID, ACT_HARDTANH = ops.ACT_NONE, ops.ACT_SIGMOID, ops.ACT_HARDTANH

# Module state (none of it belongs to one step) and what invalidates each entry:
#   _STAGE_GEN    dataset buffer address -> generation of its staging rows.  Every fused forward bumps it (it overwrites the rows a
#                 pending backward would gather its batch from): a backward whose forward was not the last one to stage refuses
#   _XT_GEN       workspace address -> generation of the transposed byte rows a forward pass left there.  Every gather bumps it; a
#                 backward that finds another generation (another step used the workspace since) redoes the gather
#   _ZEROED       "wgrad_u8" -> (workspace address, Mp, H, D) whose image region was last zero-filled; another key zero-fills
#   _P6_READY     image buffer address -> (bytes, Mp, H) it was zero-filled (and its ones row written) for; another key refills
#   _ONES         device -> a one-element tensor holding 1.0 (the unit upstream gradient of a captured step); never stale
#   _APPROX_ROWS  (device, slots, batch, dataset rows) -> the approximate-prior step's gather list: a static tail, a head every step rewrites
_STAGE_GEN, _XT_GEN, _ZEROED, _P6_READY, _ONES, _APPROX_ROWS = {}, {}, {}, {}, {}, {}
# r06: element-wise launches of the batch rows' chain merged into their neighbours (a replayed graph node costs the host 3.6 us):
# bit 0 the log-variance row's broadcast rides in the heads' launch; bit 1 RE + the unit coefficients + the sigmoid head's gradient
# are one launch (evae_bernoulli_unit_step); bits 2 / 3 the ELBO's assembly / the log-variance gradient's sum ride in the
# reparameterisation's backward (evae_reparam_logq_bwd_hardtanh_tail): five nodes less per step, bit-equal results.  Un-profiled
# (tools/ab_node_merge.sh, profiles/r06_ab/node_merge.txt): C = 200 0.199 -> 0.189 ms, c1 0.217 -> 0.208, c2a 0.315 -> 0.310; at c2
# (GPU-bound) bits 0, 1, 3 are neutral and bit 2 costs 5 us -- the assembly then sits ON the chain the layer-2 weight gradient waits
# for instead of in front of it --, so it is merged in host-bound steps only.
def node_merge(Cl, B):
    e = os.environ.get("EVAE_NODE_MERGE")
    if e is not None:
        return int(e)
    return 15 if Cl + B <= 8192 else 11


ONE_STREAM = [os.environ.get("EVAE_ONE_STREAM", "0") == "1"]      # experiment: the whole step on the caller's stream

# schedule switches (bit mask; tools/chain_bench.sh sweeps them): 1 = the prior's dz' / dlogvar reduction on the side stream,
# 2 = the finish launch of encoder layer 2's weight gradient on the side stream, 4 = byte store: the layer-2 data gradient writes
# the three-term bf16 tile images of [dh | dg]^T itself (evae_dense_bwd_data_img) instead of an fp32 buffer + transposing pre-pass:
# measured 0.7741 vs 0.7754 ms -- the 38 us pre-pass goes, but the epilogue's 8-byte scattered stores cost the GEMM +15 us and the
# weight-gradient GEMM reads the images +11 us slower; kept as an option, off.  1 and 2 OFF: measured at config 2 (r02), 0 ->
# 0.975 ms/step, 1 -> 1.002, 2 -> 1.085, 3 -> 1.076 -- a launch that runs beside a CU-filling GEMM costs that GEMM more than
# the launch saves on the main stream.  8 = byte store: the two bandwidth-bound pre-passes of the first layer's weight gradient
# (evae_dense_bwd_weight_u8_phased) on the side stream beside layer 2's weight-gradient GEMM: 0.772 / 0.800 ms vs 0.744 -- the same
# lesson once more, off.
SCHED = int(os.environ.get("EVAE_SCHED", "0"))
# byte store: encoder layer 1's (dh, dg) leave the layer-2 data gradient as the bf16 tile images of its weight gradient
# (evae_dense_bwd_data_img; r03: 16-byte stores after a lane-pair exchange, on the split-bf16 kernel) -- no fp32 [Mp x 2H]
# buffer, no 36-us split / transposition pre-pass.  EVAE_IMG_DGRAD=0: the fp32 buffer + pre-pass
FINISH_GROUP_HEAD = os.environ.get("EVAE_FINISH_GROUP_HEAD", "0") == "1"   # ... the mean head's too (needs the side stream joined first)
# One finish launch for the step's split-K weight gradients (evae_dense_bwd_weight_finish_group) instead of one behind each GEMM.
# Measured r03 and OFF: launches that follow each other on ONE stream of the replayed graph start back to back (gap 0.0 us in
# profiles/r03_step_timeline_C25000.txt; the ~6 us gaps sit at cross-stream joins), so the merged launch saves nothing -- it ran
# 23.4 us against 8.7 + 10.1 for the two it replaces (c2 0.6446-0.6468 vs 0.641-0.645 ms); with the mean head's finish in it as
# well the side stream has to be joined earlier: c2 +10 us, C = 200 +17 us.
FINISH_GROUP = os.environ.get("EVAE_FINISH_GROUP", "0") == "1"
# the mean head's weight gradient (a 29-us streaming launch alone) right behind the batch rows' reparameterisation backward instead of
# at the end of the side stream's chain: it then runs beside the HBM-bound head data gradient, not beside layer 2's data gradient
HEADW_EARLY = int(os.environ.get("EVAE_HEADW_EARLY", "0"))   # r06: OFF -- with the head gradient in front of them the batch rows' thin data gradients (which the main stream's layer-2 weight gradient waits for) finished 20 us after layer 2's data gradient: 0.553 -> 0.542 ms
ELBO_SPLIT = os.environ.get("EVAE_ELBO_SPLIT", "0") != "0"         # captured step: merge on the prior's stream, ELBO assembly beside it
# (r04 A/B, profiles/r04_ab: the 7-block merge launch takes 10.7 us against the one-block merge + ELBO's 11.6 and the join it
#  saves comes back as a 9-us gap in front of the prior's backward: c2 0.616-0.621 -> 0.623-0.629 ms.  Off; what replaced it:)
# captured step on one device: the prior's forward partials, their merge and its backward as ONE launch in the forward pass
# (csrc/evae_prior_train.h), the ELBO assembly on the side stream
PRIOR_TRAIN = os.environ.get("EVAE_PRIOR_TRAIN", "1") != "0"
GROUP_LEAVES = os.environ.get("EVAE_GROUP_LEAVES", "1") != "0"      # the batch rows' four leaf weight gradients as one launch
IMG_DGRAD = os.environ.get("EVAE_IMG_DGRAD", "1") != "0" or bool(SCHED & 4)
THIN_ROWS = 1024     # batch rows up to here take the fp32 split-K kernel for the first layer even on the byte store
# byte store, exact prior, a machine-filling exemplar count: encoder layer 2's three GEMMs over pre-split bf16 operand images
# (csrc/evae_gemm_p6.h) -- layer 1's output and the heads' (dh2, dg2) leave their producers' epilogues as the images of their
# transposes, the weights are split once per step; no fp32 operand is re-split inside a GEMM.  EVAE_P6=0: the split-bf16 /
# fp32 kernels of r03
P6 = os.environ.get("EVAE_P6", "1") != "0"

PARAM_ORDER = [
    "prior_log_variance",
    "p_x_mean.linear.weight", "p_x_mean.linear.bias",
    "q_z_layers.0.h.weight", "q_z_layers.0.h.bias", "q_z_layers.0.g.weight", "q_z_layers.0.g.bias",
    "q_z_layers.1.h.weight", "q_z_layers.1.h.bias", "q_z_layers.1.g.weight", "q_z_layers.1.g.bias",
    "q_z_mean.weight", "q_z_mean.bias",
    "q_z_logvar.linear.weight", "q_z_logvar.linear.bias",
    "p_x_layers.0.h.weight", "p_x_layers.0.h.bias", "p_x_layers.0.g.weight", "p_x_layers.0.g.bias",
    "p_x_layers.1.h.weight", "p_x_layers.1.h.bias", "p_x_layers.1.g.weight", "p_x_layers.1.g.bias",
]
_NAMES = "plv wp bp w1h b1h w1g b1g w2h b2h w2g b2g wm bm wl bl d1h e1h d1g e1g d2h e2h d2g e2g".split()
# what the backward pass drops from the step state where it returns (the rest goes with the autograd node)
_BUFS = ("x rows data_ext A1 s1 A2 s2 mean_all logvar lv_pre z D1 sd1 D2 sd2 xmean lv_row zi ci lse eps "
         "elbo_keep prior_done dd centres_p bwd").split()


# The duplicates among the exemplar draw, the `dedup` field of the step's hand-off (evae/handoff.py; set by evae/graph.py): None, or
# (draws [C] int64, inv [C] int64, rep [Cl] int64, mult [Cl] fp32) with ex_idx = the Cl DISTINCT rows (padded, multiplicity 0).  The
# encoder then runs over the distinct rows only; the prior sees all C draws -- centres gathered through inv, leave-one-out mask on
# the draws' indices -- and a distinct row's head gradient is mult x the gradient of ONE of its draws (duplicates have identical
# centres, hence identical prior gradients).  Same loss, same gradients as encoding every draw (reference models/BaseModel.py:243-254).


def _launchers(dev):
    """(main stream, side stream, the main stream's launcher, the launcher of the batch rows' chain on the side stream)"""
    k = Launcher(dev)
    main = torch.cuda.current_stream()
    side = k.side_stream(ONE_STREAM[0])
    return main, side, k, Launcher(dev, stream=side, suffix="_side")


# ------------------------------------------------------------------------------------------------ forward stages
def _fwd_rows(st, x_idx, ex_idx, n_data, rows_ext, staged):
    """Stage the batch behind the dataset; one gather list for exemplars + batch.  data_ext is the fp32 copy of the dataset or
    its uint8 store (models/BaseModel.py::resident_u8): then the first layer runs on the byte kernels."""
    x, data_ext, B, Cl, dev = st.x, st.data_ext, st.B, st.Cl, st.dev
    stage = data_ext[n_data:n_data + B]
    st.stage_gen = _STAGE_GEN[data_ext.data_ptr()] = _STAGE_GEN.get(data_ext.data_ptr(), 0) + 1
    if st.u8:
        if not staged:                        # the captured step (evae/graph.py) writes the bytes itself
            stage.copy_(torch.round(x * 255.0))
    elif x.data_ptr() != stage.data_ptr():    # the captured step gathers the batch there itself
        stage.copy_(x)
    # rows_ext: caller-kept [Cl + B] gather list whose head IS ex_idx and whose tail already names the staging rows
    if st.approx:
        # head: filled behind the top-K below; the tail (the staging rows) never changes -- one buffer per geometry, kept
        # (a second forward before this one's backward is refused by the staging-row generation check, which covers it too)
        rkey = (dev, Cl, B, int(n_data))
        st.rows = _APPROX_ROWS.get(rkey)
        if st.rows is None:
            st.rows = _APPROX_ROWS[rkey] = torch.empty(Cl + B, dtype=torch.int64, device=dev)
            st.rows[Cl:] = torch.arange(n_data, n_data + B, device=dev)
    elif rows_ext is not None and rows_ext.numel() == Cl + B and rows_ext.data_ptr() == ex_idx.data_ptr():
        st.rows = rows_ext
    else:
        st.rows = torch.cat((ex_idx, torch.arange(n_data, n_data + B, device=dev)))


def _fwd_buffers(st):
    """a gated layer keeps its output and its gate s for the backward (dg = dout * out * (1 - s)); the batch rows are the tail rows"""
    B, D, H, Z, Mp, f32, t = st.B, st.D, st.H, st.Z, st.Mp, st.f32, st.fwd
    st.A1 = torch.empty((Mp, H), **f32); st.s1 = torch.empty_like(st.A1)
    st.A2 = torch.empty((Mp, H), **f32); st.s2 = torch.empty_like(st.A2)
    st.mean_all = torch.empty((Mp, Z), **f32)
    t.centres = st.mean_all[:st.Cl]
    t.z_mean = st.mean_all[st.Cl:]
    t.A2b = st.A2[st.Cl:]
    st.logvar = torch.empty((B, Z), **f32); st.lv_pre = torch.empty_like(st.logvar)
    st.z = torch.empty((B, Z), **f32); t.logq = torch.empty(B, **f32)
    st.D1 = torch.empty((B, H), **f32); st.sd1 = torch.empty_like(st.D1)
    st.D2 = torch.empty((B, H), **f32); st.sd2 = torch.empty_like(st.D2)
    st.xmean = torch.empty((B, D), **f32)
    t.RE = torch.empty(B, **f32)


def _fwd_images(k, st, p, ho, main, side):
    """operand images of the pre-split path (p6) and the first layer's weight split of the byte store"""
    H, D, Cl, Mp, lib, t = st.H, st.D, st.Cl, st.Mp, k.lib, st.fwd
    st.p6 = bool(st.u8 and P6 and IMG_DGRAD and not st.approx and Cl > 0 and Cl % 8 == 0 and st.B <= THIN_ROWS and not (SCHED & 10)
                 and lib.evae_gemm_p6_applies(Cl, H, 1) and lib.evae_gemm_x6_applies(Cl, H, 0))
    if st.p6:
        # images: h1^T (+ the all-ones row behind its H rows: the bias gradient of layer 2), [dh2 | dg2]^T, both with k along
        # all Cl + B rows; layer 2's weights in forward ([h | g] pairs) and data-gradient (W^T, banks stacked) form
        st.nks_m = lib.evae_p6_nks_rows(Mp)
        st.t_h1 = k.ws("p6_h1", lib.evae_p6_image_bytes(H + 1, st.nks_m))
        st.t_dq2 = k.ws("p6_dq2", lib.evae_p6_image_bytes(2 * H, st.nks_m))
        t.w2_img = k.ws("p6_w2", lib.evae_p6_image_bytes((H + 63) // 64 * 128, lib.evae_p6_nks(H)))
        st.w2t_img = k.ws("p6_w2t", lib.evae_p6_image_bytes(H, lib.evae_p6_nks(2 * H)))
        for t_, rows_ in ((st.t_h1, H + 1), (st.t_dq2, 2 * H)):
            key_ = (t_.numel(), Mp, H)
            if _P6_READY.get(t_.data_ptr()) != key_:     # padding rows / k are never written: zero once per buffer and shape
                t_.zero_()
                if rows_ == H + 1:
                    _lib.check(lib.evae_p6_fill_row(vp(t_), st.nks_m, H, 1.0, 0, Mp, k.st), "p6_fill_row")
                _P6_READY[t_.data_ptr()] = key_
    if st.u8:
        # both first-layer launches read the weights as three bf16 terms in tile order: split once, in front of the fork
        t.prep = k.ws("u8prep", lib.evae_dense_u8_prepared_bytes(H, D))
        if not ho.take_prep(t.prep.data_ptr(), p.w1h.data_ptr(), p.w1g.data_ptr()):
            # (the captured step's head launch -- evae/graph.py -- does this split beside its batch prologue and says so)
            _lib.check(lib.evae_dense_u8_prepare(vp(p.w1h), vp(p.w1g), H, D, vp(t.prep), t.prep.numel(), k.st), "u8_prepare")
        side.wait_stream(main)


def _l1_fwd(kk, st, p, rows_ptr, M, o):
    """encoder layer 1 over M gathered rows of the dataset buffer, into rows o / 4 .. of its output buffers"""
    D, H, lib, t = st.D, st.H, kk.lib, st.fwd
    out, s_, fl = st.A1.data_ptr() + o * H, st.s1.data_ptr() + o * H, 2.0 * M * D * 2 * H
    if not st.u8:
        kk.gated_fwd(st.data_ext, rows_ptr, M, D, st.ldd, p.w1h, p.b1h, p.w1g, p.b1g, H, out, None, s_)
    elif st.p6:        # ... and the output as h1^T's image, rows o / 4 .. of its k range
        ops.probed("gated_dense_fwd_u8 M=%d K=%d N=%d (uint8 rows, three bf16 terms; output + its pre-split image)" % (M, D, H), fl,
                   lambda: _lib.check(lib.evae_gated_dense_fwd_u8_timg(
                       vp(st.data_ext), vp(rows_ptr), M, D, st.ldd, 1.0 / 255.0, vp(t.prep), vp(p.b1h), vp(p.b1g), H, vp(out), vp(s_),
                       vp(st.t_h1), st.nks_m, 0, o // 4, kk.st), "gated_fwd_u8_timg"), executed=3 * fl, pipe="bf16-mfma")
    else:
        ops.probed("gated_dense_fwd_u8 M=%d K=%d N=%d (uint8 rows, three bf16 terms)" % (M, D, H), fl,
                   lambda: _lib.check(lib.evae_gated_dense_fwd_u8(vp(st.data_ext), vp(rows_ptr), M, D, st.ldd, 1.0 / 255.0, vp(t.prep),
                                                                  vp(p.b1h), vp(p.b1g), H, vp(out), vp(s_), kk.st), "gated_fwd_u8"),
                   executed=3 * fl, pipe="bf16-mfma")


def _xt_gather(k, kd, st):
    """The byte layer's weight gradient wants the gathered rows transposed (pixel-major): that needs the gather list only, so it
    runs in the forward pass on the side stream instead of in the backward's chain of launches -- r03: BEHIND the batch-row chain
    (it then runs beside the prior / ELBO / prior-backward launches, when the machine is nearly idle) instead of in front of it
    (where it delayed that chain by its 28 us and shared the exemplar encoder's bandwidth: the side stream, not the main one,
    was what the prior waited for)."""
    H, lib = st.H, k.lib
    wq_ = k.ws("wgrad_u8_fused", lib.evae_dense_bwd_weight_u8_workspace_bytes(st.Mp, 2 * H, st.D))
    gen_ = _XT_GEN[wq_.data_ptr()] = _XT_GEN.get(wq_.data_ptr(), 0) + 1
    _lib.check(lib.evae_dense_bwd_weight_u8_phased(None, st.Mp, 2 * H, 2 * H, vp(st.data_ext), vp(st.rows), st.D, st.ldd, 1.0 / 255.0,
                                                   None, None, vp(wq_), wq_.numel(), 3, kd.st), "bwd_weight_u8(gather)")
    st.xt = (wq_.data_ptr(), gen_)


def _fwd_batch_rows(k, kd, st, p, ho, side):
    """The batch rows' chain on the side stream: encoder (into the tail rows of the exemplar rows' buffers), heads, sample,
    decoder, reconstruction term.  It runs BESIDE the exemplar encoder; the streams meet at the prior (z) and at the ELBO."""
    B, D, H, Z, Cl, f32, lib, t = st.B, st.D, st.H, st.Z, st.Cl, st.f32, k.lib, st.fwd
    offb = 4 * Cl                                    # byte offset of the batch rows, per float of row width
    A1b, s1b = st.A1.data_ptr() + offb * H, st.s1.data_ptr() + offb * H
    plv, x, eps = p.plv.detach(), st.x, st.eps
    with torch.cuda.stream(side):
        # (on the side stream, in front of everything: with the byte gather moved behind the batch-row chain the MAIN stream's
        # head GEMM is what the prior waits for, and this 5-us launch sat between the two)
        st.thin_heads = B <= THIN_ROWS and not (SCHED & 1024)
        bc_in_heads = bool((node_merge(Cl, B) & 1) and st.thin_heads and lib.evae_heads_reparam_fwd_bcast_applies(B, H, Z, H))
        if not bc_in_heads:
            _lib.check(lib.evae_broadcast_scalar(vp(plv), vp(st.lv_row), Z, kd.st), "broadcast_scalar")
        t.w2_ready = None
        if st.p6:
            # layer 2's weights as images (they change every step); the main stream meets them behind the first layer --
            # unless the captured step's head launch built them (evae/graph.py: two launches and one join less)
            ho.p6_images = (p.w2h.data_ptr(), p.w2g.data_ptr(), H, t.w2_img, st.w2t_img)
            if not ho.take_p6(p.w2h.data_ptr(), p.w2g.data_ptr()):
                _lib.check(lib.evae_p6_pack_rows(vp(p.w2h), vp(p.w2g), H, H, H, 1, vp(t.w2_img), t.w2_img.numel(), kd.st), "p6_pack_rows")
                _lib.check(lib.evae_p6_pack_cols(vp(p.w2h), vp(p.w2g), H, H, H, -1, lib.evae_p6_nks(2 * H), vp(st.w2t_img),
                                                 st.w2t_img.numel(), kd.st), "p6_pack_cols")
                t.w2_ready = torch.cuda.Event(); t.w2_ready.record()
        if st.xt_early and not st.xt_late:
            _xt_gather(k, kd, st)
        if st.p6:
            # the batch rows' first layer on the fp32 split-K kernel, its finish also writing rows Cl .. of h1^T's image
            t.wf = kd.ws("fwd", lib.evae_dense_fwd_workspace_bytes(B, D, H, 1))
            _lib.check(lib.evae_gated_dense_fwd_timg(vp(x), None, B, D, x.stride(0), vp(p.w1h), vp(p.b1h), vp(p.w1g), vp(p.b1g), H, vp(A1b),
                                                     None, vp(s1b), vp(st.t_h1), st.nks_m, 0, Cl, vp(t.wf), t.wf.numel(), kd.st), "gated_fwd_timg")
        elif st.u8 and B <= THIN_ROWS and not (SCHED & 32):
            # a thin launch of the byte kernel walks its 25 K-slabs on five blocks (29 us alone, 66 us beside the exemplar
            # GEMM); the batch is here as fp32 too (x = byte / 255), and the fp32 kernel splits K over the machine
            kd.gated_fwd(x, None, B, D, x.stride(0), p.w1h, p.b1h, p.w1g, p.b1g, H, A1b, None, s1b)
        else:
            _l1_fwd(kd, st, p, st.rows.data_ptr() + 8 * Cl, B, offb)
        kd.gated_fwd(A1b, None, B, H, H, p.w2h, p.b2h, p.w2g, p.b2g, H, st.A2.data_ptr() + offb * H, None, st.s2.data_ptr() + offb * H)
        if st.thin_heads:
            # both heads (one gated-style split-K GEMM: bank h = mean, bank g = log-variance) and the sample in two
            # launches instead of five
            if bc_in_heads:
                _lib.check(lib.evae_heads_reparam_fwd_bcast(vp(t.A2b), B, H, H, vp(p.wm), vp(p.bm), vp(p.wl), vp(p.bl), Z, -6.0, 2.0,
                                                            vp(eps), vp(t.z_mean), vp(st.lv_pre), vp(st.logvar), vp(st.z), vp(t.logq),
                                                            vp(plv), vp(st.lv_row), Z, kd.st), "heads_reparam_fwd_bcast")
            else:
                t.wh = kd.ws("heads", lib.evae_heads_reparam_fwd_workspace_bytes(B, H, Z))
                _lib.check(lib.evae_heads_reparam_fwd(vp(t.A2b), B, H, H, vp(p.wm), vp(p.bm), vp(p.wl), vp(p.bl), Z, -6.0, 2.0, vp(eps),
                                                      vp(t.z_mean), vp(st.lv_pre), vp(st.logvar), vp(st.z), vp(t.logq), vp(t.wh),
                                                      t.wh.numel(), kd.st), "heads_reparam_fwd")
            if st.approx:
                t.zm_ready = torch.cuda.Event(); t.zm_ready.record()
        else:
            kd.linear_fwd(t.A2b, B, H, H, p.wm, p.bm, Z, ACT_NONE, 0.0, 0.0, t.z_mean, None)
            if st.approx:
                t.zm_ready = torch.cuda.Event(); t.zm_ready.record()
            kd.linear_fwd(t.A2b, B, H, H, p.wl, p.bl, Z, ACT_HARDTANH, -6.0, 2.0, st.logvar, st.lv_pre)
            # ---- sample, decode, reconstruct
            _lib.check(lib.evae_reparam_logq_fwd(vp(t.z_mean), vp(st.logvar), vp(eps), B, Z, vp(st.z), vp(t.logq), kd.st), "reparam")
        t.z_ready = torch.cuda.Event(); t.z_ready.record()
        decoder_fwd(kd, st, p)
        if st.prior_train and (node_merge(Cl, B) & 2):
            # RE, the step's coefficient vectors and the sigmoid head's gradient in one launch (the backward pass skips its own)
            st.coef = (torch.empty(B, **f32), torch.empty(B, **f32), torch.empty(B, **f32))
            st.dpx = torch.empty((B, D), **f32)
            _lib.check(lib.evae_bernoulli_unit_step(vp(x), vp(st.xmean), B, D, vp(st.beta_dev), st.beta_host, vp(t.RE), vp(st.coef[0]),
                                                    vp(st.coef[1]), vp(st.coef[2]), vp(st.dpx), kd.st), "bernoulli_unit_step")
        else:
            _lib.check(lib.evae_bernoulli_ll_fwd(vp(x), vp(st.xmean), B, D, vp(t.RE), kd.st), "bernoulli")
        t.re_ready = torch.cuda.Event(); t.re_ready.record()
        if st.prior_train and st.dpx is None:
            # the step's coefficient vectors (-1/B, beta/B, -beta/B: evae_elbo_bwd of a unit upstream gradient on the batch mean)
            # HERE, on the stream whose backward chain reads them: that chain then waits for nothing of the prior's launch
            st.coef = (torch.empty(B, **f32), torch.empty(B, **f32), torch.empty(B, **f32))
            one = _ONES.get(st.dev)
            if one is None:
                one = _ONES[st.dev] = torch.ones(1, **f32)
            _lib.check(lib.evae_elbo_bwd(vp(one), 1, None, 0, None, 0, vp(st.beta_dev), st.beta_host, B, vp(st.coef[0]), vp(st.coef[1]),
                                         vp(st.coef[2]), kd.st), "elbo_bwd(unit)")
        if st.xt_late:
            _xt_gather(k, kd, st)


def _fwd_select(k, st, p, main, x_idx, ex_idx, approx_cache, approx_k):
    """Approximate prior: the batch's own cache rows refreshed with its means, top-k of every batch row among the candidates'
    cached latents, the B * k slots re-encoded; the rest of the batch-row path keeps running on the side stream."""
    t = st.fwd
    main.wait_event(t.zm_ready)
    t.xi = ops._i64(x_idx)
    approx_cache.index_copy_(0, t.xi, t.z_mean)
    t.sub_cache = approx_cache.index_select(0, ex_idx)
    t.nearest, _ = ops.pairdist_topk(t.z_mean, t.sub_cache, int(approx_k), want_val=False)
    t.sel_rows, t.ci_sel = ops.select_exemplars(t.nearest.view(-1), ex_idx, out_rows=st.rows[:st.Cl])     # straight into the gather list
    _l1_fwd(k, st, p, st.rows, st.Cl, 0)


def _fwd_exemplar_encoder(k, st, p, main, approx_cache):
    """encoder layer 2 and the mean head of the Cl exemplar rows on the main stream, which then meets z"""
    H, Z, Cl, lib, t = st.H, st.Z, st.Cl, k.lib, st.fwd
    if Cl > 0:
        if st.p6:
            if t.w2_ready is not None:
                main.wait_event(t.w2_ready)
            fl2 = 2.0 * Cl * H * 2 * H
            ops.probed("gated_dense_fwd M=%d K=%d N=%d (pre-split bf16 images)" % (Cl, H, H), fl2,
                       lambda: _lib.check(lib.evae_gated_dense_fwd_p6t(vp(st.t_h1), st.nks_m, Cl, H, vp(t.w2_img), vp(p.b2h), vp(p.b2g), H,
                                                                       vp(st.A2), vp(st.s2), k.st), "gated_fwd_p6t"),
                       executed=6 * fl2, pipe="bf16-mfma")
        else:
            k.gated_fwd(st.A1, None, Cl, H, H, p.w2h, p.b2h, p.w2g, p.b2g, H, st.A2, None, st.s2)
        k.linear_fwd(st.A2, Cl, H, H, p.wm, p.bm, Z, ACT_NONE, 0.0, 0.0, st.mean_all, None)
    if st.approx:
        approx_cache.index_copy_(0, t.sel_rows, t.centres)       # repeats of a row carry identical encodings
    main.wait_event(t.z_ready)                           # (also orders lv_row, written at the head of the side stream)


def _fwd_prior(k, st, x_idx, ex_idx, no_mask):
    """The exemplar prior (leave-one-out mask in training unless no_mask; with its collectives when sharded) on the main stream:
    as one launch with its backward (prior_train), as gathered shard partials, or as this device's un-merged split partials."""
    B, Z, Cl, Cp, f32, lib, t, dd = st.B, st.Z, st.Cl, st.Cp, st.f32, k.lib, st.fwd, st.fwd.dd
    z, beta = st.z, (st.beta_dev if st.beta_dev is not None else st.beta_host)
    # the centres the prior sees: one per DRAW.  With duplicate tables outside the one-launch prior (eager steps, sharded steps:
    # r06) they are gathered from the distinct rows' encodings here and the prior's kernels run over them as over any exemplar set
    st.centres_p = t.centres
    if dd is not None and not st.prior_train:
        st.centres_p = torch.empty((Cp, Z), **f32)
        _lib.check(lib.evae_gather_rows(vp(t.centres), vp(dd[1]), None, Cp, Z, vp(st.centres_p), k.st), "gather_rows(centres)")
    zi = st.zi = None if no_mask else ops._i64(x_idx)
    ci = st.ci = None if no_mask else (t.ci_sel if st.approx else ops._i64(dd[0] if dd is not None else ex_idx))
    t.logp = torch.empty(B, **f32); st.lse = torch.empty((2, B), **f32)      # lse: the (max, log sum) token of the merge
    st.z_all, st.zi_all = z, zi
    st.prior_done = None
    if st.prior_train:
        # forward AND backward of the prior here: token, log p, dcentres (rows [0, Cl) of the head-gradient buffer the backward
        # pass carries on with), dz' and dlogvar'.  ev_pre: what the side stream's backward chain waits for instead of the
        # main stream's latest launch (it needs nothing of the prior before dz')
        dmean_all = torch.empty((st.Mp, Z), **f32)
        packed = torch.empty(B * Z + Z, **f32)
        ev_pre = torch.cuda.Event(); ev_pre.record()
        keep_alive = None
        out = (t.logp, st.lse, None, packed[:B * Z].view(B, Z), dmean_all[:Cl], packed[B * Z:])
        if dd is not None:
            # the prior over all C draws: centres of the draws gathered from the distinct rows' encodings; a distinct row's
            # gradient = multiplicity x the gradient of one of its draws
            dc_x = torch.empty((Cp, Z), **f32)
            keep_alive = [dc_x]
            if os.environ.get("EVAE_PRIOR_ROWS", "1") != "0":
                # r06: the kernel reads draw j's centre through inv[j] and the reduction launch folds the per-draw gradients onto the
                # distinct rows: the two gather launches around the prior are gone (2 x ~5 us of the critical path)
                ops.prior_train_step_rows(z, t.centres, (dd[1], dd[2], dd[3]), st.lv_row, zi, ci, float(st.c_total), beta,
                                          out=out, dc_draws=dc_x, stream=k.st)
            else:
                centres_x = torch.empty((Cp, Z), **f32)
                keep_alive.append(centres_x)
                _lib.check(lib.evae_gather_rows(vp(t.centres), vp(dd[1]), None, Cp, Z, vp(centres_x), k.st), "gather_rows(centres)")
                ops.prior_train_step(z, centres_x, st.lv_row, zi, ci, float(st.c_total), beta, out=out[:4] + (dc_x, out[5]), stream=k.st)
                _lib.check(lib.evae_gather_rows(vp(dc_x), vp(dd[2]), vp(dd[3]), Cl, Z, vp(dmean_all), k.st), "gather_rows(dcentres)")
        else:
            ops.prior_train_step(z, t.centres, st.lv_row, zi, ci, float(st.c_total), beta, out=out, stream=k.st)
        # (the scratch of this launch rides along: the side stream's backward chain starts at ev_pre -- BESIDE the prior's launch -- and
        #  its buffers are allocated while the main stream is current; a scratch tensor freed at the end of this forward would be
        #  handed to them while the prior still reads / writes it.  r06: an allocation-order change made exactly that happen)
        st.prior_done = SimpleNamespace(dmean_all=dmean_all, packed=packed, ev_pre=ev_pre, keep_alive=keep_alive)
    if st.sharded == 2:
        # data-parallel batches over sharded exemplars: every rank scores the queries of ALL ranks against its
        # shard (same pair count as B queries against all C), the partials go back to their owners
        st.z_all = shard._all_gather_flat(z).reshape(-1, Z)
        st.zi_all = None if zi is None else shard._all_gather_flat(zi.contiguous()).reshape(-1)
        m, s, n, _ = ops.prior_lse_fwd(st.z_all, st.centres_p, st.lv_row, st.zi_all, ci)
        m, s, n = shard.gather_partials(m, s, n)                  # [R x R*B] each
        r0 = dist.get_rank() * B
        m, s, n = (t_[:, r0:r0 + B].contiguous() for t_ in (m, s, n))
    elif st.sharded:
        m, s, n, _ = ops.prior_lse_fwd(z, st.centres_p, st.lv_row, zi, ci)
        m, s, n = shard.gather_partials(m, s, n)
    if st.sharded:
        t.parts = (m, s, n, m.shape[0], m.shape[1])
    elif not st.prior_train:
        # one device: the per-split partials stay un-merged in the workspace
        t.w = k.ws("prior_fwd", lib.evae_prior_lse_fwd_workspace_bytes(B, Cp, Z))
        ns, prow = C.c_int(0), C.c_int(0)
        _lib.check(lib.evae_prior_lse_fwd_splits(vp(z), B, vp(st.centres_p), Cp, Z, vp(st.lv_row), vp(zi), vp(ci), vp(t.w),
                                                 t.w.numel(), C.byref(ns), C.byref(prow), k.st), "prior_lse_fwd_splits")
        pm = t.w.data_ptr(); ps = pm + 4 * prow.value * B
        t.parts = (pm, ps, ps + 4 * prow.value * B, ns.value, B)


def _fwd_merge(k, kd, st, ho, main, side, average):
    """where the main stream meets the reconstruction term, then the merge of the partial log-sum-exps (splits of this device, or
    the gathered shards) + the ELBO's assembly (+ batch means) in ONE launch"""
    B, f32, lib, t = st.B, st.f32, k.lib, st.fwd
    beta_dev, beta_host = st.beta_dev, st.beta_host
    # captured step (unit upstream promise) on one device: merge on the main stream, ELBO assembly on the side stream
    st.elbo_split = bool(ELBO_SPLIT and ho.unit_upstream and average and not st.sharded and st.xt_late and not ONE_STREAM[0])
    if st.prior_train or st.elbo_split:
        pass                             # the main stream does not meet the reconstruction term at all
    elif st.xt_late:
        main.wait_event(t.re_ready)      # (the side stream carries on with the gather; the backward pass joins it)
    else:
        main.wait_stream(side)
    t.loss = torch.empty(B, **f32); t.KL = torch.empty(B, **f32)
    t.means = torch.empty(3, **f32) if average else None
    if st.prior_train:
        return            # loss / KL / means: assembled on the side stream by the backward pass, behind its wait for dz'
    pm, ps, pn, R, ldp = t.parts
    if st.elbo_split:
        # r04: the merge (token, logp, coefficients) is all the prior's backward waits for: it follows the partials on the main
        # stream without meeting the side stream (a join and the single-block merge + ELBO launch less on the critical
        # path); loss / KL / means are assembled on the side stream, which the backward pass joins before anyone reads them
        st.coef = (torch.empty(B, **f32), torch.empty(B, **f32), torch.empty(B, **f32))
        _lib.check(lib.evae_prior_merge_coef(vp(pm), vp(ps), vp(pn), R, ldp, B, float(st.c_total), vp(beta_dev), beta_host,
                                             vp(t.logp), vp(st.lse), vp(st.coef[0]), vp(st.coef[1]), vp(st.coef[2]), k.st), "prior_merge_coef")
        t.merged = torch.cuda.Event(); t.merged.record()
        with torch.cuda.stream(side):
            side.wait_event(t.merged)
            _lib.check(lib.evae_elbo_assemble(vp(t.logp), vp(t.RE), vp(t.logq), vp(beta_dev), beta_host, B, vp(t.loss), vp(t.KL),
                                              vp(t.means), kd.st), "elbo_assemble")
    elif ho.unit_upstream and average and not st.sharded:
        # the caller (evae/graph.py) promises loss.backward(ones) on the batch mean and nothing else: the backward pass's
        # coefficient vectors are then known here (-1/B, beta/B, -beta/B) and its elbo_bwd launch is not needed
        st.coef = (torch.empty(B, **f32), torch.empty(B, **f32), torch.empty(B, **f32))
        _lib.check(lib.evae_prior_elbo_fwd_coef(vp(pm), vp(ps), vp(pn), R, ldp, B, float(st.c_total), vp(t.RE), vp(t.logq),
                                                vp(beta_dev), beta_host, vp(t.logp), vp(st.lse), vp(t.loss), vp(t.KL), vp(t.means),
                                                vp(st.coef[0]), vp(st.coef[1]), vp(st.coef[2]), k.st), "prior_elbo_fwd_coef")
    else:
        _lib.check(lib.evae_prior_elbo_fwd(vp(pm), vp(ps), vp(pn), R, ldp, B, float(st.c_total), vp(t.RE), vp(t.logq),
                                           vp(beta_dev), beta_host, vp(t.logp), vp(st.lse), vp(t.loss), vp(t.KL), vp(t.means),
                                           k.st), "prior_elbo_fwd")


# ------------------------------------------------------------------------------------------------ backward stages
def _bwd_grad_slots(st):
    """every parameter gradient is a view of one buffer (slots padded to 256 B), see shard.register_flat_grads -> the views by name"""
    D, H, Z, t = st.D, st.H, st.Z, st.bwd
    shapes = dict(plv=(1,), wp=(D, H), bp=(D,), w1=(2 * H, D), b1=(2 * H,), w2=(2 * H, H), b2=(2 * H,), wm=(Z, H), bm=(Z,), wl=(Z, H),
                  bl=(Z,), d1=(2 * H, Z), e1=(2 * H,), d2=(2 * H, H), e2=(2 * H,))
    offs, tot = {}, 0
    for name, shape in shapes.items():
        offs[name] = (tot, math.prod(shape))
        tot += (offs[name][1] + 63) // 64 * 64
    t.gflat = torch.empty(tot, **st.f32)          # the padding between slots is never read (only summed by the all-reduce)
    if st.sharded == 1 and os.environ.get("EVAE_REDUCE_ALL", "0") != "1":
        # replicated batch: only the encoder's gradients (slots w1 .. bm, contiguous) differ between the ranks
        shard.register_flat_grads(t.gflat, offs["w1"][0], offs["bm"][0] + (offs["bm"][1] + 63) // 64 * 64)
    elif st.sharded:
        shard.register_flat_grads(t.gflat)
    return SimpleNamespace(**{name: t.gflat[o:o + n].view(*shapes[name]) for name, (o, n) in offs.items()})


def _bwd_buffers(k, st, unit):
    """The gradient buffers of both chains, allocated while the main stream is current.  img_mode -- byte store: encoder layer 1's
    (dh, dg) leave the layer-2 data gradient as the bf16 tile images its weight gradient reads (no fp32 [Mp x 2H] buffer, no pre-pass);
    row blocks in aligned fours, and only where that data gradient fills the machine (C = 200: 0.291 -> 0.301 ms with it)."""
    B, D, H, Z, Cl, Mp, f32, lib, t = st.B, st.D, st.H, st.Z, st.Cl, st.Mp, st.f32, k.lib, st.bwd
    t.prior_done = st.prior_done is not None and unit
    t.dmean_all = st.prior_done.dmean_all if t.prior_done else torch.empty((Mp, Z), **f32)
    t.dq2 = torch.empty((Mp, 2 * H), **f32)                              # [dh2 | dg2] for all C + B rows
    t.img_mode = (st.data_ext.dtype == torch.uint8 and Cl % 8 == 0 and IMG_DGRAD and bool(lib.evae_gemm_x6_applies(Cl, H, 0)))
    assert t.img_mode or not st.p6
    t.dq1 = None if t.img_mode else torch.empty((Mp, 2 * H), **f32)
    if t.img_mode:
        ws_w1 = t.ws_w1 = k.ws("wgrad_u8_fused", lib.evae_dense_bwd_weight_u8_workspace_bytes(Mp, 2 * H, D))
        off_img, nslab_img = C.c_size_t(0), C.c_int(0)
        _lib.check(lib.evae_dense_bwd_weight_u8_images(Mp, 2 * H, D, C.byref(off_img), C.byref(nslab_img)), "u8_images")
        t.img_ptr, t.nslab_img = ws_w1.data_ptr() + off_img.value, nslab_img.value
        key = (ws_w1.data_ptr(), Mp, H, D)
        if _ZEROED.get("wgrad_u8") != key:       # image bytes no row / column maps to must be zero: once per buffer and shape
            # (the IMAGE region only: the transposed byte rows the forward pass left in front of it stay)
            nimg = ((2 * H + 127) // 128) * nslab_img.value * 3 * 128 * 32 * 2
            ws_w1[off_img.value:off_img.value + nimg].zero_()
            _ZEROED["wgrad_u8"] = key
    t.dpx_done = st.dpx is not None and unit     # (evae_bernoulli_unit_step, forward pass)
    t.dpx = st.dpx if t.dpx_done else torch.empty((B, D), **f32)
    t.dp2 = torch.empty((B, 2 * H), **f32)                               # [dh | dg] of decoder layer 2
    t.dp1 = torch.empty((B, 2 * H), **f32)
    t.dz = torch.empty((B, Z), **f32)
    t.dlvp = torch.empty((B, Z), **f32)
    # duplicate tables outside the one-launch prior: the prior's backward runs over the per-draw centres and a distinct row's
    # gradient is multiplicity x one of its draws' (evae_gather_rows with a scale), written where the head's data gradient reads
    t.dc_out = torch.empty((st.centres_p.shape[0], Z), **f32) if st.dd is not None else t.dmean_all


def _l2_dgrad(kk, st, p, M, ob, m_base, main_rows):
    """encoder layer 2's data gradient for M rows from byte offset ob (per float of row width), layer 1's gate derivative in its
    epilogue; main_rows: the exemplar rows on the main stream (they may read the head launch's transposed weights)"""
    H, lib, t = st.H, kk.lib, st.bwd
    dq2, wT = t.dq2.data_ptr() + ob * 2 * H, (st.wt[1] if (st.wt is not None and main_rows) else None)
    A1, s1 = st.A1.data_ptr() + ob * H, st.s1.data_ptr() + ob * H
    if not t.img_mode:
        dq1 = t.dq1.data_ptr() + ob * 2 * H
        kk.bwd_data(dq2, p.w2h, dq2 + 4 * H, p.w2g, M, H, 2 * H, H, A1, s1, dq1, dq1 + 4 * H, 2 * H, wT=wT)
        return
    fl_ = 2.0 * M * 2 * H * H
    if st.p6 and main_rows:
        # the exemplar rows: [dh2 | dg2]^T's image x W2^T's image on the bf16 pipe, (dh1, dg1) as the byte layer's images
        ops.probed("dense_bwd_data M=%d N=%d+%d K=%d (pre-split bf16 images; gate-backward epilogue -> bf16 tile images)"
                   % (M, H, H, H), fl_,
                   lambda: _lib.check(lib.evae_dense_bwd_data_p6t(vp(st.t_dq2), st.nks_m, M, 2 * H, vp(st.w2t_img), H, vp(A1), vp(s1),
                                                                  None, None, 0, vp(t.img_ptr), t.nslab_img, m_base, kk.st),
                                      "bwd_data_p6t"), executed=6 * fl_, pipe="bf16-mfma")
        return
    wd = kk.ws("dgrad", lib.evae_dense_bwd_data_workspace_bytes(M, H, H, 2))
    ex_, pipe_ = ops.gemm_pipe(M, H, False, fl_)
    ops.probed("dense_bwd_data M=%d N=%d+%d K=%d (gate-backward epilogue -> bf16 tile images)" % (M, H, H, H), fl_,
               lambda: _lib.check(lib.evae_dense_bwd_data_img(
                   vp(dq2), vp(p.w2h), vp(dq2 + 4 * H), vp(p.w2g), M, H, 2 * H, H, vp(A1), vp(s1), vp(t.img_ptr), t.nslab_img,
                   m_base, vp(wT), vp(wd), wd.numel(), kk.st), "bwd_data_img"), executed=ex_, pipe=pipe_)


def _bwd_prior(k, kd, st, main, side):
    """The prior term d(-cKL * logp) on the main stream (+ its collectives when sharded) -> dcentres, which land in the
    head-gradient buffer, dz' and dlogvar' (one packed buffer, so that the sharded case all-reduces it in place)."""
    B, Z, Cl, lib, t, dd = st.B, st.Z, st.Cl, k.lib, st.bwd, st.dd
    Cp = st.centres_p.shape[0]
    t.prior_finish = None

    def dc_fold():
        if dd is not None:
            _lib.check(lib.evae_gather_rows(vp(t.dc_out), vp(dd[2]), vp(dd[3]), Cl, Z, vp(t.dmean_all), k.st), "gather_rows(dcentres)")
    if t.prior_done:
        side.wait_event(st.prior_done.ev_pre)       # (not the prior's launch, which the forward pass put on the main stream)
    else:
        side.wait_stream(main)
    if st.sharded == 2:
        # data-parallel batches: the shard-side backward runs over the queries of all ranks (their lse and upstream
        # coefficients are gathered first); dz partials are summed over the shards and every rank keeps its rows.
        # dcentres and dlogvar are complete sums over all queries: the mean all-reduce of the parameter gradients
        # in AdamNormGrad.step then yields the gradient of the global-batch mean loss, no rescaling needed.
        RB = st.z_all.shape[0]
        t.lg = shard._all_gather_flat(torch.cat((st.lse.reshape(2, B), t.neg_cKL.reshape(1, B))))            # [R x 3 x B]
        t.lse_all = torch.stack((t.lg[:, 0].reshape(-1), t.lg[:, 1].reshape(-1))).contiguous()       # token of all R B queries
        t.gp_all = t.lg[:, 2].reshape(-1).contiguous()
        t.dz_all = torch.empty((RB, Z), **st.f32); t.dlv = torch.empty(Z, **st.f32)
        w = k.ws("prior_bwd", lib.evae_prior_lse_bwd_workspace_bytes(RB, Cp, Z))
        _lib.check(lib.evae_prior_lse_bwd(vp(st.z_all), RB, vp(st.centres_p), Cp, Z, vp(st.lv_row), vp(st.zi_all), vp(st.ci), vp(t.lse_all),
                                          vp(t.gp_all), vp(t.dz_all), vp(t.dc_out), vp(t.dlv), vp(w), w.numel(), k.st),
                   "prior_bwd")
        dc_fold()
        dist.all_reduce(t.dz_all, op=dist.ReduceOp.SUM)
        r0 = dist.get_rank() * B
        t.dzp = t.dz_all[r0:r0 + B]
    elif t.prior_done:
        t.packed = st.prior_done.packed           # the forward pass ran the prior's backward with it (evae_prior_train_step)
        t.dzp = t.packed[:B * Z].view(B, Z); t.dlv = t.packed[B * Z:]
    else:
        assert st.prior_done is None, "fused vae step: the captured form's backward was called with another upstream gradient"
        t.packed = torch.empty(B * Z + Z, **st.f32)
        t.dzp = t.packed[:B * Z].view(B, Z); t.dlv = t.packed[B * Z:]
        w = k.ws("prior_bwd", lib.evae_prior_lse_bwd_workspace_bytes(B, Cp, Z))
        pb_args = (vp(st.z), B, vp(st.centres_p), Cp, Z, vp(st.lv_row), vp(st.zi), vp(st.ci), vp(st.lse), vp(t.neg_cKL), vp(t.dzp),
                   vp(t.dc_out), vp(t.dlv), vp(w), w.numel())
        if st.sharded == 1 or dd is not None or not (SCHED & 1):
            _lib.check(lib.evae_prior_lse_bwd(*pb_args, k.st), "prior_bwd")
            dc_fold()
            if st.sharded == 1:
                dist.all_reduce(t.packed, op=dist.ReduceOp.SUM)
                if Cl > 0:
                    t.dmean_all[:Cl].mul_(float(dist.get_world_size()))
        else:
            # one device: the main stream only needs dcentres (phase 1); the reduction of the dz' / dlogvar partials
            # (phase 2) is issued on the side stream, in front of its only consumer
            _lib.check(lib.evae_prior_lse_bwd_phased(*pb_args, 1, k.st), "prior_bwd(1)")
            t.prior_finish = lambda: _lib.check(lib.evae_prior_lse_bwd_phased(*pb_args, 2, kd.st), "prior_bwd(2)")
    t.dz_ready = torch.cuda.Event(); t.dz_ready.record()


def _bwd_exemplar_dgrads(k, st, p):
    """data gradients of the mean head and of encoder layer 2 for the Cl exemplar rows (none of it needs the decoder)"""
    H, Z, Cl, lib, t = st.H, st.Z, st.Cl, k.lib, st.bwd
    wT = None if st.wt is None else st.wt[0]
    if st.p6:
        # (dh2, dg2) of the exemplar rows leave as [dh2 | dg2]^T's image only: their two consumers read images
        wh_ = k.ws("dgrad", lib.evae_dense_bwd_data_workspace_bytes(Cl, Z, H, 1))
        flh = 2.0 * Cl * Z * H
        ops.gemm_pipe(Cl, H, False, flh)      # (its answer is not used -- the launch is an HBM entry --; the query is part of the recorded issue order)
        # a K = 40 product with a [Cl x 2H] output: it streams -- reads dmean, A2 and s2, writes 6 bytes per element of [dh | dg]
        ops.probed("dense_bwd_data M=%d N=%d K=%d (gate-backward epilogue -> pre-split image)" % (Cl, Z, H), flh,
                   hbm_bytes=4.0 * Cl * (Z + 2 * H) + 6.0 * Cl * 2 * H, fn=
                   lambda: _lib.check(lib.evae_dense_bwd_data_timg(vp(t.dmean_all), vp(p.wm), None, None, Cl, Z, Z, H, vp(st.A2), vp(st.s2),
                                                                   None, None, 2 * H, vp(wT), vp(st.t_dq2), st.nks_m, 0, 0, vp(wh_),
                                                                   wh_.numel(), k.st), "bwd_data_timg"))
    else:
        k.bwd_data(t.dmean_all, p.wm, None, None, Cl, Z, Z, H, st.A2, st.s2, t.dq2, t.dq2.data_ptr() + 4 * H, 2 * H, wT=wT)
    _l2_dgrad(k, st, p, Cl, 0, 0, True)


def _bwd_batch_rows(kd, st, p, g, side):
    """The side stream's chain: reconstruction term through the decoder -> dz (+ the prior's dz') -> the head's and encoder layer
    2's data gradients for the B batch rows."""
    B, D, H, Z, Cl, lib, t = st.B, st.D, st.H, st.Z, st.Cl, kd.lib, st.bwd
    off, beta_dev, beta_host = 4 * Cl, st.beta_dev, st.beta_host
    z_mean, dmean_b = st.mean_all.data_ptr() + off * Z, t.dmean_all.data_ptr() + off * Z
    with torch.cuda.stream(side):
        # through the Bernoulli log-likelihood and the sigmoid head at once, then down the decoder
        if not t.dpx_done:
            _lib.check(lib.evae_bernoulli_sigmoid_bwd(vp(st.x), vp(st.xmean), vp(t.cRE), B, D, vp(t.dpx), kd.st), "bernoulli_sigmoid_bwd")
        decoder_dgrads(kd, st, p)
        side.wait_event(t.dz_ready)
        if t.prior_finish is not None:
            t.prior_finish()
        t.node_merge = node_merge(Cl, B)
        RE_, logq_, logp_, loss_, KL_, means_ = st.elbo_keep if t.prior_done else (None,) * 6
        if t.prior_done and not (t.node_merge & 4):      # (else the ELBO's assembly rides in the launch below)
            _lib.check(lib.evae_elbo_assemble(vp(logp_), vp(RE_), vp(logq_), vp(beta_dev), beta_host, B, vp(loss_), vp(KL_), vp(means_),
                                              kd.st), "elbo_assemble")
            loss_ = None
        if t.node_merge & 12:
            # reparameterisation + log q (+ the prior's dz', + the Hardtanh of the log-variance head), and in one more block of
            # the launch the ELBO's assembly (bit 2) and the sum of the prior's log-variance gradient row (bit 3)
            sum_here = bool(t.node_merge & 8)
            _lib.check(lib.evae_reparam_logq_bwd_hardtanh_tail(
                vp(z_mean), vp(st.logvar), vp(st.eps), vp(st.z), vp(t.dz), vp(t.dzp), vp(t.cKL), vp(st.lv_pre), -6.0, 2.0, B, Z,
                vp(dmean_b), vp(t.dlvp), vp(logp_), vp(RE_), vp(logq_), vp(beta_dev), beta_host, vp(loss_), vp(KL_), vp(means_),
                vp(t.dlv) if sum_here else None, Z, vp(g.plv) if sum_here else None, kd.st), "reparam_bwd_tail")
        else:
            # reparameterisation + log q (+ the prior's dz', + the Hardtanh of the log-variance head): one launch
            _lib.check(lib.evae_reparam_logq_bwd_hardtanh(vp(z_mean), vp(st.logvar), vp(st.eps), vp(st.z), vp(t.dz), vp(t.dzp), vp(t.cKL),
                                                          vp(st.lv_pre), -6.0, 2.0, B, Z, vp(dmean_b), vp(t.dlvp), kd.st), "reparam_bwd")
        if t.headw_early:
            kd.bwd_weight(t.dmean_all, st.Mp, Z, Z, st.A2, None, H, H, g.wm, g.bm)       # mean head, all C + B rows
        # head and encoder layer 2, batch rows
        dq2_b, A2b, s2b = t.dq2.data_ptr() + off * 2 * H, st.A2.data_ptr() + off * H, st.s2.data_ptr() + off * H
        if st.p6:
            # (fp32 rows for the batch rows' own layer-2 data gradient, and rows Cl .. of the image for the weight gradient)
            wh2 = kd.ws("dgrad", lib.evae_dense_bwd_data_workspace_bytes(B, Z, H, 2))
            _lib.check(lib.evae_dense_bwd_data_timg(vp(dmean_b), vp(p.wm), vp(t.dlvp), vp(p.wl), B, Z, Z, H, vp(A2b), vp(s2b),
                                                    vp(dq2_b), vp(dq2_b + 4 * H), 2 * H,
                                                    None, vp(st.t_dq2), st.nks_m, 0, Cl, vp(wh2), wh2.numel(), kd.st), "bwd_data_timg(batch)")
        else:
            kd.bwd_data(dmean_b, p.wm, t.dlvp, p.wl, B, Z, Z, H, A2b, s2b, dq2_b, dq2_b + 4 * H, 2 * H)
        t.dq2_rows_done = torch.cuda.Event(); t.dq2_rows_done.record()      # all layer 2's weight gradient needs of the batch rows
        _l2_dgrad(kd, st, p, B, off, Cl, False)
        t.batch_rows_done.record()


def _bwd_leaves(kd, st, g, side):
    """the weight gradients nobody waits for before the optimizer, on the side stream"""
    B, D, H, Z, t = st.B, st.D, st.H, st.Z, st.bwd
    with torch.cuda.stream(side):
        # mean head, all C + B rows (its finish joins the step's grouped finish launch when that is on)
        if t.fin_group and FINISH_GROUP_HEAD:
            kd.bwd_weight(t.dmean_all, st.Mp, Z, Z, st.A2, None, H, H, g.wm, g.bm, phase=1, ws_name="wgradh")
        elif not t.headw_early:
            kd.bwd_weight(t.dmean_all, st.Mp, Z, Z, st.A2, None, H, H, g.wm, g.bm)
        # the four leaf layers whose contraction is the B batch rows: ONE grouped launch (evae_dense_bwd_weight_group;
        # r02: four launches of 8-9 us each at the end of the side stream's chain)
        jobs = ((t.dpx, B, D, D, st.D2, H, H, g.wp, g.bp), (t.dp2, B, 2 * H, 2 * H, st.D1, H, H, g.d2, g.e2),
                (t.dp1, B, 2 * H, 2 * H, st.z, Z, Z, g.d1, g.e1),
                (t.dlvp, B, Z, Z, st.A2.data_ptr() + 4 * st.Cl * H, H, H, g.wl, g.bl))
        if B <= 128 and GROUP_LEAVES and all(n_ % 4 == 0 and k_ % 4 == 0 for _, _, n_, _, _, k_, _, _, _ in jobs):
            kd.bwd_weight_group(jobs)
        else:
            for dy_, m_, n_, ldy_, x_, k_, ldx_, dw_, db_ in jobs:
                kd.bwd_weight(dy_, m_, n_, ldy_, x_, None, k_, ldx_, dw_, db_)
        if not (t.node_merge & 8):
            _lib.check(kd.lib.evae_sum_small(vp(t.dlv), Z, vp(g.plv), kd.st), "sum_small")


def _w1_grad(k, st, g, no_finish=False):
    """encoder layer 1's weight gradient over all C + B gathered rows"""
    D, H, Mp, lib, t = st.D, st.H, st.Mp, k.lib, st.bwd
    if st.data_ext.dtype != torch.uint8:
        k.bwd_weight(t.dq1, Mp, 2 * H, 2 * H, st.data_ext, st.rows, D, st.ldd, g.w1, g.b1)
        return
    w = k.ws("wgrad_u8_fused", lib.evae_dense_bwd_weight_u8_workspace_bytes(Mp, 2 * H, D))
    fl = 2.0 * Mp * 2 * H * D
    # the forward pass left the transposed byte rows in the workspace (unless another step used it since)
    have_xt = st.xt is not None and st.xt == (w.data_ptr(), _XT_GEN.get(w.data_ptr()))
    args = (vp(t.dq1), Mp, 2 * H, 2 * H, vp(st.data_ext), vp(st.rows), D, st.ldd, 1.0 / 255.0, vp(g.w1), vp(g.b1), vp(w), w.numel())
    ops.probed("dense_bwd_weight_u8 M=%d N=%d K=%d (uint8 rows, three bf16 terms; %s)"
               % (Mp, 2 * H, D, "GEMM; planes summed by the step's last grouped launch" if no_finish else "pre-passes + GEMM + finish"),
               fl, lambda: _lib.check(lib.evae_dense_bwd_weight_u8_phased(*args, (4 if have_xt else 0) | (16 if no_finish else 0), k.st)
                                      if (have_xt or no_finish) else lib.evae_dense_bwd_weight_u8(*args, k.st), "bwd_weight_u8"),
               executed=3 * fl, pipe="bf16-mfma")


def _bwd_encoder_wgrads(k, kd, st, g, main, side, split_wait):
    """weight gradients of the two encoder layers over all C + B rows, on the main stream"""
    D, H, Z, Mp, lib, t = st.D, st.H, st.Z, st.Mp, k.lib, st.bwd
    w2_args = (t.dq2, Mp, 2 * H, 2 * H, st.A1, None, H, H, g.w2, g.b2)
    if SCHED & 2:
        # (layer 2's finish launch runs on the side stream, beside layer 1's GEMM instead of in front of it)
        k.bwd_weight(*w2_args, phase=1, ws_name="wgrad2")
        t.w2_done = torch.cuda.Event(); t.w2_done.record()
        _w1_grad(k, st, g)
        with torch.cuda.stream(side):
            side.wait_event(t.w2_done)
            k.bwd_weight(*w2_args, phase=2, ws_name="wgrad2", finish_on=kd)
    elif (SCHED & 8) and st.data_ext.dtype == torch.uint8:
        # the bandwidth-bound pre-passes of the byte layer's weight gradient (gather-transpose of the rows, split and
        # transposition of dy) on the side stream, beside layer 2's matrix-bound weight gradient
        w = k.ws("wgrad_u8_fused", lib.evae_dense_bwd_weight_u8_workspace_bytes(Mp, 2 * H, D))

        def w1_phase(phase, s_):
            _lib.check(lib.evae_dense_bwd_weight_u8_phased(vp(t.dq1), Mp, 2 * H, 2 * H, vp(st.data_ext), vp(st.rows), D, st.ldd, 1.0 / 255.0,
                                                           vp(g.w1), vp(g.b1), vp(w), w.numel(), phase, s_), "bwd_weight_u8_phased")
        t.dq1_ready = torch.cuda.Event(); t.dq1_ready.record()
        with torch.cuda.stream(side):
            side.wait_event(t.dq1_ready)
            w1_phase(1, kd.st)
            t.pre_done = torch.cuda.Event(); t.pre_done.record()
        k.bwd_weight(*w2_args)
        main.wait_event(t.pre_done)
        w1_phase(2, k.st)
    elif t.fin_group:
        # ONE finish launch for the three split-K weight gradients of the step (encoder layer 1 on the byte store, layer 2, mean
        # head) at the very end, instead of one behind each GEMM: a dependent launch less on the main stream's chain
        k.bwd_weight(*w2_args, phase=1, ws_name="wgrad2")
        if split_wait:
            main.wait_event(t.batch_rows_done)
        _w1_grad(k, st, g, no_finish=True)
        if FINISH_GROUP_HEAD:
            main.wait_stream(side)      # (the mean head's GEMM and the grouped leaves)
        w_u8 = k.ws("wgrad_u8_fused", lib.evae_dense_bwd_weight_u8_workspace_bytes(Mp, 2 * H, D))
        w_2 = k.ws("wgrad2", lib.evae_dense_bwd_weight_workspace_bytes(Mp, 2 * H, H))
        w_h = kd.ws("wgradh", lib.evae_dense_bwd_weight_workspace_bytes(Mp, Z, H))
        fjobs = ((1, Mp, 2 * H, D, 2 * H, st.ldd, 1.0 / 255.0, g.w1, g.b1, w_u8), (0, Mp, 2 * H, H, 2 * H, H, 1.0, g.w2, g.b2, w_2),
                 (0, Mp, Z, H, Z, H, 1.0, g.wm, g.bm, w_h))[:3 if FINISH_GROUP_HEAD else 2]
        arr, n, _keep = wgrad_finish_jobs(fjobs)
        _lib.check(lib.evae_dense_bwd_weight_finish_group(arr, n, k.st), "bwd_weight_finish_group")
    else:
        if st.p6:
            # layer 2's weight gradient (+ bias gradient through h1^T's ones row) from the two images, on the bf16 pipe
            ww = k.ws("wgrad_p6", lib.evae_dense_bwd_weight_p6_workspace_bytes(st.nks_m, 2 * H, H))
            flw = 2.0 * Mp * 2 * H * H
            ops.probed("dense_bwd_weight M=%d N=%d K=%d (+db; pre-split bf16 images, split-K GEMM + finish)" % (Mp, 2 * H, H), flw,
                       lambda: _lib.check(lib.evae_dense_bwd_weight_p6(vp(st.t_dq2), vp(st.t_h1), st.nks_m, 2 * H, H, vp(g.w2), vp(g.b2), vp(ww),
                                                                       ww.numel(), k.st), "bwd_weight_p6"), executed=6 * flw, pipe="bf16-mfma")
        else:
            k.bwd_weight(*w2_args)
        if split_wait:
            main.wait_event(t.batch_rows_done)
        _w1_grad(k, st, g)


class VaeExactLoss(torch.autograd.Function):
    """forward(x [B x D] binarised batch, x_idx [B], data_ext [(N + pad) x D] resident dataset with staging
    rows, n_data, ex_idx_local [Cl] int64 (device), c_total, eps [B x z], beta, sharded, *params (PARAM_ORDER))
    -> (loss [B], RE [B], KL [B])."""

    @staticmethod
    def forward(ctx, x, x_idx, data_ext, n_data, ex_idx, c_total, eps, beta, sharded, no_mask, average, rows_ext, staged,
                approx_cache, approx_k, *params):
        p = named(_NAMES, params)
        dev = x.device
        B, D = x.shape
        ho = handoff.current() or handoff.StepHandoff()       # what the step's runner says about this step; nothing without one
        # approximate prior (reference models/BaseModel.py:256-271): ex_idx holds the CANDIDATE draw; the exemplar rows are the
        # B * k static slots picked by the top-K over the cached latents of the candidates (repeats masked, evae_select_exemplars)
        approx = approx_cache is not None
        Cl = B * int(approx_k) if approx else ex_idx.numel()
        st = ctx.step = SimpleNamespace(
            dev=dev, B=B, D=D, H=p.w1h.shape[0], Z=p.wm.shape[0], Cl=Cl, Mp=Cl + B, c_total=Cl if approx else c_total, approx=approx,
            sharded=int(sharded), beta=beta, f32=dict(device=dev, dtype=torch.float32), x=x.contiguous(), eps=eps, data_ext=data_ext,
            u8=data_ext.dtype == torch.uint8, ldd=data_ext.stride(0), coef=None, dpx=None, xt=None,
            fwd=SimpleNamespace(), bwd=None)        # fwd / bwd: the temporaries of one pass, dropped where it returns
        t = st.fwd
        _fwd_rows(st, x_idx, ex_idx, n_data, rows_ext, staged)
        main, side, k, kd = _launchers(dev)
        side.wait_stream(main)
        _fwd_buffers(st)
        _fwd_images(k, st, p, ho, main, side)
        if Cl > 0 and not approx:
            _l1_fwd(k, st, p, st.rows, Cl, 0)
        st.xt_early = bool(st.u8 and not approx and not (SCHED & 64))
        st.xt_late = st.xt_early and not (SCHED & 128)
        st.lv_row = torch.empty(st.Z, **st.f32)                     # the prior's log-variance row
        st.beta_dev, st.beta_host = beta_args(beta)
        dd = t.dd = ho.dedup
        if dd is not None and (approx or dd[2].numel() != Cl or dd[3].numel() != Cl):
            raise _lib.EvaeError("fused step: the duplicate tables do not belong to this exemplar set")
        st.Cp = dd[0].numel() if dd is not None else Cl          # exemplars the prior sees (all draws; this rank's when sharded)
        st.prior_train = bool(PRIOR_TRAIN and ho.unit_upstream and average and not sharded and Cl > 0 and not ONE_STREAM[0]
                              and ops.prior_train_applies(B, st.Cp, st.Z))
        _fwd_batch_rows(k, kd, st, p, ho, side)
        t.ci_sel = None
        if approx:
            _fwd_select(k, st, p, main, x_idx, ex_idx, approx_cache, approx_k)
        _fwd_exemplar_encoder(k, st, p, main, approx_cache)
        _fwd_prior(k, st, x_idx, ex_idx, no_mask)
        _fwd_merge(k, kd, st, ho, main, side, average)
        # (kept until the backward pass has joined the side stream: the assembly reads / writes them there, behind launches of
        #  the main stream that would otherwise be free to take their memory)
        st.elbo_keep = (t.RE, t.logq, t.logp, t.loss, t.KL, t.means) if (st.elbo_split or st.prior_train) else None
        st.dd = dd if (dd is not None and not st.prior_train) else None
        st.wt = ho.take_wt(p.wm.data_ptr(), p.w2h.data_ptr(), p.w2g.data_ptr())
        ctx.set_materialize_grads(False)       # unused outputs (RE, KL) then arrive as None, not as zero-filled tensors
        ctx.save_for_backward(*params)
        st.fwd = None
        if average:
            l, r, kl = t.means.unbind(0)
            return l, r, kl
        return t.loss, t.RE, t.KL

    @staticmethod
    def backward(ctx, dloss, dRE, dKL):
        p = named(_NAMES, ctx.saved_tensors)
        st = ctx.step
        if _STAGE_GEN.get(st.data_ext.data_ptr()) != st.stage_gen:
            raise _lib.EvaeError("fused vae step: another fused forward re-used the staging rows of this dataset before this "
                                 "backward ran (gradient accumulation over two batches): set model._use_fused = False for it")
        H, Cl = st.H, st.Cl
        main, side, k, kd = _launchers(st.dev)
        t = st.bwd = SimpleNamespace()
        g = _bwd_grad_slots(st)
        unit = upstream_coefs(k, st, dloss, dRE, dKL)
        # ---- two chains from here to the weight gradients (the order of issue below is the order the captured graph starts
        #      things in, and it matters: a chain of small launches crawls next to a GEMM that fills every CU): the prior's
        #      backward and the exemplar rows' data gradients on the main stream, the batch rows' chain and the leaves on the
        #      side stream.  They meet at the weight gradients, which run over all Cl + B rows in one launch per layer.
        _bwd_buffers(k, st, unit)
        _bwd_prior(k, kd, st, main, side)
        if Cl > 0:
            _bwd_exemplar_dgrads(k, st, p)
        t.batch_rows_done = torch.cuda.Event()
        t.fin_group = FINISH_GROUP and st.data_ext.dtype == torch.uint8 and not (SCHED & 10) and st.Mp > 128 and not st.p6
        t.headw_early = bool(HEADW_EARLY and not t.fin_group and Cl > 0)
        _bwd_batch_rows(kd, st, p, g, side)
        _bwd_leaves(kd, st, g, side)
        # (the leaves are issued HERE: captured after the main stream's weight gradients instead, the same launches replay at
        #  0.82-0.94 ms for C = 200 and 1.2 ms at c2 -- this runtime's graph replay is very sensitive to where a branch's nodes
        #  sit relative to the other branch's, r03 measurement)
        # Layer 2's weight gradient starts as soon as the batch rows' dq2 exist, without waiting for their layer-1 (dh, dg) (the
        # side stream's last thin data gradient, stretched to ~40 us beside the exemplar rows' GEMM).  r03: with the leaf
        # gradients as four launches this was 0.668 -> 0.684-0.694 ms (they then started behind layer 2's CU-filling launch and
        # ended after the main stream); with the leaves grouped into one launch it is 0.662-0.664 -> 0.658 ms.  SCHED & 256: off.
        split_wait = bool(SCHED & 256) and not (SCHED & 10)    # r04: off -- the thin batch-row chain ends long before layer 2's data gradient; one join less (-4 us)
        main.wait_event(t.dq2_rows_done if split_wait else t.batch_rows_done)
        _bwd_encoder_wgrads(k, kd, st, g, main, side, split_wait)
        main.wait_stream(side)
        for name in _BUFS:
            setattr(st, name, None)
        grads = (g.plv, g.wp, g.bp, g.w1[:H], g.b1[:H], g.w1[H:], g.b1[H:], g.w2[:H], g.b2[:H], g.w2[H:], g.b2[H:],
                 g.wm, g.bm, g.wl, g.bl, g.d1[:H], g.e1[:H], g.d1[H:], g.e1[H:], g.d2[:H], g.e2[:H], g.d2[H:], g.e2[H:])
        return (None,) * 15 + grads
