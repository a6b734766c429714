"""Host-side operators over the C ABI: raw launches on the current HIP stream plus the
torch.autograd.Function wrappers the reference-named modules (utils/nn.py, utils/distributions.py,
models/BaseModel.py) are built from.  PyTorch here is device memory, streams and autograd plumbing;
all arithmetic on [rows x features] data happens in libevae_hip.so.  No CPU fallback."""
import collections
import ctypes as C
import os

import torch

from . import _lib, handoff, launch
from ._lib import vp

ACT_NONE, ACT_SIGMOID, ACT_HARDTANH = 0, 1, 2
TOPK_SQRT = 1

_ws = {}
_ws_retired = []   # replaced buffers stay allocated: a captured hipGraph (evae/graph.py) may hold their addresses
PROBE = None   # bench.py sets {"records": []}: (name, start event, end event, algorithmic flops, executed flops, pipe) per big launch


def probed(name, flops, fn, executed=None, pipe="fp32-mfma", min_flops=2e9, hbm_bytes=None):
    """Run fn(); while bench.py's roofline probe is on, bracket it with a HIP event pair on the current stream (launches
    below min_flops are not worth an event pair).  `executed`: flops issued to the matrix pipe when they differ from the
    algorithmic count (three bf16 terms per product on the uint8 path).  hbm_bytes (pipe="hbm"): the ALGORITHMIC bytes of a
    streaming launch -- what it must read and write once -- recorded in place of the flop counts (>= 16 MB to be worth a pair)."""
    if PROBE is None or (flops < PROBE.get("min_flops", min_flops) if hbm_bytes is None else hbm_bytes < 16e6):
        return fn()
    if hbm_bytes is not None:
        flops, executed, pipe = hbm_bytes, hbm_bytes, "hbm"
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    PROBE["records"].append((name, e0, e1, float(flops), float(executed if executed is not None else flops), pipe))
    return r


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.EvaeError(
                "evae ops run on MI355X only (got a %s tensor); there is no CPU fallback" % t.device)


_SIDE_STREAM_OBJS = []     # ... the stream objects themselves
_SIDE_STREAMS = {}         # raw handle -> tag of streams registered as "side" streams: launches issued there get their own workspaces


def register_side_stream(stream, tag="side"):
    """Two launches that share a named workspace must not run at the same time.  A model that issues part of its step on a
    second stream (evae/fused_vae.py, models/AbsHModel.py) registers that stream here: every workspace requested while it is
    the current stream -- also from autograd's backward nodes, which run on the stream of their forward -- is a separate buffer."""
    _SIDE_STREAMS[int(stream.cuda_stream)] = tag
    if all(s_.cuda_stream != stream.cuda_stream for s_ in _SIDE_STREAM_OBJS):
        _SIDE_STREAM_OBJS.append(stream)


_MODEL_SIDE = {}


def model_side_stream(device):
    """The registered second stream of the modular two-stream training paths (one per device, made on first use)."""
    key = device.index if device.index is not None else torch.cuda.current_device()
    st = _MODEL_SIDE.get(key)
    if st is None:
        st = _MODEL_SIDE[key] = torch.cuda.Stream(device=device)
        register_side_stream(st)
    return st


_MODEL_LEAF = {}
_LEAF_ACTIVE = [None]


def model_leaf_stream(device):
    """Third stream of the modular two-stream training paths: the weight gradients of the thin layers (leaves of the backward
    pass: nothing but the optimizer reads them) run there, off the chain of data gradients."""
    key = device.index if device.index is not None else torch.cuda.current_device()
    st = _MODEL_LEAF.get(key)
    if st is None:
        st = _MODEL_LEAF[key] = torch.cuda.Stream(device=device)
        register_side_stream(st, "leaf")
    return st


class leaf_branch:
    """with ops.leaf_branch(stream): layers built inside (utils.nn.GatedDense) put their weight-gradient node on `stream`
    (gated_dense_split below); stream None: no effect."""

    def __init__(self, stream):
        self.stream = stream

    def __enter__(self):
        self.prev = _LEAF_ACTIVE[0]
        _LEAF_ACTIVE[0] = self.stream

    def __exit__(self, *a):
        _LEAF_ACTIVE[0] = self.prev


def active_leaf_stream():
    return _LEAF_ACTIVE[0]


def _workspace(name, nbytes, device):
    if _SIDE_STREAMS:
        tag = _SIDE_STREAMS.get(int(torch.cuda.current_stream(device).cuda_stream))
        if tag is not None:
            name = name + "@" + tag
    key = (name, device.index if device.index is not None else torch.cuda.current_device())
    buf = _ws.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is not None:
            # Never free a workspace: launches captured into a hipGraph have its raw address baked in, and a later,
            # larger request under the same name (evaluate_loss scores against all N_train exemplars) must not turn
            # every replay into a write to freed memory.  Growth is geometric, so the retired total stays < the live size.
            _ws_retired.append(buf)
            nbytes = max(int(nbytes), 2 * buf.numel())
        buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _ws[key] = buf
    return buf


_p = _vp = vp       # (the names this file, tests/ and tools/ call the one pointer conversion by)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32(t):
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


def _i64(t):
    if t is None:
        return None
    if t.dtype != torch.int64:
        t = t.long()
    t = t.reshape(-1)
    return t if t.is_contiguous() else t.contiguous()


# ------------------------------------------------------------------------------------------------
# exemplar prior
# ------------------------------------------------------------------------------------------------
def prior_lse_fwd(z, centres, log_var, z_idx=None, c_idx=None, want_prob=False):
    """One shard's partials: (max [B], sumexp [B], nmask [B], prob [B x C] or None)."""
    lib = _lib.load()
    _need_cuda(z, centres, log_var, z_idx, c_idx)
    z, centres, log_var = _f32(z), _f32(centres), _f32(log_var).reshape(-1)
    B, zd = z.shape
    Cn = centres.shape[0]
    z_idx, c_idx = _i64(z_idx), _i64(c_idx)
    if z_idx is not None and c_idx is not None:
        assert z_idx.numel() == B and c_idx.numel() == Cn
    else:
        z_idx = c_idx = None
    m = torch.empty(B, device=z.device); s = torch.empty_like(m); n = torch.empty_like(m)
    prob = torch.empty((B, Cn), device=z.device) if want_prob else None
    nb = lib.evae_prior_lse_fwd_workspace_bytes(B, Cn, zd)
    ws = _workspace("prior_fwd", nb, z.device)
    _lib.check(lib.evae_prior_lse_fwd(_p(z), B, _p(centres), Cn, zd, _p(log_var), _p(z_idx), _p(c_idx),
                                      _p(m), _p(s), _p(n), _p(prob), _p(ws), ws.numel(), _stream()),
               "evae_prior_lse_fwd")
    return m, s, n, prob


def gemm_x6_configure(enabled=-1, min_rows=-1):
    """Policy of the split-bf16 fp32 GEMM kernel (include/evae_hip.h: evae_gemm_x6_configure)."""
    _lib.check(_lib.load().evae_gemm_x6_configure(int(enabled), int(min_rows)), "evae_gemm_x6_configure")


def thin_configure(max_rows=-1):
    """Row-count limit of the one-launch thin layer kernels (include/evae_hip.h: evae_thin_configure); returns the value in force."""
    return int(_lib.load().evae_thin_configure(int(max_rows)))


def gemm_pipe(M, N, gated, flops):
    """(executed flops, pipe label) of an fp32 GEMM launch with M x N outputs for the roofline probe: six bf16 products per
    fp32 product when it takes the split-bf16 kernel."""
    if _lib.load().evae_gemm_x6_applies(int(M), int(N), int(bool(gated))):
        return 6.0 * flops, "bf16-mfma"
    return flops, "fp32-mfma"


def prior_set_norm_limit(limit):
    """Largest centred squared norm (sigma units) of a query tile the matrix-core prior kernels still evaluate in the
    expanded form; above it they switch to direct differences.  Negative restores the default, 0 forces the direct path."""
    _lib.check(_lib.load().evae_prior_set_norm_limit(float(limit)), "evae_prior_set_norm_limit")


def prior_merge(m, s, n, c_total, out=None):
    """[R x B] shard partials -> (logprior [B], token [2 x B]); `out` = caller-allocated (logprior, token).  The token is what
    the backward takes in place of the row log-sum-exp: row 0 = the row maximum, row 1 = the log of the normalised sum, kept
    apart (lse = token.sum(0)) so that exp(p_ij - lse_i) stays exact at any magnitude of the log-density
    (csrc/evae_prior.hip::prior_merge_kernel)."""
    lib = _lib.load()
    _need_cuda(m, s, n)
    ldp = _column_block_stride(m, s, n)
    if ldp is None:
        m, s, n = _f32(m), _f32(s), _f32(n)
    if m.dim() == 1:
        m, s, n = m[None], s[None], n[None]
    R, B = m.shape
    lp, lse = out if out is not None else (torch.empty(B, device=m.device), torch.empty((2, B), device=m.device))
    assert lse.numel() == 2 * B and lse.is_contiguous()
    if ldp is not None:
        # B columns of wider rows (a rank's own queries in the all-gathered partials, evae/shard.py): merged where they lie
        _lib.check(lib.evae_prior_merge_ld(_p(m), _p(s), _p(n), R, ldp, B, float(c_total), _p(lp), _p(lse), _stream()),
                   "evae_prior_merge_ld")
        return lp, lse
    _lib.check(lib.evae_prior_merge(_p(m), _p(s), _p(n), R, B, float(c_total), _p(lp), _p(lse), _stream()),
               "evae_prior_merge")
    return lp, lse


def _column_block_stride(m, s, n):
    """The common row stride of three fp32 [R x B] views that are column blocks of wider row-major buffers (unit column stride,
    rows ldp > B apart) -- or None: anything else goes through the contiguous form."""
    if not all(t.dim() == 2 and t.dtype == torch.float32 and t.shape == m.shape and t.shape[1] > 0 for t in (m, s, n)):
        return None
    if any(t.is_contiguous() or t.stride(1) != 1 or t.stride(0) != m.stride(0) for t in (m, s, n)):
        return None
    return int(m.stride(0)) if m.stride(0) > m.shape[1] else None


_PT_STATE = {}


def prior_train_state(device):
    """The 256-byte inter-block state of evae_prior_train_step: one per device and stream tag, zeroed when it is made and never again"""
    tag = _SIDE_STREAMS.get(int(torch.cuda.current_stream(device).cuda_stream), "") if _SIDE_STREAMS else ""
    key = (device.index if device.index is not None else torch.cuda.current_device(), tag)
    st = _PT_STATE.get(key)
    if st is None:
        st = _PT_STATE[key] = torch.zeros(64, dtype=torch.int32, device=device)
    return st


def prior_train_check():
    """Raise if any block of any one-launch prior (evae_prior_train_step) gave up waiting for the other blocks since the last
    check: its grid was not co-resident (another tenant of the device, a partition smaller than the query said) and some step's
    dz / dcentres / dlogvar were formed with a stale token.  Reads back: call it where the host synchronises anyway (end of an
    epoch, the replica check, the end of a timed loop) -- never inside a capture."""
    lib = _lib.load()
    for key, st in list(_PT_STATE.items()):
        n = lib.evae_prior_train_gave_up(_p(st), torch.cuda.current_stream(st.device).cuda_stream)
        if n < 0:
            _lib.check(n, "evae_prior_train_gave_up")
        if n > 0:
            raise RuntimeError("evae: %d block(s) of the one-launch exemplar prior gave up waiting for the rest of their grid (device "
                               "%s): gradients of at least one step are wrong.  The grid was not co-resident -- set "
                               "EVAE_PRIOR_TRAIN=0 to use the three-launch prior on this device" % (n, key[0]))


def prior_train_applies(B, Cn, zd):
    return bool(_lib.load().evae_prior_train_applies(int(B), int(Cn), int(zd)))


def prior_train_step_rows(z, centres, rows, log_var, z_idx, c_idx, c_total, beta, out, dc_draws, stream=None):
    """prior_train_step for a step that encoded each distinct image once: centres [n_rows x z], rows = (inv [C], rep [n_rows],
    mult [n_rows]); out = (logp, token, coef, dz, dcentres [n_rows x z], dlogvar), dc_draws [C x z] scratch."""
    lib = _lib.load()
    inv, rep, mult = rows
    B, zd = z.shape
    Cn = inv.numel()
    logp, token, coef, dz, dc, dlv = out
    beta_dev = beta if torch.is_tensor(beta) else None
    ws = _workspace("prior_train", lib.evae_prior_train_workspace_bytes(B, Cn, zd), z.device)
    st = prior_train_state(z.device)
    c3 = coef if coef is not None else (None, None, None)
    _lib.check(lib.evae_prior_train_step_rows(_p(z), B, _p(centres), centres.shape[0], _p(inv), _p(rep), _p(mult), Cn, zd, _p(log_var),
                                              _p(_i64(z_idx)), _p(_i64(c_idx)), float(c_total), _p(beta_dev),
                                              0.0 if beta_dev is not None else float(beta), _p(logp), _p(token), _p(c3[0]), _p(c3[1]),
                                              _p(c3[2]), _p(dz), _p(dc), _p(dc_draws), _p(dlv), _p(st), _p(ws), ws.numel(),
                                              _stream() if stream is None else stream), "evae_prior_train_step_rows")
    return out


def prior_train_step(z, centres, log_var, z_idx, c_idx, c_total, beta, want_coef=True, out=None, phase=0, stream=None):
    """The exemplar prior of a captured training step in one launch (+ the dz / dlogvar reduction): returns
    (logp [B], token [2 x B], (cRE, cKL, neg_cKL) or None, dz [B x z], dcentres [C x z], dlogvar [z]) for the loss
    mean_i(beta (logq_i - logp_i) - RE_i) with upstream gradient 1 (csrc/evae_prior_train.h).  `beta`: float or device scalar.
    `out` = caller-allocated (logp, token, coef, dz, dcentres, dlogvar)."""
    lib = _lib.load()
    _need_cuda(z, centres, log_var, z_idx, c_idx)
    z, centres, log_var = _f32(z), _f32(centres), _f32(log_var).reshape(-1)
    B, zd = z.shape
    Cn = centres.shape[0]
    z_idx, c_idx = _i64(z_idx), _i64(c_idx)
    if z_idx is None or c_idx is None:
        z_idx = c_idx = None
    dev = z.device
    if out is None:
        f = dict(device=dev, dtype=torch.float32)
        coef = (torch.empty(B, **f), torch.empty(B, **f), torch.empty(B, **f)) if want_coef else None
        out = (torch.empty(B, **f), torch.empty((2, B), **f), coef, torch.empty((B, zd), **f), torch.empty((Cn, zd), **f), torch.empty(zd, **f))
    logp, token, coef, dz, dc, dlv = out
    beta_dev = beta if torch.is_tensor(beta) else None
    ws = _workspace("prior_train", lib.evae_prior_train_workspace_bytes(B, Cn, zd), dev)
    st = prior_train_state(dev)
    c3 = coef if coef is not None else (None, None, None)
    _lib.check(lib.evae_prior_train_step(_p(z), B, _p(centres), Cn, zd, _p(log_var), _p(z_idx), _p(c_idx), float(c_total), _p(beta_dev),
                                         0.0 if beta_dev is not None else float(beta), _p(logp), _p(token), _p(c3[0]), _p(c3[1]), _p(c3[2]),
                                         _p(dz), _p(dc), _p(dlv), _p(st), _p(ws), ws.numel(), int(phase),
                                         _stream() if stream is None else stream), "evae_prior_train_step")
    return out


def prior_lse_bwd(z, centres, log_var, z_idx, c_idx, lse, grad_out):
    lib = _lib.load()
    _need_cuda(z, centres, log_var, lse, grad_out)
    if lse.numel() == z.shape[0] and lse.numel() > 0:      # a plain row log-sum-exp: token (lse, 0)
        lse = torch.stack((lse.reshape(-1).float(), torch.zeros_like(lse.reshape(-1), dtype=torch.float32)))
    assert lse.numel() == 2 * z.shape[0], "prior_lse_bwd: lse is the [2 x B] token of prior_merge (or a plain [B] log-sum-exp)"
    z, centres, log_var = _f32(z), _f32(centres), _f32(log_var).reshape(-1)
    lse, grad_out = _f32(lse), _f32(grad_out)
    B, zd = z.shape
    Cn = centres.shape[0]
    z_idx, c_idx = _i64(z_idx), _i64(c_idx)
    if z_idx is None or c_idx is None:
        z_idx = c_idx = None
    dz = torch.empty_like(z); dc = torch.empty_like(centres); dlv = torch.empty(zd, device=z.device)
    nb = lib.evae_prior_lse_bwd_workspace_bytes(B, Cn, zd)
    ws = _workspace("prior_bwd", nb, z.device)
    _lib.check(lib.evae_prior_lse_bwd(_p(z), B, _p(centres), Cn, zd, _p(log_var), _p(z_idx), _p(c_idx),
                                      _p(lse), _p(grad_out), _p(dz), _p(dc), _p(dlv), _p(ws), ws.numel(),
                                      _stream()), "evae_prior_lse_bwd")
    return dz, dc, dlv


class PriorLogP(torch.autograd.Function):
    """log p(z_i) under the exemplar mixture of ONE device's exemplars (models/BaseModel.py:98-128).
    forward(z, centres, log_var_row [zdim], z_idx|None, c_idx|None) -> logprior [B]."""

    @staticmethod
    def forward(ctx, z, centres, log_var_row, z_idx, c_idx):
        m, s, n, _ = prior_lse_fwd(z, centres, log_var_row, z_idx, c_idx)
        lp, lse = prior_merge(m, s, n, centres.shape[0])
        ctx.save_for_backward(z, centres, log_var_row, lse)
        ctx.idx = (z_idx, c_idx)
        return lp

    @staticmethod
    def backward(ctx, g):
        z, centres, log_var_row, lse = ctx.saved_tensors
        z_idx, c_idx = ctx.idx
        dz, dc, dlv = prior_lse_bwd(z, centres, log_var_row, z_idx, c_idx, lse, g.contiguous())
        return dz, dc, dlv.reshape(log_var_row.shape), None, None


# The captured step's promise (evae/graph.py): the loss is mean_i(beta KL_i - RE_i) with log p(z_i) entering KL_i with coefficient
# -1, and what follows is loss.backward(ones) -- so d loss / d log p(z_i) = -beta / B is known in the forward pass.  The runner
# puts its beta (device scalar) on the step's hand-off (evae/handoff.py: `beta`); None, or no hand-off: no promise.


class PriorLogPTrain(torch.autograd.Function):
    """PriorLogP under the promise of the hand-off's `beta`: forward partials, merge and backward in ONE launch (evae_prior_train_step,
    csrc/evae_prior_train.h); backward() hands out the gradients the forward pass computed (EVAE_PRIOR_TRAIN_CHECK=1: after
    checking the upstream gradient against -beta / B)."""

    @staticmethod
    def forward(ctx, z, centres, log_var_row, z_idx, c_idx, beta):
        logp, _tok, _c, dz, dc, dlv = prior_train_step(z.detach(), centres.detach(), log_var_row.detach(), z_idx, c_idx,
                                                       centres.shape[0], beta, want_coef=False)
        ctx.grads = (dz, dc, dlv.reshape(log_var_row.shape))
        ctx.beta = beta
        return logp

    @staticmethod
    def backward(ctx, g):
        dz, dc, dlv = ctx.grads
        if os.environ.get("EVAE_PRIOR_TRAIN_CHECK") == "1" and not torch.cuda.is_current_stream_capturing():
            want = -(ctx.beta if torch.is_tensor(ctx.beta) else torch.tensor(float(ctx.beta), device=g.device)) / g.numel()
            assert torch.allclose(g, want.expand_as(g), rtol=1e-6, atol=0.0), "PriorLogPTrain: the upstream gradient is not -beta / B"
        ctx.grads = None
        return dz, dc, dlv, None, None, None


def prior_logp(z, centres, log_var_row, z_idx, c_idx):
    """log p(z) [B] of ONE device's exemplars, differentiable: PriorLogP, or its one-launch training form under the hand-off's `beta`"""
    h = handoff.current()
    beta = h.beta if h is not None else None
    if (beta is not None and torch.is_grad_enabled() and z.is_cuda and z.dim() == 2 and centres.dim() == 2
            and z.dtype == torch.float32 and centres.dtype == torch.float32 and z.is_contiguous() and centres.is_contiguous()
            and (z.data_ptr() | centres.data_ptr()) % 16 == 0 and prior_train_applies(z.shape[0], centres.shape[0], z.shape[1])):
        return PriorLogPTrain.apply(z, centres, log_var_row, z_idx, c_idx, beta)
    return PriorLogP.apply(z, centres, log_var_row, z_idx, c_idx)


# ------------------------------------------------------------------------------------------------
# VampPrior: mixture of diagonal Gaussians with per-component variance (csrc/evae_mixture.hip)
# ------------------------------------------------------------------------------------------------
def _mixture_args(z, means, log_var):
    _need_cuda(z, means, log_var)
    z, means, log_var = _f32(z), _f32(means), _f32(log_var)
    if z.dim() != 2 or means.dim() != 2 or means.shape != log_var.shape or means.shape[1] != z.shape[1]:
        raise _lib.EvaeError("mixture: z [B x zdim], means and log_var [C x zdim] expected, got %s, %s, %s"
                             % (tuple(z.shape), tuple(means.shape), tuple(log_var.shape)))
    return z, means, log_var


def mixture_lse_fwd(z, means, log_var, n_components, want_prob=False):
    """log p(z_i) under the uniform mixture of the C diagonal Gaussians (means_j, exp(log_var_j)), weight 1 / n_components each:
    (logp [B], token [2 x B] for mixture_lse_bwd, prob [B x C] or None)."""
    lib = _lib.load()
    z, means, log_var = _mixture_args(z, means, log_var)
    B, zd = z.shape
    Cn = means.shape[0]
    logp = torch.empty(B, device=z.device)
    token = torch.empty((2, B), device=z.device)
    prob = torch.empty((B, Cn), device=z.device) if want_prob else None
    ws = _workspace("mixture_fwd", lib.evae_mixture_lse_fwd_workspace_bytes(B, Cn, zd), z.device)
    _lib.check(lib.evae_mixture_lse_fwd(_p(z), B, _p(means), _p(log_var), Cn, zd, float(n_components), _p(logp), _p(token),
                                        _p(prob), _p(ws), ws.numel(), _stream()), "evae_mixture_lse_fwd")
    return logp, token, prob


def mixture_lse_bwd(z, means, log_var, n_components, lse, grad_out, need=(True, True, True)):
    """Gradients (dz, dmeans, dlog_var) of sum_i grad_out_i logp_i from the token of mixture_lse_fwd; `need` leaves out the
    ones nobody asked for (None in their place).  n_components only shifts logp: it does not enter the gradients."""
    lib = _lib.load()
    z, means, log_var = _mixture_args(z, means, log_var)
    _need_cuda(lse, grad_out)
    lse, grad_out = _f32(lse), _f32(grad_out).reshape(-1)
    B, zd = z.shape
    Cn = means.shape[0]
    assert lse.numel() == 2 * B and grad_out.numel() == B, "mixture_lse_bwd: lse is the [2 x B] token of mixture_lse_fwd"
    dz = torch.empty_like(z) if need[0] else None
    dm = torch.empty_like(means) if need[1] else None
    dlv = torch.empty_like(log_var) if need[2] else None
    ws = _workspace("mixture_bwd", lib.evae_mixture_lse_bwd_workspace_bytes(B, Cn, zd), z.device)
    _lib.check(lib.evae_mixture_lse_bwd(_p(z), B, _p(means), _p(log_var), Cn, zd, _p(lse), _p(grad_out), _p(dz), _p(dm), _p(dlv),
                                        _p(ws), ws.numel(), _stream()), "evae_mixture_lse_bwd")
    return dz, dm, dlv


class MixtureLogP(torch.autograd.Function):
    """log p(z_i) under the VampPrior mixture (models/BaseModel.py:84-96,124-128).
    forward(z, means [C x zdim], log_var [C x zdim], n_components) -> logp [B]."""

    @staticmethod
    def forward(ctx, z, means, log_var, n_components):
        logp, token, _ = mixture_lse_fwd(z, means, log_var, n_components)
        ctx.save_for_backward(z, means, log_var, token)
        ctx.n_components = n_components
        return logp

    @staticmethod
    def backward(ctx, g):
        z, means, log_var, token = ctx.saved_tensors
        need = tuple(ctx.needs_input_grad[:3])
        dz, dm, dlv = mixture_lse_bwd(z, means, log_var, ctx.n_components, token, g, need=need)
        return dz, dm, dlv, None


def mixture_logp(z, means, log_var, n_components):
    """log p(z) [B] under the VampPrior mixture, differentiable in z, means and log_var"""
    _need_cuda(z, means, log_var)
    return MixtureLogP.apply(z, means, log_var, float(n_components))


class PseudoInputsFn(torch.autograd.Function):
    """X [C x D] = clamp(W^T, 0, 1) for the [D x C] weight of the VampPrior's `means` layer: what hardtanh(eye(C) @ W^T) gives,
    without the identity GEMM forward and its weight-gradient GEMM backward."""

    @staticmethod
    def forward(ctx, weight):
        lib = _lib.load()
        w = _f32(weight)
        D, Cn = w.shape
        out = torch.empty((Cn, D), device=w.device)
        _lib.check(lib.evae_pseudo_inputs_fwd(_p(w), D, Cn, _p(out), _stream()), "evae_pseudo_inputs_fwd")
        ctx.save_for_backward(w)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        w, = ctx.saved_tensors
        D, Cn = w.shape
        g = _f32(g)
        dw = torch.empty_like(w)
        _lib.check(lib.evae_pseudo_inputs_bwd(_p(w), _p(g), D, Cn, _p(dw), _stream()), "evae_pseudo_inputs_bwd")
        return dw


def pseudo_inputs(weight):
    _need_cuda(weight)
    if weight.dim() != 2:
        raise _lib.EvaeError("pseudo_inputs: a [D x C] weight expected, got %s" % (tuple(weight.shape),))
    return PseudoInputsFn.apply(weight)


# ------------------------------------------------------------------------------------------------
# distance + top-K
# ------------------------------------------------------------------------------------------------
def pairdist_topk(q, cache, k, sqrt=False, index_base=0, want_val=True):
    lib = _lib.load()
    _need_cuda(q, cache)
    q, cache = _f32(q), _f32(cache)
    B, zd = q.shape
    N = cache.shape[0]
    idx = torch.empty((B, k), dtype=torch.int64, device=q.device)
    val = torch.empty((B, k), device=q.device) if want_val else None
    nb = lib.evae_pairdist_topk_workspace_bytes(B, N, zd, k)
    ws = _workspace("topk", nb, q.device)
    _lib.check(lib.evae_pairdist_topk(_p(q), B, _p(cache), N, zd, k, TOPK_SQRT if sqrt else 0,
                                      int(index_base), _p(idx), _p(val), _p(ws), ws.numel(), _stream()),
               "evae_pairdist_topk")
    return idx, val


def pairwise_distance(q, cache):
    """[B x N] fp32 squared distances (fp64-accumulated)."""
    lib = _lib.load()
    _need_cuda(q, cache)
    q, cache = _f32(q), _f32(cache)
    out = torch.empty((q.shape[0], cache.shape[0]), device=q.device)
    _lib.check(lib.evae_pairwise_distance(_p(q), q.shape[0], _p(cache), cache.shape[0], q.shape[1], _p(out),
                                          _stream()), "evae_pairwise_distance")
    return out


class PairwiseDistance(torch.autograd.Function):
    """utils/distributions.py:12-18 with its gradient: D_ij = |q_i - c_j|^2,
    dq = 2 (rowsum(G) q - G c), dc = 2 (colsum(G) c - G^T q), the two products on the dense GEMM kernels."""

    @staticmethod
    def forward(ctx, q, cache):
        ctx.save_for_backward(q, cache)
        return pairwise_distance(q.detach(), cache.detach())

    @staticmethod
    def backward(ctx, G):
        q, cache = ctx.saved_tensors
        lib = _lib.load()
        qf, cf, G = _f32(q.detach()), _f32(cache.detach()), _f32(G)
        B, zd = qf.shape
        Cn = cf.shape[0]
        dq = dc = None
        if ctx.needs_input_grad[0]:
            Gc = _bwd_data(G.data_ptr(), cf, None, None, B, Cn, Cn, G.device)          # G c  [B x z]
            dq = 2.0 * (G.sum(dim=1, keepdim=True) * qf - Gc)
        if ctx.needs_input_grad[1]:
            Gtq, colsum = _bwd_weight(G, qf, None, zd)                                    # G^T q [C x z], colsum(G) [C]
            dc = 2.0 * (colsum.unsqueeze(1) * cf - Gtq)
        return dq, dc


PRIOR_MASK_ALL = -3      # EVAE_PRIOR_MASK_ALL: a c_idx entry that masks its exemplar slot for every query
SELECT_EXEMPLARS_MAX = 16384   # evae_select_exemplars keeps a call's positions in one block's LDS (csrc/evae_topk.hip)


def select_exemplars(pos, cand_idx, want_count=False, out_rows=None):
    """Static-shape form of `unique` + gather (models/BaseModel.py:265-266): pos [n] top-k positions into cand_idx [C].
    -> (sel_rows [n] dataset rows of every slot, c_idx [n]: the row for the first slot naming a position, PRIOR_MASK_ALL
    for its repeats).  out_rows: a contiguous int64 [n] tensor to take sel_rows (the head of a step's gather list)."""
    lib = _lib.load()
    _need_cuda(pos, cand_idx)
    pos, cand_idx = _i64(pos), _i64(cand_idx)
    n = pos.numel()
    if out_rows is not None:
        assert out_rows.dtype == torch.int64 and out_rows.numel() == n and out_rows.is_contiguous()
    sel = out_rows if out_rows is not None else torch.empty(n, dtype=torch.int64, device=pos.device)
    cidx = torch.empty(n, dtype=torch.int64, device=pos.device)
    cnt = torch.empty(1, dtype=torch.int32, device=pos.device) if want_count else None
    _lib.check(lib.evae_select_exemplars(_p(pos), n, _p(cand_idx), cand_idx.numel(), _p(sel), _p(cidx), _p(cnt), _stream()),
               "evae_select_exemplars")
    return (sel, cidx, cnt) if want_count else (sel, cidx)


def topk_merge(val, idx):
    """[R x B x k] candidate lists -> global ([B x k] idx, [B x k] val)."""
    lib = _lib.load()
    _need_cuda(val, idx)
    val = _f32(val)
    idx = idx.long().contiguous()
    R, B, k = val.shape
    oi = torch.empty((B, k), dtype=torch.int64, device=val.device)
    ov = torch.empty((B, k), device=val.device)
    _lib.check(lib.evae_topk_merge(_p(val), _p(idx), R, B, k, _p(oi), _p(ov), _stream()), "evae_topk_merge")
    return oi, ov


# ------------------------------------------------------------------------------------------------
# exact t-SNE (csrc/evae_tsne.hip); the driver is evae/tsne.py
# ------------------------------------------------------------------------------------------------
TSNE_SEARCH_STEPS = 100     # length of the precision search of every row (fixed: no data-dependent exit)
TSNE_PART_COLS = 8          # evae_tsne_forces' row record: A_x, A_y, R_x, R_y, Z_i, K_i, S_i, unused (include/evae_hip.h)


def tsne_max_points():
    """largest N the t-SNE kernels take (a row of distances in one workgroup's LDS)"""
    return int(_lib.load().evae_tsne_max_points())


def _tsne_state(name, t, N):
    if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (N, 2):
        raise _lib.EvaeError("tsne: %s must be a contiguous float32 [%d x 2] tensor (it is updated in place)" % (name, N))


def tsne_affinities(z, perplexity, steps=TSNE_SEARCH_STEPS):
    """z [N x zd] -> (P [N x N] joint affinities: symmetric bit for bit, zero diagonal, sum 1; beta [N] row precisions).
    The squared distances come from pairwise_distance; the conditionals and then P overwrite them in place."""
    _need_cuda(z)
    z = _f32(z)
    if z.dim() != 2:
        raise _lib.EvaeError("tsne_affinities: a [N x zd] tensor expected, got %s" % (tuple(z.shape),))
    N = z.shape[0]
    if N > tsne_max_points():
        raise _lib.EvaeError("tsne_affinities: N=%d above the cap of %d points" % (N, tsne_max_points()))
    P = pairwise_distance(z, z)
    beta = torch.empty(N, device=z.device)
    launch.Launcher(z.device).tsne_affinities(P, N, perplexity, steps, beta, P)
    return P, beta


def tsne_forces(P, Y, exaggeration=1.0, want_kl=False):
    """One pass over the pairs at embedding Y [N x 2] -> part [N x 8] float64, row i = (A_ix, A_iy, R_ix, R_iy, Z_i, K_i, S_i, -):
    w_ij = 1 / (1 + |y_i - y_j|^2), A_i = exaggeration sum_j P_ij w_ij (y_i - y_j), R_i = sum_j w_ij^2 (y_i - y_j),
    Z_i = sum_{j != i} w_ij; with want_kl K_i = sum_j P_ij log(P_ij / w_ij) and S_i = sum_j P_ij (otherwise 0)."""
    _need_cuda(P, Y)
    N = Y.shape[0]
    _tsne_state("Y", Y, N)
    if P.dtype != torch.float32 or not P.is_contiguous() or tuple(P.shape) != (N, N):
        raise _lib.EvaeError("tsne_forces: P must be a contiguous float32 [%d x %d] tensor" % (N, N))
    part = torch.empty((N, TSNE_PART_COLS), dtype=torch.float64, device=Y.device)
    launch.Launcher(Y.device).tsne_forces(P, Y, N, exaggeration, want_kl, part)
    return part


def tsne_update(part, Y, velocity, gains, momentum, lr, want_kl=False, want_grad=False):
    """One descent step from tsne_forces' part, IN PLACE on Y, velocity, gains [N x 2]: grad = 4 (A - R / Z), scikit-learn's
    gains (+0.2 where grad and velocity disagree in sign, x0.8 where they agree, floor 0.01), velocity = momentum velocity -
    lr gains grad, Y += velocity, Y -= mean(Y).  -> (grad [N x 2] or None, stats float64 [2] = (Z, KL of the Y the forces were
    taken at; 0 without want_kl))."""
    _need_cuda(part, Y, velocity, gains)
    N = Y.shape[0]
    for name, t in (("Y", Y), ("velocity", velocity), ("gains", gains)):
        _tsne_state(name, t, N)
    _tsne_part(part, N)
    grad = torch.empty((N, 2), device=Y.device) if want_grad else None
    stats = torch.empty(2, dtype=torch.float64, device=Y.device)
    launch.Launcher(Y.device).tsne_update(part, N, want_kl, momentum, lr, Y, velocity, gains, grad, stats)
    return grad, stats


def tsne_stats(part, want_kl=True):
    """float64 [2] = (Z, KL) of tsne_forces' part alone (KL needs the part of a want_kl pass)"""
    _need_cuda(part)
    N = part.shape[0]
    _tsne_part(part, N)
    stats = torch.empty(2, dtype=torch.float64, device=part.device)
    launch.Launcher(part.device).tsne_stats(part, N, want_kl, stats)
    return stats


def _tsne_part(part, N):
    if part.dtype != torch.float64 or not part.is_contiguous() or tuple(part.shape) != (N, TSNE_PART_COLS):
        raise _lib.EvaeError("tsne: part must be the float64 [%d x %d] tensor tsne_forces returns" % (N, TSNE_PART_COLS))


# ------------------------------------------------------------------------------------------------
# t-SNE on sparse affinities with exact repulsion (csrc/evae_tsne_nn.hip); TSNE(method='neighbours')
# ------------------------------------------------------------------------------------------------
def tsne_nn_max_points():
    """largest N of the sparse path (include/evae_hip.h says what sets it); tsne_update and tsne_stats take as many"""
    return int(_lib.load().evae_tsne_nn_max_points())


def tsne_nn_max_neighbours():
    """largest k of tsne_knn: one wave holds a row of the precision search in registers"""
    return int(_lib.load().evae_tsne_nn_max_neighbours())


def tsne_nn_neighbours(N, perplexity):
    """scikit-learn's n_neighbors: min(N - 1, floor(3 perplexity) + 1)"""
    return min(int(N) - 1, int(3.0 * float(perplexity) + 1))


def tsne_knn(z, k, strip_rows=0):
    """z [N x zd] -> (idx int32 [N x k], d2 float32 [N x k]): every point's k nearest OTHER points, nearest first, ordered by
    (value, index); fp64-accumulated squared distances as pairwise_distance gives them; the point itself is left out by index,
    so its exact duplicates stay eligible.  strip_rows: query rows per strip of distances (0: what fits 256 MiB); the result
    does not depend on it."""
    _need_cuda(z)
    z = _f32(z)
    if z.dim() != 2:
        raise _lib.EvaeError("tsne_knn: a [N x zd] tensor expected, got %s" % (tuple(z.shape),))
    N, zd = z.shape
    k = int(k)
    if N > tsne_nn_max_points():
        raise _lib.EvaeError("tsne_knn: N=%d above the cap of %d points" % (N, tsne_nn_max_points()))
    if not 1 <= k <= min(N - 1, tsne_nn_max_neighbours()):
        raise _lib.EvaeError("tsne_knn: k=%d outside [1, min(N - 1 = %d, %d)]" % (k, N - 1, tsne_nn_max_neighbours()))
    strip_rows = _strip_rows(strip_rows, "tsne_knn")
    idx = torch.empty((N, k), dtype=torch.int32, device=z.device)
    d2 = torch.empty((N, k), device=z.device)
    ws = torch.empty(_lib.load().evae_tsne_knn_workspace_bytes(N, strip_rows), dtype=torch.uint8, device=z.device)
    launch.Launcher(z.device).tsne_knn(z, N, zd, k, strip_rows, idx, d2, ws)
    return idx, d2


def nn_rank(z, nbr, strip_rows=0):
    """z [N x zd], nbr int32 [N x k] -> (rank int32 [N x k], row_sums int64 [N x 2]) (csrc/evae_nn_rank.hip):
    rank[i][m] = 1 + the number of points l != i with (d2(i, l), l) < (d2(i, j), j), j = nbr[i][m] -- the order and the distances
    of tsne_knn, whose own m-th neighbour has rank m + 1.  An entry j == i or outside [0, N) gets rank 0 (nbr is trusted, not
    checked: that would wait for the device; the kernel reads nothing for such an entry).  row_sums[i] = (sum of
    max(0, rank - k) over the entries with rank > 0, the number of entries with 1 <= rank <= k).  Exact integers; the result does
    not depend on strip_rows (query rows per strip of distances, 0: what fits 256 MiB)."""
    _need_cuda(z, nbr)
    z = _f32(z)
    if z.dim() != 2:
        raise _lib.EvaeError("nn_rank: a [N x zd] tensor expected, got %s" % (tuple(z.shape),))
    N, zd = z.shape
    if nbr.dtype != torch.int32 or not nbr.is_contiguous() or nbr.dim() != 2 or nbr.shape[0] != N:
        raise _lib.EvaeError("nn_rank: nbr must be a contiguous int32 [%d x k] tensor" % N)
    k = nbr.shape[1]
    if not 2 <= N <= tsne_nn_max_points():
        raise _lib.EvaeError("nn_rank: N=%d outside [2, %d]" % (N, tsne_nn_max_points()))
    if not 1 <= k <= min(N - 1, tsne_nn_max_neighbours()):
        raise _lib.EvaeError("nn_rank: k=%d outside [1, min(N - 1 = %d, %d)]" % (k, N - 1, tsne_nn_max_neighbours()))
    strip_rows = _strip_rows(strip_rows, "nn_rank")
    rank = torch.empty((N, k), dtype=torch.int32, device=z.device)
    row_sums = torch.empty((N, 2), dtype=torch.int64, device=z.device)
    ws = torch.empty(_lib.load().evae_nn_rank_workspace_bytes(N, strip_rows), dtype=torch.uint8, device=z.device)
    launch.Launcher(z.device).nn_rank(z, N, zd, nbr, k, strip_rows, rank, row_sums, ws)
    return rank, row_sums


def ball_count_max_points():
    """largest B and N of ball_count: the cap of the neighbour search its radii come from"""
    return int(_lib.load().evae_ball_count_max_points())


BallCount = collections.namedtuple("BallCount", "col_hits row_hits nn_idx nn_d2")


def ball_count(q, c, col_radius=None, row_radius=None, want_nearest=True, strip_rows=0):
    """q [B x d], c [N x d] -> BallCount(col_hits, row_hits, nn_idx, nn_d2) (csrc/evae_ball_count.hip):
    col_hits[i] = #{ j : D(q_i, c_j) < col_radius[j] }, row_hits[i] = #{ j : D(q_i, c_j) < row_radius[i] } (int32 [B]) and
    (nn_d2[i], nn_idx[i]) = the minimum of (D(q_i, c_j), j): the nearest column, the lower index on a tie.  D is
    pairwise_distance's fp32 value and every comparison strict, so radii from tsne_knn compare with the distances they were taken
    from.  A radius of None switches its count off, want_nearest=False the nearest pair; what is off is None.  Exact integers;
    the result does not depend on strip_rows (query rows per strip of distances, 0: what fits 256 MiB)."""
    _need_cuda(q, c, col_radius, row_radius)
    q, c = _f32(q), _f32(c)
    if q.dim() != 2 or c.dim() != 2:
        raise _lib.EvaeError("ball_count: [B x d] and [N x d] tensors expected, got %s and %s" % (tuple(q.shape), tuple(c.shape)))
    (B, d), (N, dc) = q.shape, c.shape
    if d != dc or d < 1:
        raise _lib.EvaeError("ball_count: q has %d features, c has %d (equal and >= 1 expected)" % (d, dc))
    cap = ball_count_max_points()
    if not (1 <= B <= cap and 1 <= N <= cap):
        raise _lib.EvaeError("ball_count: B=%d, N=%d outside [1, %d]" % (B, N, cap))
    if col_radius is not None:
        _dev_tensor("col_radius", col_radius, torch.float32, (N,), "ball_count")
    if row_radius is not None:
        _dev_tensor("row_radius", row_radius, torch.float32, (B,), "ball_count")
    if col_radius is None and row_radius is None and not want_nearest:
        raise _lib.EvaeError("ball_count: no output asked for (no radius and want_nearest=False)")
    strip_rows = _strip_rows(strip_rows, "ball_count")
    col_hits = torch.empty(B, dtype=torch.int32, device=q.device) if col_radius is not None else None
    row_hits = torch.empty(B, dtype=torch.int32, device=q.device) if row_radius is not None else None
    nn_idx = torch.empty(B, dtype=torch.int32, device=q.device) if want_nearest else None
    nn_d2 = torch.empty(B, device=q.device) if want_nearest else None
    ws = torch.empty(_lib.load().evae_ball_count_workspace_bytes(B, N, strip_rows), dtype=torch.uint8, device=q.device)
    launch.Launcher(q.device).ball_count(q, B, c, N, d, col_radius, row_radius, strip_rows, col_hits, row_hits, nn_idx, nn_d2, ws)
    return BallCount(col_hits, row_hits, nn_idx, nn_d2)


def kth_neighbour_radius(x, k, strip_rows=0):
    """x [N x d] -> float32 [N]: the squared distance from every row to its k-th nearest OTHER row (tsne_knn's column k - 1)"""
    return tsne_knn(x, k, strip_rows)[1][:, int(k) - 1].contiguous()


def tsne_nn_conditionals(d2, perplexity, steps=TSNE_SEARCH_STEPS):
    """d2 [N x k] from tsne_knn -> (beta [N], cond [N x k]): the precision search of tsne_affinities over each row's k values
    and the row's conditional p(j|i) on them (rows sum to 1)."""
    _need_cuda(d2)
    if d2.dim() != 2 or d2.dtype != torch.float32 or not d2.is_contiguous():
        raise _lib.EvaeError("tsne_nn_conditionals: d2 must be a contiguous float32 [N x k] tensor")
    N, k = d2.shape
    beta = torch.empty(N, device=d2.device)
    cond = torch.empty((N, k), device=d2.device)
    launch.Launcher(d2.device).tsne_nn_conditionals(d2, N, k, perplexity, steps, beta, cond)
    return beta, cond


def tsne_nn_affinities(z, perplexity, steps=TSNE_SEARCH_STEPS, strip_rows=0):
    """z [N x zd] -> (row_ptr int32 [N + 1], col int32 [nnz], val float32 [nnz], beta [N]): the joint
    P_ij = (p(j|i) + p(i|j)) / 2N in CSR, a conditional outside its row's k = min(N - 1, floor(3 perplexity) + 1) nearest
    neighbours being 0.  Columns ascend strictly within a row, there is no diagonal, nnz <= 2 N k, and val is bit-equal to its
    transpose.  The pattern is index plumbing in torch (one stable sort of the int64 keys i N + j of the forward edges and
    j N + i of the reverse ones; equal keys, two at most, end up adjacent); every floating-point value is formed in a kernel."""
    _need_cuda(z)
    z = _f32(z)
    if z.dim() != 2:
        raise _lib.EvaeError("tsne_nn_affinities: a [N x zd] tensor expected, got %s" % (tuple(z.shape),))
    N = z.shape[0]
    if not 0.0 < float(perplexity) < N:
        raise _lib.EvaeError("tsne_nn_affinities: perplexity %g outside (0, N=%d)" % (perplexity, N))
    k = tsne_nn_neighbours(N, perplexity)
    idx, d2 = tsne_knn(z, k, strip_rows)
    beta, cond = tsne_nn_conditionals(d2, perplexity, steps)
    del d2
    E = N * k
    rows = torch.arange(N, device=z.device, dtype=torch.int64).repeat_interleave(k)
    cols = idx.reshape(-1).long()
    keys, perm = torch.sort(torch.cat((rows * N + cols, cols * N + rows)), stable=True)     # forward edges first among equals
    del rows, cols, idx
    first = torch.ones(2 * E, dtype=torch.bool, device=z.device)
    first[1:] = keys[1:] != keys[:-1]
    entry = torch.cumsum(first, 0) - 1                       # the CSR entry each of the 2 E edges lands in
    nnz = int(entry[-1].item()) + 1
    forward = perm < E
    ia = torch.full((nnz,), -1, dtype=torch.int32, device=z.device)
    ib = torch.full((nnz,), -1, dtype=torch.int32, device=z.device)
    ia[entry[forward]] = perm[forward].int()                 # (i, j) listed by i: p(j|i) = cond[that edge]
    ib[entry[~forward]] = (perm[~forward] - E).int()         # (i, j) as the reverse of j's edge to i: p(i|j) = cond[that edge]
    keys = keys[first]
    del perm, entry, forward, first
    col = (keys % N).int()
    row_ptr = torch.zeros(N + 1, dtype=torch.int32, device=z.device)
    row_ptr[1:] = torch.cumsum(torch.bincount(keys // N, minlength=N), 0).int()
    val = torch.empty(nnz, device=z.device)
    launch.Launcher(z.device).tsne_nn_joint(cond, ia, ib, nnz, N, val)
    return row_ptr, col, val, beta


def tsne_nn_forces(row_ptr, col, val, Y, exaggeration=1.0, want_kl=False):
    """tsne_forces on the CSR matrix of tsne_nn_affinities -> the same part [N x 8] float64: A_i, K_i, S_i over row i's
    non-zeros, R_i and Z_i over all N points.  row_ptr [N + 1] is trusted to end at len(col) (checking would wait for the device)."""
    _need_cuda(row_ptr, col, val, Y)
    N = Y.shape[0]
    _tsne_state("Y", Y, N)
    if N > tsne_nn_max_points():
        raise _lib.EvaeError("tsne_nn_forces: N=%d above the cap of %d points" % (N, tsne_nn_max_points()))
    if row_ptr.dtype != torch.int32 or not row_ptr.is_contiguous() or tuple(row_ptr.shape) != (N + 1,):
        raise _lib.EvaeError("tsne_nn_forces: row_ptr must be a contiguous int32 [%d] tensor" % (N + 1))
    if col.dtype != torch.int32 or not col.is_contiguous() or col.dim() != 1:
        raise _lib.EvaeError("tsne_nn_forces: col must be a contiguous int32 [nnz] tensor")
    if val.dtype != torch.float32 or not val.is_contiguous() or tuple(val.shape) != tuple(col.shape):
        raise _lib.EvaeError("tsne_nn_forces: val must be a contiguous float32 [%d] tensor" % col.numel())
    part = torch.empty((N, TSNE_PART_COLS), dtype=torch.float64, device=Y.device)
    ws = torch.empty(_lib.load().evae_tsne_nn_forces_workspace_bytes(N), dtype=torch.uint8, device=Y.device)
    launch.Launcher(Y.device).tsne_nn_forces(row_ptr, col, val, Y, N, exaggeration, want_kl, part, ws)
    return part


# ------------------------------------------------------------------------------------------------
# argument checks the latent-analysis entries share (the strip-wise ones above; PCA, k-means, the scores and the mixture below)
# ------------------------------------------------------------------------------------------------
def _strip_rows(strip_rows, who):
    strip_rows = int(strip_rows)
    if strip_rows < 0:
        raise _lib.EvaeError("%s: strip_rows=%d (0 = automatic)" % (who, strip_rows))
    return strip_rows


def _dev_tensor(name, t, dtype, shape, who):
    """what the kernels take, converted by nobody: a wrong dtype, shape or a strided tensor is refused"""
    _need_cuda(t)
    if t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise _lib.EvaeError("%s: %s must be a contiguous %s %s tensor, got %s %s" % (who, name, dtype, list(shape), t.dtype,
                                                                                     tuple(t.shape)))


def _dev_rows(name, x, who, max_features=None, max_points=None):
    """the rows of an entry, float32 [N x d] within the entry's caps (None: checked elsewhere) -> (N, d)"""
    _need_cuda(x)
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_contiguous():
        raise _lib.EvaeError("%s: %s must be a contiguous float32 [N x d] tensor, got %s %s" % (who, name, x.dtype, tuple(x.shape)))
    N, d = x.shape
    if max_features is not None and not 1 <= d <= max_features:
        raise _lib.EvaeError("%s: %d features outside [1, %d]" % (who, d, max_features))
    if max_points is not None and not 1 <= N <= max_points:
        raise _lib.EvaeError("%s: N=%d outside [1, %d]" % (who, N, max_points))
    return N, d


# ------------------------------------------------------------------------------------------------
# PCA in fp64 (csrc/evae_pca.hip); the driver is evae/pca.py, TSNE(init='pca') its first user
# ------------------------------------------------------------------------------------------------
def pca_max_features():
    """widest input the PCA kernels take (the widest latent the project has)"""
    return int(_lib.load().evae_pca_max_features())


def pca_max_points():
    return int(_lib.load().evae_pca_max_points())


def pca_chunk_rows():
    """rows a block of pca_moments owns: the partial sums of the chunks are added in index order"""
    return int(_lib.load().evae_pca_chunk_rows())


def pca_max_sweeps():
    """the compile-time bound of pca_eigh's sweep loop"""
    return int(_lib.load().evae_pca_max_sweeps())


def pca_moments(x):
    """x [N x d] -> (mean [d], cov [d x d]), float64: the covariance (ddof 1) of the rows centred in fp64, two passes, symmetric
    bit for bit; equal inputs give bit-equal outputs."""
    _need_cuda(x)
    x = _f32(x)
    N, d = _dev_rows("x", x, "pca_moments", pca_max_features(), pca_max_points())
    if N < 2:
        raise _lib.EvaeError("pca_moments: N=%d, at least 2 rows expected" % N)
    mean = torch.empty(d, dtype=torch.float64, device=x.device)
    cov = torch.empty((d, d), dtype=torch.float64, device=x.device)
    ws = torch.empty(_lib.load().evae_pca_workspace_bytes(N, d), dtype=torch.uint8, device=x.device)
    launch.Launcher(x.device).pca_moments(x, N, d, mean, cov, ws)
    return mean, cov


def pca_eigh(cov):
    """symmetric positive semi-definite cov [d x d] float64 -> (evals [d] descending, clamped at 0; evecs [d x d], row i =
    component i, its entry of largest magnitude positive; info float64 [4] = (sweeps run, converged, the largest
    |g_p . g_q| / (|g_p| |g_q|) met in the last sweep, trace)).  Nothing is read back here: a matrix that did not converge
    within pca_max_sweeps() sweeps says so in info[1]."""
    _need_cuda(cov)
    if cov.dim() != 2 or cov.shape[0] != cov.shape[1]:
        raise _lib.EvaeError("pca_eigh: a square matrix expected, got %s" % (tuple(cov.shape),))
    d = cov.shape[0]
    if not 1 <= d <= pca_max_features():
        raise _lib.EvaeError("pca_eigh: d=%d outside [1, %d]" % (d, pca_max_features()))
    _dev_tensor("cov", cov, torch.float64, (d, d), "pca_eigh")
    evals = torch.empty(d, dtype=torch.float64, device=cov.device)
    evecs = torch.empty((d, d), dtype=torch.float64, device=cov.device)
    info = torch.empty(4, dtype=torch.float64, device=cov.device)
    nbytes = _lib.load().evae_pca_eigh_workspace_bytes(d)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cov.device) if nbytes else None
    launch.Launcher(cov.device).pca_eigh(cov, d, evals, evecs, info, ws)
    return evals, evecs, info


def pca_project(x, mean, comps, scale=1.0):
    """out [N x k] float32 = scale (x - mean) comps^T: x [N x d], mean [d] and comps [k x d] float64, 1 <= k <= d; accumulated
    in fp64, rounded once"""
    _need_cuda(x, mean, comps)
    x = _f32(x)
    N, d = _dev_rows("x", x, "pca_project", pca_max_features(), pca_max_points())
    if comps.dim() != 2 or not 1 <= comps.shape[0] <= d:
        raise _lib.EvaeError("pca_project: comps must be [k x %d] with 1 <= k <= %d, got %s" % (d, d, tuple(comps.shape)))
    k = comps.shape[0]
    _dev_tensor("mean", mean, torch.float64, (d,), "pca_project")
    _dev_tensor("comps", comps, torch.float64, (k, d), "pca_project")
    out = torch.empty((N, k), device=x.device)
    launch.Launcher(x.device).pca_project(x, N, d, mean, comps, k, scale, out)
    return out


def pca_reconstruct(y, mean, comps):
    """out [N x d] float32 = mean + y comps: y [N x k], the reverse map of pca_project at scale 1"""
    _need_cuda(y, mean, comps)
    y = _f32(y)
    N, k = _dev_rows("y", y, "pca_reconstruct", pca_max_features(), pca_max_points())
    if comps.dim() != 2 or comps.shape[0] != k or not k <= comps.shape[1] <= pca_max_features():
        raise _lib.EvaeError("pca_reconstruct: comps must be [%d x d] with %d <= d <= %d, got %s"
                             % (k, k, pca_max_features(), tuple(comps.shape)))
    d = comps.shape[1]
    _dev_tensor("mean", mean, torch.float64, (d,), "pca_reconstruct")
    _dev_tensor("comps", comps, torch.float64, (k, d), "pca_reconstruct")
    out = torch.empty((N, d), device=y.device)
    launch.Launcher(y.device).pca_reconstruct(y, N, k, mean, comps, d, out)
    return out


# ------------------------------------------------------------------------------------------------
# k-means and clustering scores in fp64 (csrc/evae_kmeans.hip); the driver is evae/cluster.py.  These take what the
# kernels take and convert nothing: a wrong dtype or a strided tensor is refused, not copied.
# ------------------------------------------------------------------------------------------------
KMEANS_STATE = 8     # the record of kmeans_step: iterations, done, labels changed, shift, inertia, relocations, of this step, 0


def kmeans_max_clusters():
    return int(_lib.load().evae_kmeans_max_clusters())


def kmeans_max_features():
    return int(_lib.load().evae_kmeans_max_features())


def kmeans_max_points():
    return int(_lib.load().evae_kmeans_max_points())


def kmeans_chunk_rows():
    """rows of a histogram chunk and positions of a segment of the sorted order"""
    return int(_lib.load().evae_kmeans_chunk_rows())


def kmeans_centre_tile():
    """centres that pass through LDS together in kmeans_assign"""
    return int(_lib.load().evae_kmeans_centre_tile())


def _km_clusters(K, who, N=None):
    K = int(K)
    if not 1 <= K <= kmeans_max_clusters() or (N is not None and K > N):
        raise _lib.EvaeError("%s: K=%d outside [1, min(N, %d)]" % (who, K, kmeans_max_clusters()))
    return K


def _km_centres(centres, d, who, N=None):
    """centres float64 [K x d] (K <= N where N is given) -> K"""
    _need_cuda(centres)
    if centres.dim() != 2:
        raise _lib.EvaeError("%s: centres must be [K x %d], got %s" % (who, d, tuple(centres.shape)))
    K = _km_clusters(centres.shape[0], who, N)
    _dev_tensor("centres", centres, torch.float64, (K, d), who)
    return K


def kmeans_workspace(N, d, K, device):
    """the one workspace of the kmeans_* entries for these sizes (a uint8 tensor)"""
    return torch.empty(_lib.load().evae_kmeans_workspace_bytes(N, d, K), dtype=torch.uint8, device=device)


def kmeans_assign(x, centres):
    """x [N x d] float32, centres [K x d] float64 -> (labels int32 [N], d2 float64 [N]): the nearest centre by
    sum_k (x_ik - c_jk)^2 in fp64, k ascending, ties to the lowest index; d2 is the winning sum"""
    N, d = _dev_rows("x", x, "kmeans_assign", kmeans_max_features(), kmeans_max_points())
    K = _km_centres(centres, d, "kmeans_assign")
    labels = torch.empty(N, dtype=torch.int32, device=x.device)
    d2 = torch.empty(N, dtype=torch.float64, device=x.device)
    launch.Launcher(x.device).kmeans_assign(x, N, d, centres, K, labels, d2)
    return labels, d2


def kmeans_transform(x, centres):
    """x [N x d] float32, centres [K x d] float64 -> float32 [N x K]: the distances (not squared) to every centre, the sums of
    kmeans_assign, one square root and one rounding each"""
    N, d = _dev_rows("x", x, "kmeans_transform", kmeans_max_features(), kmeans_max_points())
    K = _km_centres(centres, d, "kmeans_transform")
    out = torch.empty((N, K), dtype=torch.float32, device=x.device)
    launch.Launcher(x.device).kmeans_transform(x, N, d, centres, K, out)
    return out


def kmeans_update(x, labels, K, ws=None):
    """x [N x d], labels int32 [N] in [0, K) -> (order int32 [N], start int32 [K + 1], sums float64 [K x d]): the stable counting
    sort of the rows by label (cluster c owns order[start[c] : start[c + 1]], in index order) and the fp64 column sums of every
    cluster in a fixed order.  A label outside [0, K) is left out of all three (labels are trusted, the kernels only guard)."""
    N, d = _dev_rows("x", x, "kmeans_update", kmeans_max_features(), kmeans_max_points())
    K = _km_clusters(K, "kmeans_update")
    _dev_tensor("labels", labels, torch.int32, (N,), "kmeans_update")
    order = torch.empty(N, dtype=torch.int32, device=x.device)
    start = torch.empty(K + 1, dtype=torch.int32, device=x.device)
    sums = torch.empty((K, d), dtype=torch.float64, device=x.device)
    ws = kmeans_workspace(N, d, K, x.device) if ws is None else ws
    launch.Launcher(x.device).kmeans_update(x, N, d, labels, K, order, start, sums, ws)
    return order, start, sums


def kmeans_state(device):
    """a zeroed record for kmeans_step"""
    return torch.zeros(KMEANS_STATE, dtype=torch.float64, device=device)


def kmeans_step(x, centres, labels, d2, order, start, tol_abs, state, ws):
    """One Lloyd iteration in place (assign + update + finish on the current stream): centres [K x d] float64 are replaced by
    the means of their clusters, labels / d2 / order / start belong to the centres that came in, state (kmeans_state) is advanced.
    Once state[1] (done) is set, further calls change nothing: a caller may issue several and read the record once."""
    N, d = _dev_rows("x", x, "kmeans_step", kmeans_max_features(), kmeans_max_points())
    K = _km_centres(centres, d, "kmeans_step", N)
    _dev_tensor("labels", labels, torch.int32, (N,), "kmeans_step")
    _dev_tensor("d2", d2, torch.float64, (N,), "kmeans_step")
    _dev_tensor("order", order, torch.int32, (N,), "kmeans_step")
    _dev_tensor("start", start, torch.int32, (K + 1,), "kmeans_step")
    _dev_tensor("state", state, torch.float64, (KMEANS_STATE,), "kmeans_step")
    _need_cuda(ws)
    if not float(tol_abs) >= 0.0:
        raise _lib.EvaeError("kmeans_step: tol_abs=%r" % (tol_abs,))
    launch.Launcher(x.device).kmeans_step(x, N, d, K, centres, labels, d2, order, start, tol_abs, state, ws)


def kmeans_seed(x, K, u, ws=None):
    """k-means++ by D^2 sampling from the caller's uniforms: x [N x d], u float64 [K] in [0, 1) -> (idx int32 [K], centres
    float64 [K x d] = x[idx]).  The first pick is min(floor(u_0 N), N - 1); pick t is the first row whose running sum of
    min-distances (chunks in order, rows in order) exceeds u_t times their total; when the total is 0 (fewer distinct rows than
    centres) it is the lowest index not chosen yet.  scikit-learn's greedy local trials are not carried over: one candidate per
    centre."""
    N, d = _dev_rows("x", x, "kmeans_seed", kmeans_max_features(), kmeans_max_points())
    K = _km_clusters(K, "kmeans_seed", N)
    _dev_tensor("u", u, torch.float64, (K,), "kmeans_seed")
    idx = torch.empty(K, dtype=torch.int32, device=x.device)
    centres = torch.empty((K, d), dtype=torch.float64, device=x.device)
    ws = kmeans_workspace(N, d, K, x.device) if ws is None else ws
    launch.Launcher(x.device).kmeans_seed(x, N, d, K, u, idx, centres, ws)
    return idx, centres


def kmeans_inertia(d2):
    """d2 float64 [N] -> float64 [1]: the sum, chunk sums added in chunk order"""
    _need_cuda(d2)
    if d2.dim() != 1 or not 1 <= d2.shape[0] <= kmeans_max_points():
        raise _lib.EvaeError("kmeans_inertia: d2 must be [N], N in [1, %d], got %s" % (kmeans_max_points(), tuple(d2.shape)))
    N = d2.shape[0]
    _dev_tensor("d2", d2, torch.float64, (N,), "kmeans_inertia")
    out = torch.empty(1, dtype=torch.float64, device=d2.device)
    ws = torch.empty(8 * ((N + kmeans_chunk_rows() - 1) // kmeans_chunk_rows()), dtype=torch.uint8, device=d2.device)
    launch.Launcher(d2.device).kmeans_inertia(d2, N, out, ws)
    return out


def cluster_contingency(a, Ka, b, Kb):
    """a, b int32 [N] with values in [0, Ka) and [0, Kb) -> table int64 [Ka x Kb], table[i][j] = #{n : a_n = i, b_n = j}"""
    _need_cuda(a, b)
    if a.dim() != 1 or not 1 <= a.shape[0] <= kmeans_max_points():
        raise _lib.EvaeError("cluster_contingency: a must be [N], N in [1, %d], got %s" % (kmeans_max_points(), tuple(a.shape)))
    N = a.shape[0]
    _dev_tensor("a", a, torch.int32, (N,), "cluster_contingency")
    _dev_tensor("b", b, torch.int32, (N,), "cluster_contingency")
    Ka, Kb = _km_clusters(Ka, "cluster_contingency"), _km_clusters(Kb, "cluster_contingency")
    table = torch.empty((Ka, Kb), dtype=torch.int64, device=a.device)
    launch.Launcher(a.device).cluster_contingency(a, Ka, b, Kb, N, table)
    return table


CLUSTER_SCORES = ("entropy_a", "entropy_b", "mutual_info", "nmi", "ari", "purity", "n_samples")


def cluster_scores(table):
    """table int64 [Ka x Kb] -> float64 [8] = (H(a), H(b), MI, NMI with the arithmetic mean, ARI, purity = sum_j max_i n_ij / N,
    N, 0), natural logarithms; one non-empty row and one non-empty column give NMI = ARI = 1"""
    _need_cuda(table)
    if table.dim() != 2:
        raise _lib.EvaeError("cluster_scores: a [Ka x Kb] table expected, got %s" % (tuple(table.shape),))
    Ka, Kb = _km_clusters(table.shape[0], "cluster_scores"), _km_clusters(table.shape[1], "cluster_scores")
    _dev_tensor("table", table, torch.int64, (Ka, Kb), "cluster_scores")
    out = torch.empty(8, dtype=torch.float64, device=table.device)
    launch.Launcher(table.device).cluster_scores(table, Ka, Kb, out)
    return out


def silhouette_samples(x, order, start, strip_rows=0):
    """x [N x d], (order, start) of kmeans_update -> float64 [N]: s_i = (b_i - a_i) / max(a_i, b_i), a_i the mean distance to the
    rest of i's cluster, b_i the smallest mean distance to another non-empty cluster; 0 for a singleton and for max(a, b) = 0.
    Distances are sqrt of pairwise_distance's squared ones, strip by strip (strip_rows query rows, 0: what fits 256 MiB); the
    result does not depend on strip_rows."""
    N, d = _dev_rows("x", x, "silhouette_samples", kmeans_max_features(), tsne_nn_max_points())
    if N < 2:
        raise _lib.EvaeError("silhouette_samples: N=%d, at least 2 rows expected" % N)
    _need_cuda(start)
    if start.dim() != 1 or not 2 <= start.shape[0] <= N + 1:
        raise _lib.EvaeError("silhouette_samples: start must be [K + 1] with 1 <= K <= N=%d, got %s" % (N, tuple(start.shape)))
    K = start.shape[0] - 1
    _dev_tensor("order", order, torch.int32, (N,), "silhouette_samples")
    _dev_tensor("start", start, torch.int32, (K + 1,), "silhouette_samples")
    strip_rows = _strip_rows(strip_rows, "silhouette_samples")
    out = torch.zeros(N, dtype=torch.float64, device=x.device)
    ws = torch.empty(_lib.load().evae_silhouette_workspace_bytes(N, d, strip_rows), dtype=torch.uint8, device=x.device)
    launch.Launcher(x.device).silhouette_samples(x, N, d, order, start, K, out, ws, strip_rows)
    return out


# ------------------------------------------------------------------------------------------------
# Gaussian mixture in fp64 (csrc/evae_gmm.hip); the driver is evae/mixture.py.  Like the kmeans_* entries these
# take what the kernels take and convert nothing.  The parameters of a mixture live in ONE float64 buffer (gmm_params) that
# gmm_views slices without copying.
# ------------------------------------------------------------------------------------------------
GMM_STATE = 8        # the record of gmm_step: iterations, done, converged, lower bound, previous lower bound, failed component, 0, 0
GMM_TYPES = {'full': 0, 'diag': 1, 'spherical': 2}


def gmm_max_components():
    return int(_lib.load().evae_gmm_max_components())


def gmm_max_features(covariance_type='full'):
    """96 for 'full' (the factor of a component lives in LDS), 256 for 'diag' and 'spherical'"""
    return int(_lib.load().evae_gmm_max_features(GMM_TYPES[covariance_type]))


def gmm_max_points():
    return int(_lib.load().evae_gmm_max_points())


def gmm_chunk_rows():
    """rows whose weighted sums are formed together in the M-step"""
    return int(_lib.load().evae_gmm_chunk_rows())


def gmm_strip_rows():
    """rows a block of the E-step owns"""
    return int(_lib.load().evae_gmm_strip_rows())


def gmm_max_bytes():
    """log_resp plus workspace may not exceed this"""
    return int(_lib.load().evae_gmm_max_bytes())


def gmm_workspace_bytes(N, d, K, covariance_type):
    return int(_lib.load().evae_gmm_workspace_bytes(int(N), int(d), int(K), GMM_TYPES[covariance_type]))


def gmm_check_sizes(N, d, K, covariance_type, who):
    """what the kernels refuse, from the sizes alone: before any allocation or launch"""
    if covariance_type not in GMM_TYPES:
        raise _lib.EvaeError("%s: covariance_type=%r; one of %s expected" % (who, covariance_type, sorted(GMM_TYPES)))
    if not 1 <= K <= gmm_max_components():
        raise _lib.EvaeError("%s: K=%d outside [1, %d]" % (who, K, gmm_max_components()))
    if not 1 <= d <= gmm_max_features(covariance_type):
        raise _lib.EvaeError("%s: %d features outside [1, %d] for covariance_type=%r" % (who, d, gmm_max_features(covariance_type),
                                                                                        covariance_type))
    if N is None:
        return
    if not 1 <= N <= gmm_max_points():
        raise _lib.EvaeError("%s: N=%d outside [1, %d]" % (who, N, gmm_max_points()))
    resp, ws = 8 * N * K, gmm_workspace_bytes(N, d, K, covariance_type)
    if resp + ws > gmm_max_bytes():
        raise _lib.EvaeError("%s: log_resp of %d bytes plus a workspace of %d bytes for N=%d, d=%d, K=%d exceed %d bytes"
                             % (who, resp, ws, N, d, K, gmm_max_bytes()))


def gmm_params(d, K, covariance_type, device):
    """an uninitialised parameter buffer (float64) for these sizes"""
    gmm_check_sizes(None, d, K, covariance_type, "gmm_params")
    n = _lib.load().evae_gmm_params_doubles(int(d), int(K), GMM_TYPES[covariance_type])
    return torch.empty(n, dtype=torch.float64, device=device)


def gmm_views(params, d, K, covariance_type):
    """-> dict of views into a parameter buffer: weights [K], nk [K], log_det [K], means [K x d], b [K x d], covariances and
    precisions_cholesky ([K x d x d], [K x d] or [K])"""
    cs = {'full': d * d, 'diag': d, 'spherical': 1}[covariance_type]
    shape = {'full': (K, d, d), 'diag': (K, d), 'spherical': (K,)}[covariance_type]
    o = 3 * K
    return dict(weights=params[0:K], nk=params[K:2 * K], log_det=params[2 * K:3 * K], means=params[o:o + K * d].view(K, d),
                b=params[o + K * d:o + 2 * K * d].view(K, d), covariances=params[o + 2 * K * d:o + 2 * K * d + K * cs].view(shape),
                precisions_cholesky=params[o + 2 * K * d + K * cs:o + 2 * K * d + 2 * K * cs].view(shape))


def _gmm_params(params, d, K, covariance_type, who):
    """`params` must be the one buffer gmm_params lays out for these (already checked) sizes"""
    n = _lib.load().evae_gmm_params_doubles(int(d), int(K), GMM_TYPES[covariance_type])
    _dev_tensor("params", params, torch.float64, (n,), who)


def _gmm_args(x, params, K, covariance_type, who):
    N, d = _dev_rows("x", x, who)                            # the caps depend on the covariance type: gmm_check_sizes
    gmm_check_sizes(N, d, int(K), covariance_type, who)
    _gmm_params(params, d, K, covariance_type, who)
    return N, d, int(K), GMM_TYPES[covariance_type]


def gmm_workspace(N, d, K, covariance_type, device):
    """the one workspace of the gmm_* entries for these sizes (a uint8 tensor)"""
    return torch.empty(gmm_workspace_bytes(N, d, K, covariance_type), dtype=torch.uint8, device=device)


def gmm_state(device):
    """a zeroed record for gmm_step / gmm_mstep"""
    return torch.zeros(GMM_STATE, dtype=torch.float64, device=device)


def gmm_estep(x, params, K, covariance_type, ws=None, log_resp=None, logp=None):
    """x [N x d] float32 -> (log_resp float64 [N x K], logp float64 [N] = log p(x_i), mean_logp float64 [1])"""
    N, d, K, t = _gmm_args(x, params, K, covariance_type, "gmm_estep")
    log_resp = torch.empty((N, K), dtype=torch.float64, device=x.device) if log_resp is None else log_resp
    logp = torch.empty(N, dtype=torch.float64, device=x.device) if logp is None else logp
    _dev_tensor("log_resp", log_resp, torch.float64, (N, K), "gmm_estep")
    _dev_tensor("logp", logp, torch.float64, (N,), "gmm_estep")
    mean = torch.empty(1, dtype=torch.float64, device=x.device)
    ws = gmm_workspace(N, d, K, covariance_type, x.device) if ws is None else ws
    _need_cuda(ws)
    launch.Launcher(x.device).gmm_estep(x, N, d, K, t, params, log_resp, logp, mean, ws)
    return log_resp, logp, mean


def gmm_mstep(x, params, K, covariance_type, reg_covar, state, log_resp=None, labels=None, ws=None):
    """The parameters in `params` from responsibilities: log_resp float64 [N x K] (r = exp) or labels int32 [N] (one-hot),
    exactly one of them.  state[5] names the lowest component whose covariance is not positive definite (-1: none)."""
    N, d, K, t = _gmm_args(x, params, K, covariance_type, "gmm_mstep")
    if (log_resp is None) == (labels is None):
        raise _lib.EvaeError("gmm_mstep: exactly one of log_resp and labels expected")
    if log_resp is not None:
        _dev_tensor("log_resp", log_resp, torch.float64, (N, K), "gmm_mstep")
    else:
        _dev_tensor("labels", labels, torch.int32, (N,), "gmm_mstep")
    _dev_tensor("state", state, torch.float64, (GMM_STATE,), "gmm_mstep")
    if not float(reg_covar) >= 0.0:
        raise _lib.EvaeError("gmm_mstep: reg_covar=%r" % (reg_covar,))
    ws = gmm_workspace(N, d, K, covariance_type, x.device) if ws is None else ws
    _need_cuda(ws)
    launch.Launcher(x.device).gmm_mstep(x, N, d, K, t, log_resp, labels, reg_covar, params, state, ws)


def gmm_step(x, params, K, covariance_type, log_resp, logp, reg_covar, tol, state, ws):
    """One EM iteration in place (E-step, M-step, record: six launches on the current stream).  Once state[1] (done) is set,
    further calls change nothing: a caller may issue several and read the record once."""
    N, d, K, t = _gmm_args(x, params, K, covariance_type, "gmm_step")
    _dev_tensor("log_resp", log_resp, torch.float64, (N, K), "gmm_step")
    _dev_tensor("logp", logp, torch.float64, (N,), "gmm_step")
    _dev_tensor("state", state, torch.float64, (GMM_STATE,), "gmm_step")
    _need_cuda(ws)
    if not float(reg_covar) >= 0.0 or not float(tol) >= 0.0:
        raise _lib.EvaeError("gmm_step: reg_covar=%r, tol=%r" % (reg_covar, tol))
    launch.Launcher(x.device).gmm_step(x, N, d, K, t, params, log_resp, logp, reg_covar, tol, state, ws)


def gmm_prepare(params, d, K, covariance_type):
    """b = mu P and log_det = sum log diag P from the means and factors already in params"""
    gmm_check_sizes(None, d, int(K), covariance_type, "gmm_prepare")
    _gmm_params(params, d, K, covariance_type, "gmm_prepare")
    launch.Launcher(params.device).gmm_prepare(params, int(d), int(K), GMM_TYPES[covariance_type])


def gmm_argmax(log_resp):
    """float64 [N x K] -> int32 [N]: the first of the largest entries of every row"""
    _need_cuda(log_resp)
    if log_resp.dim() != 2 or not 1 <= log_resp.shape[0] <= gmm_max_points() or not 1 <= log_resp.shape[1] <= gmm_max_components():
        raise _lib.EvaeError("gmm_argmax: log_resp must be [N x K] within the caps, got %s" % (tuple(log_resp.shape),))
    N, K = log_resp.shape
    _dev_tensor("log_resp", log_resp, torch.float64, (N, K), "gmm_argmax")
    labels = torch.empty(N, dtype=torch.int32, device=log_resp.device)
    launch.Launcher(log_resp.device).gmm_argmax(log_resp, N, K, labels)
    return labels


def gmm_sample(params, d, K, covariance_type, comp, eps):
    """comp int32 [n] in [0, K), eps float64 [n x d] standard normals -> float32 [n x d]: mu_c + (P_c^T)^-1 eps"""
    gmm_check_sizes(None, d, int(K), covariance_type, "gmm_sample")
    _gmm_params(params, d, K, covariance_type, "gmm_sample")
    _need_cuda(comp, eps)
    if comp.dim() != 1 or not 1 <= comp.shape[0] <= gmm_max_points():
        raise _lib.EvaeError("gmm_sample: comp must be [n], n in [1, %d], got %s" % (gmm_max_points(), tuple(comp.shape)))
    n = comp.shape[0]
    _dev_tensor("comp", comp, torch.int32, (n,), "gmm_sample")
    _dev_tensor("eps", eps, torch.float64, (n, d), "gmm_sample")
    z = torch.empty((n, d), dtype=torch.float32, device=params.device)
    launch.Launcher(params.device).gmm_sample(params, int(d), int(K), GMM_TYPES[covariance_type], comp, eps, n, z)
    return z


# ------------------------------------------------------------------------------------------------
# Aggregate posterior in fp64 (csrc/evae_agg_lse.hip); the driver is evae/latent_info.py.  Takes what the kernels
# take and converts nothing.
# ------------------------------------------------------------------------------------------------
AggPosteriorLse = collections.namedtuple("AggPosteriorLse", "log_q log_qd log_cond")


def agg_lse_max_features():
    return int(_lib.load().evae_agg_lse_max_features())


def agg_lse_max_points():
    return int(_lib.load().evae_agg_lse_max_points())


def agg_lse_tile():
    """components of one (maximum, sum) pair of the log-sum-exp: a constant of the kernels"""
    return int(_lib.load().evae_agg_lse_tile())


def _agg_rows(name, t):
    _need_cuda(t)
    if t.dim() != 2 or t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError("agg_posterior_lse: %s must be a contiguous float32 [rows x d] tensor, got %s %s%s"
                         % (name, t.dtype, tuple(t.shape), "" if t.is_contiguous() else " (strided)"))
    return t.shape


def agg_posterior_lse(z, mean, log_var, rows=None, joint=True, per_dimension=True):
    """z [B x d], mean and log_var [N x d], all float32 -> AggPosteriorLse(log_q [B], log_qd [B x d], log_cond [B x d]), float64
    on the device, of q(z) = 1/N sum_j N(z; mean_j, diag exp(log_var_j)): the joint log-density (joint), the log-density of
    every dimension's marginal (per_dimension) and, with rows int32 [B], log N(z_id; mean_{rows[i] d}, exp(log_var_{rows[i] d})).
    What is switched off is None.  rows is checked here (one read of its extremes): outside [0, N) is a ValueError."""
    (B, d), (N, dm) = _agg_rows("z", z), _agg_rows("mean", mean)
    if tuple(_agg_rows("log_var", log_var)) != (N, dm):
        raise ValueError("agg_posterior_lse: mean is %s, log_var %s" % (tuple(mean.shape), tuple(log_var.shape)))
    if d != dm or not 1 <= d <= agg_lse_max_features():
        raise ValueError("agg_posterior_lse: z has %d features, mean %d (equal and in [1, %d] expected)" % (d, dm, agg_lse_max_features()))
    cap = agg_lse_max_points()
    if not 1 <= B <= cap or not 1 <= N <= cap:
        raise ValueError("agg_posterior_lse: B=%d, N=%d outside [1, %d]" % (B, N, cap))
    if rows is not None:
        _need_cuda(rows)
        if rows.dtype != torch.int32 or not rows.is_contiguous() or tuple(rows.shape) != (B,):
            raise ValueError("agg_posterior_lse: rows must be a contiguous int32 [%d] tensor, got %s %s" % (B, rows.dtype, tuple(rows.shape)))
        lo, hi = torch.stack((rows.min(), rows.max())).tolist()
        if lo < 0 or hi >= N:
            raise ValueError("agg_posterior_lse: rows span [%d, %d], outside [0, %d)" % (lo, hi, N))
    if not (joint or per_dimension or rows is not None):
        raise ValueError("agg_posterior_lse: no output asked for (joint=False, per_dimension=False, rows=None)")
    dev = z.device
    log_q = torch.empty(B, dtype=torch.float64, device=dev) if joint else None
    log_qd = torch.empty((B, d), dtype=torch.float64, device=dev) if per_dimension else None
    log_cond = torch.empty((B, d), dtype=torch.float64, device=dev) if rows is not None else None
    ws = torch.empty(_lib.load().evae_agg_lse_workspace_bytes(B, N, d), dtype=torch.uint8, device=dev)
    launch.Launcher(dev).agg_lse(z, B, mean, log_var, N, d, rows, log_q, log_qd, log_cond, ws)
    return AggPosteriorLse(log_q, log_qd, log_cond)


# ------------------------------------------------------------------------------------------------
# Kernel sums in fp64 (csrc/evae_kernel_sum.hip); the driver is evae/sample_quality.py (kernel_mmd,
# frechet_distance).  Rows are taken as float32 (converted like pca_moments does); the fp64 operands are converted by nobody.
# ------------------------------------------------------------------------------------------------
KERNEL_KINDS = {'poly': 0, 'rbf': 1}     # EVAE_KERNEL_POLY, EVAE_KERNEL_RBF


def kernel_sum_tile():
    """columns of one tile of kernel_row_sums: a tile's terms are added in index order, the tiles in order; a constant"""
    return int(_lib.load().evae_kernel_sum_tile())


def kernel_sum_max_features():
    return int(_lib.load().evae_kernel_sum_max_features())


def kernel_sum_max_points():
    return int(_lib.load().evae_kernel_sum_max_points())


def kernel_sum_max_degree():
    return int(_lib.load().evae_kernel_sum_max_degree())


def kernel_sum_check(kind, degree, coef0, who, name="kind"):
    """the kernel's own arguments, checked without a tensor in sight (kernel_mmd asks before it launches anything): a kind
    that is not 'poly' or 'rbf', and for 'poly' a degree that is not an integer in [1, kernel_sum_max_degree()] or a coef0
    that is not a number, are ValueErrors"""
    if kind not in KERNEL_KINDS:
        raise ValueError("%s: %s=%r, 'poly' or 'rbf' expected" % (who, name, kind))
    if kind != 'poly':
        return
    top = kernel_sum_max_degree()
    if isinstance(degree, bool) or not isinstance(degree, (int, float)) or degree != int(degree) or not 1 <= degree <= top:
        raise ValueError("%s: degree=%r, an integer in [1, %d] expected" % (who, degree, top))
    if isinstance(coef0, bool) or not isinstance(coef0, (int, float)):
        raise ValueError("%s: coef0=%r, a number expected" % (who, coef0))


def _ks_rows(name, t):
    _need_cuda(t)
    if t.dim() != 2 or not t.is_floating_point():
        raise ValueError("kernel_row_sums: %s must be a floating-point [rows x d] tensor, got %s %s" % (name, t.dtype, tuple(t.shape)))
    return _f32(t)


def kernel_row_sums(q, c, kind='poly', gamma=None, coef0=1.0, degree=3, skip_self=False):
    """q [B x d], c [N x d] -> float64 [B]: row_sum[i] = sum_j k(q_i, c_j) in fp64, j ascending (tiles of kernel_sum_tile()
    columns, a tile's terms in index order, the tiles in order).  kind 'poly': (gamma <q_i, c_j> + coef0)^degree, degree an
    integer in [1, 8]; 'rbf': exp(-gamma |q_i - c_j|^2) from direct differences.  gamma=None: 1 / d.  skip_self (the
    within-set form, B == N) leaves the term j == i out by index.  Equal inputs give bit-equal outputs; a row's bits do not
    depend on the batch it is in.  d <= kernel_sum_max_features() = 256: the kernel keeps a wave's 64 query rows in LDS whole
    (d x 256 bytes beside the staged columns); wider rows, the 784 pixels for one, would need the query staged in chunks of
    features as the columns are, which this kernel does not do."""
    q, c = _ks_rows("q", q), _ks_rows("c", c)
    (B, d), (N, dc) = q.shape, c.shape
    if d != dc:
        raise ValueError("kernel_row_sums: q has %d features, c %d" % (d, dc))
    if not 1 <= d <= kernel_sum_max_features():
        raise ValueError("kernel_row_sums: q and c have %d features, outside [1, %d]" % (d, kernel_sum_max_features()))
    cap = kernel_sum_max_points()
    if not 1 <= B <= cap:
        raise ValueError("kernel_row_sums: q has %d rows, outside [1, %d]" % (B, cap))
    if not 1 <= N <= cap:
        raise ValueError("kernel_row_sums: c has %d rows, outside [1, %d]" % (N, cap))
    kernel_sum_check(kind, degree, coef0, "kernel_row_sums")
    if skip_self and B != N:
        raise ValueError("kernel_row_sums: skip_self with %d rows in q and %d in c (the within-set form needs B == N)" % (B, N))
    if gamma is not None and (isinstance(gamma, bool) or not isinstance(gamma, (int, float))):
        raise ValueError("kernel_row_sums: gamma=%r, a number or None (1 / d) expected" % (gamma,))
    gamma = 1.0 / d if gamma is None else float(gamma)
    row_sum = torch.empty(B, dtype=torch.float64, device=q.device)
    launch.Launcher(q.device).kernel_row_sums(q, B, c, N, d, KERNEL_KINDS[kind], gamma, coef0, int(degree) if kind == 'poly' else 1,
                                              skip_self, row_sum)
    return row_sum


def ordered_sum(x):
    """x float64 [n] -> float64 0-d tensor on the device: x[0] + x[1] + .. from left to right, one workgroup, bit-reproducible"""
    _need_cuda(x)
    if x.dim() != 1 or x.dtype != torch.float64 or not x.is_contiguous():
        raise ValueError("ordered_sum: x must be a contiguous float64 [n] tensor, got %s %s" % (x.dtype, tuple(x.shape)))
    n = x.shape[0]
    if not 1 <= n <= kernel_sum_max_points():
        raise ValueError("ordered_sum: x has %d entries, outside [1, %d]" % (n, kernel_sum_max_points()))
    out = torch.empty(1, dtype=torch.float64, device=x.device)
    launch.Launcher(x.device).ordered_sum(x, n, out)
    return out[0]


def sym_congruence(A, S):
    """A, S float64 [d x d], S symmetric -> A S A^T float64 [d x d], symmetric bit for bit: T = A S, then T A^T, every entry's
    sum in ascending index; d <= kernel_sum_max_features()"""
    _need_cuda(A, S)
    if A.dim() != 2 or A.shape[0] != A.shape[1] or A.dtype != torch.float64 or not A.is_contiguous():
        raise ValueError("sym_congruence: A must be a contiguous float64 [d x d] tensor, got %s %s" % (A.dtype, tuple(A.shape)))
    d = A.shape[0]
    if not 1 <= d <= kernel_sum_max_features():
        raise ValueError("sym_congruence: A is [%d x %d], d outside [1, %d]" % (d, d, kernel_sum_max_features()))
    if tuple(S.shape) != (d, d) or S.dtype != torch.float64 or not S.is_contiguous():
        raise ValueError("sym_congruence: S must be a contiguous float64 [%d x %d] tensor, got %s %s" % (d, d, S.dtype, tuple(S.shape)))
    out = torch.empty((d, d), dtype=torch.float64, device=A.device)
    ws = torch.empty(_lib.load().evae_sym_congruence_workspace_bytes(d), dtype=torch.uint8, device=A.device)
    launch.Launcher(A.device).sym_congruence(A, S, out, d, ws)
    return out


# ------------------------------------------------------------------------------------------------
# Linear probe in fp64 (csrc/evae_logreg.hip); the driver is evae/linear.py.  Like the gmm_* entries these take
# what the kernels take and convert nothing.  The vectors of the solver live in ONE float64 buffer (logreg_solver) that
# logreg_views slices without copying; W is [K x p] with the intercept column last (p = d + 1, or d without an intercept).
# ------------------------------------------------------------------------------------------------
LOGREG_STATE = 8     # the record: iterations, done, converged, f, t, j, line search failed, G.D


def logreg_max_classes():
    return int(_lib.load().evae_logreg_max_classes())


def logreg_max_features():
    return int(_lib.load().evae_logreg_max_features())


def logreg_max_points():
    return int(_lib.load().evae_logreg_max_points())


def logreg_max_history():
    return int(_lib.load().evae_logreg_max_history())


def logreg_max_line_steps():
    return int(_lib.load().evae_logreg_max_line_steps())


def logreg_chunk_rows():
    """rows whose losses and gradient sums are formed together"""
    return int(_lib.load().evae_logreg_chunk_rows())


def logreg_max_bytes():
    """Z and Z_D plus workspace may not exceed this"""
    return int(_lib.load().evae_logreg_max_bytes())


def logreg_workspace_bytes(N, d, K, fit_intercept, line_steps):
    return int(_lib.load().evae_logreg_workspace_bytes(int(N), int(d), int(K), int(bool(fit_intercept)), int(line_steps)))


def logreg_check_sizes(N, d, K, fit_intercept, history, line_steps, who):
    """what the kernels refuse, from the sizes alone: before any allocation or launch (N None: the shape of W only)"""
    if not 2 <= K <= logreg_max_classes():
        raise _lib.EvaeError("%s: K=%d outside [2, %d]" % (who, K, logreg_max_classes()))
    if not 1 <= d <= logreg_max_features():
        raise _lib.EvaeError("%s: %d features outside [1, %d]" % (who, d, logreg_max_features()))
    if not 1 <= history <= logreg_max_history():
        raise _lib.EvaeError("%s: history=%d outside [1, %d]" % (who, history, logreg_max_history()))
    if not 1 <= line_steps <= logreg_max_line_steps():
        raise _lib.EvaeError("%s: line_steps=%d outside [1, %d]" % (who, line_steps, logreg_max_line_steps()))
    if N is None:
        return
    if not 1 <= N <= logreg_max_points():
        raise _lib.EvaeError("%s: N=%d outside [1, %d]" % (who, N, logreg_max_points()))
    z, ws = 8 * N * K, logreg_workspace_bytes(N, d, K, fit_intercept, line_steps)
    if 2 * z + ws > logreg_max_bytes():
        raise _lib.EvaeError("%s: Z and Z_D of %d bytes each plus a workspace of %d bytes for N=%d, d=%d, K=%d exceed %d bytes"
                             % (who, z, ws, N, d, K, logreg_max_bytes()))


def _logreg_p(d, fit_intercept):
    return int(d) + (1 if fit_intercept else 0)


def logreg_solver(d, K, fit_intercept, history, device):
    """a zeroed solver buffer (float64) for these sizes"""
    logreg_check_sizes(None, d, K, fit_intercept, history, 1, "logreg_solver")
    n = _lib.load().evae_logreg_solver_doubles(int(d), int(K), int(bool(fit_intercept)), int(history))
    return torch.zeros(n, dtype=torch.float64, device=device)


def logreg_views(solver, d, K, fit_intercept, history):
    """-> dict of views into a solver buffer: G, Q, D [K x p]; S, Y [m x K x p]; sy, yy, alpha [m]; scal [8] (pairs held, next
    slot, max|G| / N, ww)"""
    p, m = _logreg_p(d, fit_intercept), int(history)
    L = K * p
    o = 3 * L + 2 * m * L
    return dict(G=solver[0:L].view(K, p), Q=solver[L:2 * L].view(K, p), D=solver[2 * L:3 * L].view(K, p),
                S=solver[3 * L:3 * L + m * L].view(m, K, p), Y=solver[3 * L + m * L:o].view(m, K, p), sy=solver[o:o + m],
                yy=solver[o + m:o + 2 * m], alpha=solver[o + 2 * m:o + 3 * m], scal=solver[o + 3 * m:o + 3 * m + 8])


def logreg_workspace(N, d, K, fit_intercept, line_steps, device):
    """the one workspace of the logreg_* entries for these sizes (a uint8 tensor)"""
    return torch.empty(logreg_workspace_bytes(N, d, K, fit_intercept, line_steps), dtype=torch.uint8, device=device)


def logreg_workspace_views(ws, N, d, K, fit_intercept, line_steps):
    """-> dict of float64 views into a workspace: partial [chunks x K x p] (the gradient sums of the chunks), loss [chunks],
    line [chunks x line_steps] (the trial losses of the chunks); each part starts on a 256-byte boundary"""
    p, chunks = _logreg_p(d, fit_intercept), (N + logreg_chunk_rows() - 1) // logreg_chunk_rows()
    up = lambda b: (b + 255) // 256 * 256
    o1 = up(8 * chunks * K * p)
    o2 = o1 + up(8 * chunks)
    f = ws.view(torch.float64) if ws.numel() % 8 == 0 else ws[:ws.numel() // 8 * 8].view(torch.float64)
    return dict(partial=f[0:chunks * K * p].view(chunks, K, p), loss=f[o1 // 8:o1 // 8 + chunks],
                line=f[o2 // 8:o2 // 8 + chunks * line_steps].view(chunks, line_steps))


def logreg_state(device):
    """a zeroed record for logreg_begin / logreg_step"""
    return torch.zeros(LOGREG_STATE, dtype=torch.float64, device=device)


def logreg_check_labels(y, K, who):
    """y int32 [N] on the device: a label outside [0, K) is refused here (one read of two numbers), never met by a kernel"""
    lo, hi = int(y.min().item()), int(y.max().item())
    if lo < 0 or hi >= K:
        raise _lib.EvaeError("%s: labels in [%d, %d], outside [0, %d)" % (who, lo, hi, K))


def _logreg_w(name, W, d, fit_intercept, who):
    _need_cuda(W)
    if W.dim() != 2:
        raise _lib.EvaeError("%s: %s must be [K x p], got %s" % (who, name, tuple(W.shape)))
    K = W.shape[0]
    _dev_tensor(name, W, torch.float64, (K, _logreg_p(d, fit_intercept)), who)
    return K


def _logreg_solver(solver, d, K, fit_intercept, history, who):
    n = _lib.load().evae_logreg_solver_doubles(int(d), int(K), int(bool(fit_intercept)), int(history))
    _dev_tensor("solver", solver, torch.float64, (n,), who)


def logreg_logits(x, W, fit_intercept=True, out=None):
    """x [N x d] float32, W float64 [K x p] -> float64 [N x K]: x_n . w_k by fma in feature order, the intercept last"""
    N, d = _dev_rows("x", x, "logreg_logits", logreg_max_features(), logreg_max_points())
    K = _logreg_w("W", W, d, fit_intercept, "logreg_logits")
    logreg_check_sizes(None, d, K, fit_intercept, 1, 1, "logreg_logits")
    out = torch.empty((N, K), dtype=torch.float64, device=x.device) if out is None else out
    _dev_tensor("out", out, torch.float64, (N, K), "logreg_logits")
    launch.Launcher(x.device).logreg_logits(x, N, d, W, K, bool(fit_intercept), out)
    return out


def _logreg_zs(Z, ZD, y, who, labels_checked):
    _need_cuda(Z)
    if Z.dim() != 2:
        raise _lib.EvaeError("%s: Z must be [N x K], got %s" % (who, tuple(Z.shape)))
    N, K = Z.shape
    _dev_tensor("Z", Z, torch.float64, (N, K), who)
    _dev_tensor("ZD", ZD, torch.float64, (N, K), who)
    _dev_tensor("y", y, torch.int32, (N,), who)
    if not labels_checked:
        logreg_check_labels(y, K, who)
    return N, K


def logreg_line(Z, ZD, y, W, d, fit_intercept, solver, history, lam, line_steps, state, ring, ws, labels_checked=False):
    """The line launch: from Z, Z_D, W, the solver's D, state[3] = f and state[7] = G.D the first t = 2^-j, j < line_steps, with
    f(W + t D) <= f + 1e-4 t G.D -> state[4] = t, state[5] = j, ring[state[0]] = j, W += t D in place; none: state[6] = state[1]
    = 1 and W as it was.  The chunks' trial losses stay in the workspace (logreg_workspace_views)."""
    N, K = _logreg_zs(Z, ZD, y, "logreg_line", labels_checked)
    logreg_check_sizes(N, d, K, fit_intercept, history, line_steps, "logreg_line")
    _logreg_w("W", W, d, fit_intercept, "logreg_line")
    _logreg_solver(solver, d, K, fit_intercept, history, "logreg_line")
    _dev_tensor("state", state, torch.float64, (LOGREG_STATE,), "logreg_line")
    if ring is not None:
        _dev_tensor("ring", ring, torch.int32, (ring.numel(),), "logreg_line")
    _need_cuda(ws)
    launch.Launcher(Z.device).logreg_line(Z, ZD, y, N, int(d), K, bool(fit_intercept), W, solver, history, lam, line_steps, state,
                                          ring, ws)


def logreg_grad(x, y, Z, ZD, fit_intercept, line_steps, state, ws, labels_checked=False):
    """The gradient launch: Z += state[4] Z_D in place, R = softmax(Z) - onehot(y) into Z_D, the chunks' sums of R_nk a_nc and
    losses into the workspace"""
    N, d = _dev_rows("x", x, "logreg_grad", logreg_max_features(), logreg_max_points())
    N2, K = _logreg_zs(Z, ZD, y, "logreg_grad", labels_checked)
    if N2 != N:
        raise _lib.EvaeError("logreg_grad: x has %d rows, Z %d" % (N, N2))
    logreg_check_sizes(N, d, K, fit_intercept, 1, line_steps, "logreg_grad")
    _dev_tensor("state", state, torch.float64, (LOGREG_STATE,), "logreg_grad")
    _need_cuda(ws)
    launch.Launcher(x.device).logreg_grad(x, y, N, d, K, bool(fit_intercept), line_steps, Z, ZD, state, ws)


def logreg_finish(N, d, W, fit_intercept, solver, history, lam, tol, line_steps, state, ws):
    """The finish launch: G from the workspace's chunk sums and lam W, the pair, f, the stop, the next D and G.D"""
    K = _logreg_w("W", W, d, fit_intercept, "logreg_finish")
    logreg_check_sizes(N, d, K, fit_intercept, history, line_steps, "logreg_finish")
    _logreg_solver(solver, d, K, fit_intercept, history, "logreg_finish")
    _dev_tensor("state", state, torch.float64, (LOGREG_STATE,), "logreg_finish")
    _need_cuda(ws)
    launch.Launcher(W.device).logreg_finish(int(N), int(d), K, bool(fit_intercept), line_steps, W, solver, history, lam, tol, state, ws)


def logreg_direction(solver, d, K, fit_intercept, history, state):
    """D = -H G by the two-loop recursion over the pairs in the solver, and state[7] = G.D"""
    logreg_check_sizes(None, d, int(K), fit_intercept, history, 1, "logreg_direction")
    _logreg_solver(solver, d, K, fit_intercept, history, "logreg_direction")
    _dev_tensor("state", state, torch.float64, (LOGREG_STATE,), "logreg_direction")
    launch.Launcher(solver.device).logreg_direction(solver, int(d), int(K), bool(fit_intercept), history, state)


def _logreg_fit_args(x, y, W, Z, ZD, fit_intercept, solver, history, line_steps, state, ws, who, labels_checked):
    N, d = _dev_rows("x", x, who, logreg_max_features(), logreg_max_points())
    K = _logreg_w("W", W, d, fit_intercept, who)
    logreg_check_sizes(N, d, K, fit_intercept, history, line_steps, who)
    _dev_tensor("Z", Z, torch.float64, (N, K), who)
    _dev_tensor("ZD", ZD, torch.float64, (N, K), who)
    _dev_tensor("y", y, torch.int32, (N,), who)
    _logreg_solver(solver, d, K, fit_intercept, history, who)
    _dev_tensor("state", state, torch.float64, (LOGREG_STATE,), who)
    _need_cuda(ws)
    if not labels_checked:
        logreg_check_labels(y, K, who)
    return N, d, K


def logreg_begin(x, y, W, Z, ZD, fit_intercept, solver, history, lam, tol, line_steps, state, ws, labels_checked=False):
    """state, solver and the workspace's ticket zeroed, then Z = logits(W), the gradient, f and the first direction at W"""
    N, d, K = _logreg_fit_args(x, y, W, Z, ZD, fit_intercept, solver, history, line_steps, state, ws, "logreg_begin", labels_checked)
    launch.Launcher(x.device).logreg_begin(x, y, N, d, K, bool(fit_intercept), W, Z, ZD, solver, history, lam, tol, line_steps, state, ws)


def logreg_step(x, y, W, Z, ZD, fit_intercept, solver, history, lam, tol, line_steps, state, ring, ws, labels_checked=False):
    """One L-BFGS iteration in place (logits of D, line, gradient, finish: four launches on the current stream), after
    logreg_begin with the same buffers.  Once state[1] (done) is set, further calls change nothing: a caller may issue several
    and read the record once."""
    N, d, K = _logreg_fit_args(x, y, W, Z, ZD, fit_intercept, solver, history, line_steps, state, ws, "logreg_step", labels_checked)
    if ring is not None:
        _dev_tensor("ring", ring, torch.int32, (ring.numel(),), "logreg_step")
    launch.Launcher(x.device).logreg_step(x, y, N, d, K, bool(fit_intercept), W, Z, ZD, solver, history, lam, tol, line_steps, state,
                                          ring, ws)


def logreg_softmax(Z):
    """float64 [N x K] -> (log-probabilities float64 [N x K], labels int32 [N]: the first of the largest entries of every row)"""
    _need_cuda(Z)
    if Z.dim() != 2 or not 1 <= Z.shape[0] <= logreg_max_points() or not 2 <= Z.shape[1] <= logreg_max_classes():
        raise _lib.EvaeError("logreg_softmax: Z must be [N x K] within the caps, got %s" % (tuple(Z.shape),))
    N, K = Z.shape
    _dev_tensor("Z", Z, torch.float64, (N, K), "logreg_softmax")
    logp = torch.empty((N, K), dtype=torch.float64, device=Z.device)
    labels = torch.empty(N, dtype=torch.int32, device=Z.device)
    launch.Launcher(Z.device).logreg_softmax(Z, N, K, logp, labels)
    return logp, labels


# ------------------------------------------------------------------------------------------------
# dense layers
# ------------------------------------------------------------------------------------------------
# The launches of this section go through evae/launch.py's Launcher (workspace names, entry points, the probe's names), built
# where the operator runs: its stream is the one current there.
#
# Weight gradients of thin layers (a contraction over <= 128 batch rows) are leaves of the backward pass: nothing but the optimizer
# reads them, yet each one is a launch on the chain of data gradients (8-15 us apiece in the 2-level model's step, a dozen of them).
# Inside `with ops.deferred_wgrads():` (the captured step and utils.training put it around loss.backward()) such a gradient is only
# ALLOCATED where autograd asks for it and the products are formed behind the backward pass, six jobs per grouped launch
# (evae_dense_bwd_weight_group), on the stream the layer's backward ran on.  Only weights that ONE layer application uses per pass
# qualify (a weight met twice -- q(z2 | x) runs over the exemplar rows and over the batch, through whichever Functions -- has its two
# gradients added by autograd as soon as both exist): the scope walks the loss's autograd graph once and keeps the leaves that
# exactly one edge leads to; a deferred weight that turns up a second time after all is flushed at once with every stream made
# to wait for it.  EVAE_DEFER_WGRAD=0: off.
_DEFER = [None]
_DEFER_ON = os.environ.get("EVAE_DEFER_WGRAD", "1") != "0"


def _flush_wgrads(jobs, everyone_waits=False):
    """launch the pending jobs, grouped by the stream their layer's backward ran on; the current stream (everyone_waits: every
    registered stream) then waits for those launches"""
    cur = torch.cuda.current_stream()
    by_stream = {}
    for j in jobs:
        by_stream.setdefault(j[8].cuda_stream, (j[8], []))[1].append(j)
    for st, js in by_stream.values():
        k = launch.Launcher(js[0][0].device, stream=st)
        for i in range(0, len(js), 6):
            part = js[i:i + 6]
            for j in part:
                if j[9] is not None:               # dw += ...: behind the launch that wrote the other application's gradient
                    st.wait_event(j[9])
            k.bwd_weight_group([(dy, M, N, dy.stride(0), x, K, x.stride(0), dw, db, int(made_ev is not None))
                                for dy, M, N, x, K, dw, db, _key, _st, made_ev in part])
        waiters = [cur]
        if everyone_waits:
            waiters += [s_ for s_ in _SIDE_STREAM_OBJS if s_.cuda_stream != cur.cuda_stream]
        for w_ in waiters:
            if w_.cuda_stream != st.cuda_stream:
                w_.wait_stream(st)


def _single_use_leaves(root):
    """(single, stealable): data pointers of the leaf tensors that exactly ONE edge of root's autograd graph leads to (one layer
    application per pass), and of the leaves whose AccumulateGrad will INSTALL the tensor it is handed instead of adding it to an
    existing one -- .grad is None and no tensor hooks.  Deferring (or accumulating in place) hands autograd a buffer that is
    filled later: a leaf with a gradient already there would get `grad += <unfilled buffer>` at once (zero_grad(set_to_none=
    False), gradient accumulation, a second backward), so only stealable leaves qualify; the others are computed on the spot."""
    counts = {}
    stealable = set()
    fn0 = getattr(root, "grad_fn", None)
    if fn0 is None:
        return set(), set()
    seen, stack = {fn0}, [fn0]
    while stack:
        n = stack.pop()
        for nf, _ in n.next_functions:
            if nf is None:
                continue
            v = getattr(nf, "variable", None)
            if v is not None:                      # AccumulateGrad of a leaf
                counts[v.data_ptr()] = counts.get(v.data_ptr(), 0) + 1
                if v.grad is None and not getattr(v, "_backward_hooks", None):
                    stealable.add(v.data_ptr())
            elif nf not in seen:
                seen.add(nf); stack.append(nf)
    return {k for k, c in counts.items() if c == 1 and k in stealable}, stealable


class deferred_wgrads:
    """with ops.deferred_wgrads(loss): loss.backward() -- `loss`: the tensor whose graph is about to be walked backwards (None: the
    scope defers nothing)"""

    def __init__(self, root=None):
        self.root = root

    def __enter__(self):
        self.prev = _DEFER[0]
        if _DEFER_ON and self.root is not None:
            single, stealable = _single_use_leaves(self.root)
            _DEFER[0] = {"jobs": [], "uses": {}, "made": {}, "single": single, "stealable": stealable}
        else:
            _DEFER[0] = None
        self.root = None
        return self

    def __exit__(self, et, ev, tb):
        cur, _DEFER[0] = _DEFER[0], self.prev
        if cur is not None and et is None and cur["jobs"]:
            _flush_wgrads(cur["jobs"])
        return False


def _try_defer(dy, x, K, key, dw=None, db=None):
    """(dw, db) views for autograd with the product left to the scope's grouped launches, or None (not deferrable: compute now)"""
    cur = _DEFER[0]
    if cur is None or key is None:
        return None
    M, N = dy.shape
    uses = cur["uses"][key] = cur["uses"].get(key, 0) + 1
    if uses > 1 and any(j[7] == key for j in cur["jobs"]):
        # a deferred weight used again in this pass: autograd is about to add the two gradients
        _flush_wgrads(cur["jobs"], everyone_waits=True); cur["jobs"] = []
        return None
    thin = (0 < M <= 128 and N % 4 == 0 and K % 4 == 0
            and dy.dtype == torch.float32 and x.dtype == torch.float32 and dy.stride(1) == 1 and x.stride(1) == 1
            and dy.stride(0) % 4 == 0 and x.stride(0) % 4 == 0 and (dy.data_ptr() | x.data_ptr()) % 16 == 0)
    made = cur["made"].get(key)
    if uses == 2 and made is not None and thin and _ACC_WGRAD and made[0].shape == (N, K) and made[1] is not None:
        # the layer's OTHER application (q(z2 | .) over the exemplar rows: a big GEMM, already launched) made this weight's
        # gradient in this pass: the batch rows' product is ADDED to it by a grouped launch behind the backward pass, and this
        # application hands autograd nothing -- the sum autograd would form with an element-wise launch per tensor (ten per step
        # of the 2-level model, four of them behind the last weight gradient, in front of the optimizer) is formed in place
        cur["jobs"].append((dy, M, N, x, K, made[0], made[1], key, torch.cuda.current_stream(), made[2]))
        return _ACCUMULATED
    if not (uses == 1 and key in cur["single"] and thin):
        return None
    if dw is None:
        dw = torch.empty((N, K), device=dy.device); db = torch.empty(N, device=dy.device)
    # (autograd gets VIEWS of dw / db: AccumulateGrad installs a gradient it is handed without copying only while nobody
    #  else holds that tensor object -- handed the buffers the job keeps, it would clone them, still unfilled; and a view
    #  made here holds its base, so it is the job that keeps the bases)
    cur["jobs"].append((dy, M, N, x, K, dw, db, key, torch.cuda.current_stream(), None))
    return dw.view(N, K), db.view(N)


_ACCUMULATED = (None, None)          # _bwd_weight's answer when the product joins a gradient made earlier in the pass
_ACC_WGRAD = os.environ.get("EVAE_ACC_WGRAD", "1") != "0"


def _note_made(key, dw, db):
    """A weight gradient computed NOW (not deferred) inside a deferred_wgrads scope: remembered under the weight's identity, with
    an event behind its launches, so that a second application of the layer can add its product to it (see _try_defer).  Returns
    the views to hand to autograd (the scope keeps the bases: handed the bases themselves, AccumulateGrad would clone them)."""
    cur = _DEFER[0]
    if (cur is None or key is None or not _ACC_WGRAD or db is None or key in cur["made"] or cur["uses"].get(key, 0) != 1
            or key not in cur["stealable"]):
        return dw, db
    ev = torch.cuda.Event(); ev.record()
    cur["made"][key] = (dw, db, ev)
    return dw.view(dw.shape), db.view(db.shape)


def _bwd_weight(dy, x, rows, K, want_db=True, key=None):
    """dw [N x K] = dy^T x(rows), db [N]; dy may be the combined [M x 2N] buffer [dh | dg].  `key`: identity of the weight
    (its data pointer) for the deferred form above."""
    M, N = dy.shape
    dw = torch.empty((N, K), device=dy.device)
    db = torch.empty(N, device=dy.device) if want_db else None
    if rows is None and want_db and key is not None:
        d = _try_defer(dy, x, K, key, dw, db)
        if d is not None:
            return d
    elif key is not None and _DEFER[0] is not None:
        _DEFER[0]["uses"][key] = _DEFER[0]["uses"].get(key, 0) + 1
    launch.Launcher(dy.device).bwd_weight_call(dy, M, N, dy.stride(0), x, rows, K, x.stride(0), dw, db)()
    return _note_made(key, dw, db)


def _bwd_data(dy1_ptr, w1, dy2_ptr, w2, M, N, ldy, device, out_prev=None, s_prev=None, out=None, dg_ptr=None, ldo=None):
    """Launcher.bwd_data_call on the current stream (operands as tensors or addresses); without `out`, dx [M x K] is allocated
    here.  With out_prev / s_prev, (dh, dg) of the layer below may go into the halves of one [M x 2K] buffer (out, dg_ptr, ldo)."""
    K = w1.shape[1]
    if out is None:
        out = torch.empty((M, K), device=device)
        ldo = K
    launch.Launcher(device).bwd_data_call(dy1_ptr, w1, dy2_ptr, w2, M, N, ldy, K, out_prev, s_prev, out, dg_ptr, ldo)()
    return out


def _dout_rows(dout, N):
    """a gated layer's upstream gradient as the kernels read it: fp32 rows of unit stride (a column block of a wider gradient --
    half of a torch.cat's -- is read where it lies)"""
    if dout.dtype == torch.float32 and dout.dim() == 2 and dout.stride(1) == 1 and dout.stride(0) >= N:
        return dout
    return _f32(dout)


def _gated_bwd(dout, gout, s, wh, wg):
    """A gated layer's backward wrt its input (reference utils/nn.py:62-68 under autograd): (dpre = [dh | dg] for the weight
    gradient, dx = dh Wh + dg Wg) -- Launcher.gated_bwd."""
    M, N = gout.shape
    K = wh.shape[1]
    dpre = torch.empty((M, 2 * N), device=gout.device)
    dx = torch.empty((M, K), device=gout.device)
    launch.Launcher(gout.device).gated_bwd(dout, dout.stride(0), gout, s, M, N, wh, wg, K, dpre, dx)
    return dpre, dx


def _gate_bwd(dout, gout, s):
    """The gate derivative alone: dpre = [dh | dg], one buffer for one weight-gradient GEMM."""
    M, N = gout.shape
    dpre = torch.empty((M, 2 * N), device=gout.device)
    _lib.check(_lib.load().evae_gated_dense_bwd_input_ld(_p(dout), dout.stride(0), _p(gout), _p(s), M, N, _p(dpre), _p(dpre.data_ptr() + 4 * N),
                                                         2 * N, _stream()), "evae_gated_dense_bwd_input_ld")
    return dpre


def _rows_x(x, rows):
    """Validate the (x, rows) pair: x is [R x K] with unit inner stride; rows gathers M rows of it."""
    x = x if x.dtype == torch.float32 else x.float()
    if x.dim() != 2:
        x = x.reshape(x.shape[0], -1)
    if x.stride(1) != 1:
        x = x.contiguous()
    rows = _i64(rows)
    M = x.shape[0] if rows is None else rows.numel()
    return x, rows, M


class ExpandRowsFn(torch.autograd.Function):
    """Encodings of the DISTINCT exemplar rows [U x z] -> encodings of every draw [C x z] (out[j] = src[inv[j]]), for a captured
    step that encodes each distinct image once (the reference draws with replacement, models/BaseModel.py:245, and encodes every
    draw).  Backward: a distinct row's gradient = its multiplicity x the gradient of ONE of its draws (rep) -- duplicates have
    identical encodings, hence identical gradients from the prior; padding rows have multiplicity 0.  evae_gather_rows both ways."""

    @staticmethod
    def forward(ctx, src, inv, rep, mult):
        lib = _lib.load()
        src = _f32(src)
        if not src.is_contiguous():
            src = src.contiguous()
        n, z = inv.numel(), src.shape[1]
        out = torch.empty((n, z), device=src.device)
        _lib.check(lib.evae_gather_rows(_p(src), _p(inv), None, n, z, _p(out), _stream()), "evae_gather_rows")
        ctx.save_for_backward(rep, mult)
        ctx.u = src.shape[0]
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        rep, mult = ctx.saved_tensors
        g = _f32(g)
        if not g.is_contiguous():
            g = g.contiguous()
        out = torch.empty((ctx.u, g.shape[1]), device=g.device)
        _lib.check(lib.evae_gather_rows(_p(g), _p(rep), _p(mult), ctx.u, g.shape[1], _p(out), _stream()), "evae_gather_rows(bwd)")
        return out, None, None, None


def expand_rows(src, inv, rep, mult):
    return ExpandRowsFn.apply(src, inv, rep, mult)


class GatedDenseFn(torch.autograd.Function):
    """utils/nn.py:44-69 (activation None, gate on): h(x) * sigmoid(g(x)), optional row gather."""

    @staticmethod
    def forward(ctx, x, rows, wh, bh, wg, bg):
        _need_cuda(x, rows, wh, wg)
        x, rows, M = _rows_x(x, rows)
        wh, wg = _f32(wh), _f32(wg)
        N, K = wh.shape
        out = torch.empty((M, N), device=x.device)
        need_grad = any(ctx.needs_input_grad)
        s = torch.empty_like(out) if need_grad else None     # the backward needs out and s only (dg = dout*out*(1-s))
        launch.Launcher(x.device).gated_fwd(x, rows, M, K, x.stride(0), wh, bh, wg, bg, N, out, None, s)
        if need_grad:
            ctx.save_for_backward(x, rows, wh, wg, out, s)
        ctx.has_bias = (bh is not None, bg is not None)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, rows, wh, wg, gout, s = ctx.saved_tensors
        N, K = wh.shape
        dout = _dout_rows(dout, N)
        dx = None
        if ctx.needs_input_grad[0]:
            if rows is not None:
                raise _lib.EvaeError("gradient wrt a row-gathered input is not supported")
            dpre, dx = _gated_bwd(dout, gout, s, wh, wg)           # gate derivative + data gradient (one launch when batch-sized)
        else:
            dpre = _gate_bwd(dout, gout, s)
        dw, db = _bwd_weight(dpre, x, rows, K, key=wh.data_ptr())  # [dWh ; dWg], [dbh ; dbg]
        if dw is None:             # added, behind the backward pass, to the gradient the layer's other application made (_try_defer)
            return (dx, None, None, None, None, None)
        return (dx, None, dw[:N], (db[:N] if ctx.has_bias[0] else None), dw[N:],
                (db[N:] if ctx.has_bias[1] else None))


class GatedDenseDataFn(torch.autograd.Function):
    """GatedDenseFn without the parameters' gradients: (x, wh, bh, wg, bg) -> (out, s), backward = dx only."""

    @staticmethod
    def forward(ctx, x, wh, bh, wg, bg):
        _need_cuda(x, wh, wg)
        x, _, M = _rows_x(x, None)
        wh, wg = _f32(wh), _f32(wg)
        N, K = wh.shape
        out = torch.empty((M, N), device=x.device); s = torch.empty_like(out)
        launch.Launcher(x.device).gated_fwd_call(x, None, M, K, x.stride(0), wh, bh, wg, bg, N, out, None, s)()
        ctx.save_for_backward(wh, wg, out, s)
        ctx.mark_non_differentiable(s)
        ctx.set_materialize_grads(False)
        return out, s

    @staticmethod
    def backward(ctx, dout, _ds):
        wh, wg, gout, s = ctx.saved_tensors
        if dout is None or not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        _dpre, dx = _gated_bwd(_dout_rows(dout, gout.shape[1]), gout, s, wh, wg)
        return dx, None, None, None, None


class GatedDenseParamFn(torch.autograd.Function):
    """The parameters' half of a gated layer as a node of its own: forward is an alias of the layer's output (no launch); the
    backward turns the output's gradient into (dWh, dbh, dWg, dbg).  Built under a third stream, autograd runs it there, beside
    the chain of data gradients instead of inside it."""

    @staticmethod
    def forward(ctx, out, s, x, wh, bh, wg, bg):
        ctx.save_for_backward(out, s, x)
        ctx.K = wh.shape[1]
        ctx.has_bias = (bh is not None, bg is not None)
        ctx.set_materialize_grads(False)
        return out.view_as(out)

    @staticmethod
    def backward(ctx, dout):
        if dout is None:
            return (None,) * 7
        gout, s, x = ctx.saved_tensors
        N = gout.shape[1]
        dout = _dout_rows(dout, N)
        st = torch.cuda.current_stream()
        for t in (gout, s, x, dout):       # made on another stream's pool, read here
            t.record_stream(st)
        dpre = _gate_bwd(dout, gout, s)
        dw, db = _bwd_weight(dpre, x, None, ctx.K)
        return (None, None, None, dw[:N], (db[:N] if ctx.has_bias[0] else None), dw[N:], (db[N:] if ctx.has_bias[1] else None))


class _MergeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, token):
        return a.view_as(a)

    @staticmethod
    def backward(ctx, g):
        return g, g


def gated_dense_split(x, wh, bh, wg, bg, leaf):
    """gated_dense with the parameters' gradient node on the stream `leaf` (same values, same gradients)"""
    x2, _, _ = _rows_x(x, None)
    det = lambda t: None if t is None else t.detach()
    out, s = GatedDenseDataFn.apply(x2, det(wh), det(bh), det(wg), det(bg))
    with torch.cuda.stream(leaf):
        token = GatedDenseParamFn.apply(out.detach(), s, x2.detach(), wh, bh, wg, bg)
    return _MergeFn.apply(out, token)


def u8_prepare(wh, wg, out=None):
    """fp32 weight banks [N x K] -> the three-term bf16 tile images of the uint8 first-layer kernels"""
    lib = _lib.load()
    _need_cuda(wh, wg)
    wh, wg = _f32(wh.detach()), _f32(wg.detach())
    N, K = wh.shape
    nb = lib.evae_dense_u8_prepared_bytes(N, K)
    if out is None or out.numel() < nb:
        out = torch.empty(nb, dtype=torch.uint8, device=wh.device)
    _lib.check(lib.evae_dense_u8_prepare(_p(wh), _p(wg), N, K, _p(out), out.numel(), _stream()), "evae_dense_u8_prepare")
    return out


def gated_dense_fwd_u8(x_u8, rows, x_scale, prepared, bh, bg, N, out=None, save_s=None):
    """forward only: out [M x N] for the M gathered rows of the byte store x_u8 [R x K]"""
    lib = _lib.load()
    _need_cuda(x_u8, rows, prepared)
    assert x_u8.dtype == torch.uint8 and x_u8.dim() == 2 and x_u8.stride(1) == 1
    rows = _i64(rows)
    M, K = rows.numel(), x_u8.shape[1]
    if out is None:
        out = torch.empty((M, N), device=x_u8.device)
    _lib.check(lib.evae_gated_dense_fwd_u8(_p(x_u8), _p(rows), M, K, x_u8.stride(0), float(x_scale), _p(prepared), _p(bh),
                                           _p(bg), N, _p(out), _p(save_s), _stream()), "evae_gated_dense_fwd_u8")
    return out


def dense_bwd_weight_u8(dy, x_u8, rows, x_scale, dw=None, db=None, ws_name="wgrad_u8"):
    """dw [N x K] = x_scale * dy^T x_u8[rows], db [N] = column sums of dy (dy [M x N], any row stride)"""
    lib = _lib.load()
    _need_cuda(dy, x_u8, rows)
    assert dy.dtype == torch.float32 and dy.stride(1) == 1 and x_u8.dtype == torch.uint8
    rows = _i64(rows)
    M, N = dy.shape
    K = x_u8.shape[1]
    if dw is None:
        dw = torch.empty((N, K), device=dy.device)
    if db is None:
        db = torch.empty(N, device=dy.device)
    nb = lib.evae_dense_bwd_weight_u8_workspace_bytes(M, N, K)
    ws = _workspace(ws_name, nb, dy.device)
    _lib.check(lib.evae_dense_bwd_weight_u8(_p(dy), M, N, dy.stride(0), _p(x_u8), _p(rows), K, x_u8.stride(0), float(x_scale),
                                            _p(dw), _p(db), _p(ws), ws.numel(), _stream()), "evae_dense_bwd_weight_u8")
    return dw, db


class LinearFn(torch.autograd.Function):
    """act(x W^T + b): torch.nn.Linear / utils/nn.py:29-41 NonLinear."""

    @staticmethod
    def forward(ctx, x, rows, w, b, act, lo, hi):
        _need_cuda(x, rows, w)
        x, rows, M = _rows_x(x, rows)
        w = _f32(w)
        N, K = w.shape
        y = torch.empty((M, N), device=x.device)
        need_grad = any(ctx.needs_input_grad)
        pre = torch.empty_like(y) if (need_grad and act == ACT_HARDTANH) else None
        launch.Launcher(x.device).linear_fwd(x, M, K, x.stride(0), w, b, N, act, float(lo), float(hi), y, pre, rows=rows)
        if need_grad:
            ctx.save_for_backward(x, rows, w, pre if pre is not None else y)
        ctx.act = (act, float(lo), float(hi))
        ctx.has_bias = b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, rows, w, aux = ctx.saved_tensors
        act, lo, hi = ctx.act
        dy = _f32(dy)
        if act != ACT_NONE:
            dpre = torch.empty_like(dy)
            _lib.check(lib.evae_act_bwd(_p(dy), _p(aux), dy.numel(), act, lo, hi, _p(dpre), _stream()),
                       "evae_act_bwd")
        else:
            dpre = dy
        dw, db = _bwd_weight(dpre, x, rows, w.shape[1], key=w.data_ptr())
        dx = None
        if ctx.needs_input_grad[0]:
            if rows is not None:
                raise _lib.EvaeError("gradient wrt a row-gathered input is not supported")
            dx = _bwd_data(dpre.data_ptr(), w, None, None, dpre.shape[0], dpre.shape[1], dpre.stride(0), dpre.device)
        return dx, None, dw, (db if ctx.has_bias else None), None, None, None


class GatedDenseU8Fn(torch.autograd.Function):
    """GatedDense over M gathered rows of the uint8-resident image store (pixel = byte * x_scale): the first encoder layer of
    the exemplar rows on the modular autograd path (hvae_2level, or vae outside the fused node) -- same byte kernels as the
    fused step (csrc/evae_dense_u8.hip: bytes exact in bf16, weights / dy as three bf16 terms, fp32-GEMM accuracy)."""

    @staticmethod
    def forward(ctx, x_u8, rows, x_scale, wh, bh, wg, bg):
        _need_cuda(x_u8, rows, wh, wg)
        rows = _i64(rows)
        wh, wg = _f32(wh), _f32(wg)
        N, K = wh.shape
        M = rows.numel()
        prep = u8_prepare(wh.detach(), wg.detach(), out=_workspace("u8prep_mod%d" % N, _lib.load().evae_dense_u8_prepared_bytes(N, K),
                                                                   x_u8.device))
        need_grad = any(ctx.needs_input_grad)
        out = torch.empty((M, N), device=x_u8.device)
        s = torch.empty_like(out) if need_grad else None
        fl = 2.0 * M * K * 2 * N
        probed("gated_dense_fwd_u8 M=%d K=%d N=%d (uint8 rows, three bf16 terms)" % (M, K, N), fl,
               lambda: gated_dense_fwd_u8(x_u8, rows, x_scale, prep, bh, bg, N, out=out, save_s=s), executed=3 * fl, pipe="bf16-mfma")
        if need_grad:
            ctx.save_for_backward(x_u8, rows, out, s)
        ctx.wkey = wh.data_ptr()
        ctx.x_scale = float(x_scale)
        ctx.has_bias = (bh is not None, bg is not None)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        x_u8, rows, gout, s = ctx.saved_tensors
        dout = _f32(dout)
        M, N = gout.shape
        K = x_u8.shape[1]
        dpre = torch.empty((M, 2 * N), device=gout.device)          # [dh | dg]: one buffer, one weight-grad GEMM
        base = dpre.data_ptr()
        _lib.check(lib.evae_gated_dense_bwd_input(_p(dout), _p(gout), _p(s), M, N, _vp(base), _vp(base + 4 * N),
                                                  2 * N, _stream()), "evae_gated_dense_bwd_input")
        fl = 2.0 * M * 2 * N * K
        dw, db = probed("dense_bwd_weight_u8 M=%d N=%d K=%d (uint8 rows, three bf16 terms; pre-passes + GEMM + finish)" % (M, 2 * N, K),
                        fl, lambda: dense_bwd_weight_u8(dpre, x_u8, rows, ctx.x_scale, ws_name="wgrad_u8_mod"), executed=3 * fl,
                        pipe="bf16-mfma")
        if _DEFER[0] is not None:          # (the batch rows' application of this layer may add its product to this one: _try_defer)
            _DEFER[0]["uses"][ctx.wkey] = _DEFER[0]["uses"].get(ctx.wkey, 0) + 1
            dw, db = _note_made(ctx.wkey, dw, db)
        return (None, None, None, dw[:N], (db[:N] if ctx.has_bias[0] else None), dw[N:], (db[N:] if ctx.has_bias[1] else None))


def gated_dense(x, wh, bh, wg, bg, rows=None, x_scale=None):
    """x fp32 [R x K] (optionally row-gathered), or the uint8 image store with x_scale (pixel = byte * x_scale; rows required)"""
    if x.dtype == torch.uint8:
        if rows is None or x_scale is None:
            raise _lib.EvaeError("gated_dense on the uint8 store needs the gather list and x_scale")
        return GatedDenseU8Fn.apply(x, rows, float(x_scale), wh, bh, wg, bg)
    return GatedDenseFn.apply(x, rows, wh, bh, wg, bg)


def linear(x, w, b, act=ACT_NONE, lo=0.0, hi=0.0, rows=None):
    return LinearFn.apply(x, rows, w, b, act, lo, hi)


# ------------------------------------------------------------------------------------------------
# convolutions (implicit GEMM)
# ------------------------------------------------------------------------------------------------
def _conv_desc(x, w, stride, pad):
    N, Cc, H, W = x.shape
    Co, Ci, KH, KW = w.shape
    assert Ci == Cc, "groups != 1 is not supported"
    d = _lib.ConvDesc(N, Cc, H, W, Co, KH, KW, int(stride), int(pad))
    OH = (H + 2 * pad - KH) // stride + 1
    OW = (W + 2 * pad - KW) // stride + 1
    return d, OH, OW


def _int1(v):
    if isinstance(v, (tuple, list)):
        assert all(e == v[0] for e in v), "only square stride / padding"
        return int(v[0])
    return int(v)


CL = torch.channels_last


def _cl(t):
    """channels-last storage ([N][H][W][C]) of a logical NCHW tensor"""
    return t if t.is_contiguous(memory_format=CL) else t.contiguous(memory_format=CL)


class Conv2dFn(torch.autograd.Function):
    """act(conv2d(x, wh) + bh) [* sigmoid(conv2d(x, wg) + bg)]  -- utils/nn.py:72-114, nn.Conv2d.

    Two kernel families behind one interface (include/evae_hip.h): channels-last GEMM instances when the geometry
    qualifies (input channels a multiple of 32: every layer but the first of the reference's conv stacks), the NCHW
    implicit-GEMM kernels otherwise.  Tensors keep their logical NCHW shape; outputs of the channels-last family
    are torch.channels_last tensors, so a stack of qualifying layers never changes layout."""

    @staticmethod
    def forward(ctx, x, wh, bh, wg, bg, stride, pad, act, lo, hi):
        lib = _lib.load()
        _need_cuda(x, wh, wg)
        x = x.float(); wh = _f32(wh); wg = None if wg is None else _f32(wg)
        d, OH, OW = _conv_desc(x, wh, stride, pad)
        gated = wg is not None
        need_grad = any(ctx.needs_input_grad)
        cl = bool(lib.evae_conv2d_cl_supported(C.byref(d), 0, int(gated)))
        if cl:
            x = _cl(x)
            fmt = dict(device=x.device, memory_format=CL)
        else:
            x = x.contiguous()
            fmt = dict(device=x.device)
        out = torch.empty((d.N, d.Co, OH, OW), **fmt)
        s = torch.empty((d.N, d.Co, OH, OW), **fmt) if (gated and need_grad) else None   # out and s suffice for the backward
        pre = torch.empty((d.N, d.Co, OH, OW), **fmt) if (not gated and need_grad and act == ACT_HARDTANH) else None
        if cl:
            if os.environ.get("EVAE_CONV_TRACE"):
                print("conv_cl_fwd N=%d C=%d H=%d W=%d Co=%d k=%d s=%d p=%d gated=%d grad=%d" % (d.N, d.C, d.H, d.W, d.Co, d.KH, d.stride, d.pad, gated, need_grad), flush=True)
            nb = lib.evae_conv2d_cl_workspace_bytes(C.byref(d), 0, int(gated))
            ws = _workspace("conv", nb, x.device)
            _lib.check(lib.evae_conv2d_cl_fwd(_p(x), C.byref(d), _p(wh), _p(bh), _p(wg), _p(bg), act, float(lo), float(hi),
                                              _p(out), _p(None if gated else pre), _p(s), _p(ws), ws.numel(), _stream()),
                       "evae_conv2d_cl_fwd")
        else:
            nb = lib.evae_conv2d_workspace_bytes(C.byref(d), 0, int(gated))
            ws = _workspace("conv", nb, x.device)
            _lib.check(lib.evae_conv2d_fwd(_p(x), C.byref(d), _p(wh), _p(bh), _p(wg), _p(bg), act, float(lo), float(hi),
                                           _p(out), _p(None if gated else pre), _p(s), _p(ws), ws.numel(), _stream()),
                       "evae_conv2d_fwd")
        if need_grad:
            ctx.save_for_backward(x, wh, wg, s, pre if pre is not None else out)
        ctx.cfg = (d, gated, act, float(lo), float(hi), bh is not None, bg is not None, cl)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        x, wh, wg, s, aux = ctx.saved_tensors
        d, gated, act, lo, hi, has_bh, has_bg, cl = ctx.cfg
        dev = dout.device
        shp = wh.shape
        ctot = d.Co * (2 if gated else 1)
        K = d.C * d.KH * d.KW
        OH, OW = dout.shape[2], dout.shape[3]
        # channels-last family for the gradients when this layer ran it forward (saved tensors are channels-last)
        # or when the weight gradient qualifies anyway (then x is re-laid out once)
        cl_w = bool(lib.evae_conv2d_cl_supported(C.byref(d), 2, int(gated))) and cl
        cl_d = bool(lib.evae_conv2d_cl_supported(C.byref(d), 1, int(gated))) and cl
        if gated and act != ACT_NONE:
            raise _lib.EvaeError("gated conv with an activation on h: compose it from two plain convs")
        need_dx = ctx.needs_input_grad[0]
        dout = _cl(dout.float()) if cl else _f32(dout)
        n = dout.numel()

        def act_bwd(dst):
            _lib.check(lib.evae_act_bwd(_p(dout), _p(aux), n, act, lo, hi, _p(dst), _stream()), "evae_act_bwd")

        # 1. the gradient at the convolution's output(s), once: dy (channels-last family) or dh, dg (NCHW family)
        dh = dg = dy = None
        if cl:
            # [dh | dg | zero padding] per pixel in ONE buffer: logical [N, ldy, OH, OW], channels-last
            ldy = lib.evae_conv2d_cl_dy_stride(ctot)
            dy = torch.empty((d.N, ldy, OH, OW), device=dev, memory_format=CL)
            if ldy != ctot:
                dy.zero_()
            if gated:
                # rows = pixels, columns = Co channels: dh to columns [0, Co), dg to [Co, 2 Co)
                _lib.check(lib.evae_gated_dense_bwd_input(_p(dout), _p(aux), _p(s), n // d.Co, d.Co, _p(dy), _p(dy.data_ptr() + 4 * d.Co),
                                                          ldy, _stream()), "evae_gated_dense_bwd_input")
            elif ldy != ctot:
                src = dout
                if act != ACT_NONE:
                    src = torch.empty_like(dout)
                    act_bwd(src)
                dy[:, :ctot].copy_(src)
            elif act != ACT_NONE:
                act_bwd(dy)
            else:
                dy = dout
            if (not cl_w) or (need_dx and not cl_d):
                # what the channels-last kernels do not take goes through the NCHW ones (e.g. the data gradient of a thin first layer)
                dh = dy[:, :d.Co].contiguous()
                dg = dy[:, d.Co:ctot].contiguous() if gated else None
                xn = x.contiguous()
        else:
            xn = x
            if gated:
                dh = torch.empty_like(dout); dg = torch.empty_like(dout)
                _lib.check(lib.evae_gated_dense_bwd_input(_p(dout), _p(aux), _p(s), 1, n, _p(dh), _p(dg), n, _stream()),
                           "evae_gated_dense_bwd_input")
            elif act != ACT_NONE:
                dh = torch.empty_like(dout)
                act_bwd(dh)
            else:
                dh = dout
        # 2. the weight gradient, on the family cl_w picks
        dw = torch.empty((ctot, K), device=dev); db = torch.empty(ctot, device=dev)
        if cl_w:
            ws = _workspace("conv", lib.evae_conv2d_cl_workspace_bytes(C.byref(d), 2, int(gated)), dev)
            _lib.check(lib.evae_conv2d_cl_bwd_weight(_p(dy), _p(x), C.byref(d), int(gated), _p(dw), _p(db), _p(ws), ws.numel(), _stream()),
                       "evae_conv2d_cl_bwd_weight")
        else:
            ws = _workspace("conv", lib.evae_conv2d_workspace_bytes(C.byref(d), 2, int(gated)), dev)
            _lib.check(lib.evae_conv2d_bwd_weight(_p(dh), _p(dg), _p(xn), C.byref(d), _p(dw), _p(db), _p(ws), ws.numel(), _stream()),
                       "evae_conv2d_bwd_weight")
        # 3. the data gradient, on the family cl_d picks
        dx = None
        if need_dx and cl_d:
            dx = torch.empty(x.shape, device=dev, memory_format=CL)
            ws = _workspace("conv", lib.evae_conv2d_cl_workspace_bytes(C.byref(d), 1, int(gated)), dev)
            _lib.check(lib.evae_conv2d_cl_bwd_data(_p(dy), _p(wh), _p(wg), C.byref(d), _p(dx), _p(ws), ws.numel(), _stream()),
                       "evae_conv2d_cl_bwd_data")
        elif need_dx:
            dx = torch.empty(xn.shape, device=dev)
            ws = _workspace("conv", lib.evae_conv2d_workspace_bytes(C.byref(d), 1, int(gated)), dev)
            _lib.check(lib.evae_conv2d_bwd_data(_p(dh), _p(wh), _p(dg), _p(wg), C.byref(d), _p(dx), _p(ws), ws.numel(), _stream()),
                       "evae_conv2d_bwd_data")
        gwh = dw[:d.Co].reshape(shp)
        gwg = dw[d.Co:].reshape(shp) if gated else None
        return (dx, gwh, db[:d.Co] if has_bh else None, gwg, (db[d.Co:] if (gated and has_bg) else None),
                None, None, None, None, None)


class ResBlockFn(torch.autograd.Function):
    """x + conv2d(ELU(x), w) + b -- the residual block of models/fully_conv.py:13-23 on the channels-last kernels: ELU is one
    elementwise launch (its output is the convolution's operand AND what the backward needs), the residual add rides in the
    convolution's epilogue, and the block's data gradient dy + ELU'(x) * conv_transpose(dy, w) is ONE launch."""

    @staticmethod
    def forward(ctx, x, w, b):
        lib = _lib.load()
        _need_cuda(x, w)
        x = _cl(x.float()); w = _f32(w)
        d, OH, OW = _conv_desc(x, w, 1, (w.shape[2] - 1) // 2)
        a = torch.empty_like(x, memory_format=CL)
        _lib.check(lib.evae_elu_fwd(_p(x), x.numel(), _p(a), _stream()), "evae_elu_fwd")
        out = torch.empty_like(x, memory_format=CL)
        ws = _workspace("conv", lib.evae_conv2d_cl_workspace_bytes(C.byref(d), 0, 0), x.device)
        _lib.check(lib.evae_conv2d_cl_fwd_res(_p(a), C.byref(d), _p(w), _p(b), _p(x), _p(out), _p(ws), ws.numel(), _stream()),
                   "evae_conv2d_cl_fwd_res")
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(a, w)
        ctx.cfg = (d, b is not None)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        a, w = ctx.saved_tensors
        d, has_b = ctx.cfg
        dev = dout.device
        dy = _cl(dout.float())
        K = d.C * d.KH * d.KW
        dw = db = None
        if ctx.needs_input_grad[1] or (has_b and ctx.needs_input_grad[2]):
            dw = torch.empty((d.Co, K), device=dev); db = torch.empty(d.Co, device=dev)
            ws = _workspace("conv", lib.evae_conv2d_cl_workspace_bytes(C.byref(d), 2, 0), dev)
            _lib.check(lib.evae_conv2d_cl_bwd_weight(_p(dy), _p(a), C.byref(d), 0, _p(dw), _p(db), _p(ws), ws.numel(), _stream()),
                       "evae_conv2d_cl_bwd_weight")
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(a, memory_format=CL)
            ws = _workspace("conv", lib.evae_conv2d_cl_workspace_bytes(C.byref(d), 1, 0), dev)
            _lib.check(lib.evae_conv2d_cl_bwd_data_res(_p(dy), _p(w), C.byref(d), _p(dy), _p(a), _p(dx), _p(ws), ws.numel(),
                                                       _stream()), "evae_conv2d_cl_bwd_data_res")
        return dx, (None if dw is None else dw.reshape(w.shape)), (db if has_b else None)


def res_block_supported(x, w, stride, padding):
    """ELU -> 3x3 'same' convolution -> + x on the fused path?  The geometry rules live in ONE place, the library's
    evae_conv2d_cl_res_supported (shape kept, stride 1, channel counts / workspace / images-per-pass limits of the
    channels-last kernels); anything it refuses runs as x + f(x) on the plain layers."""
    if not (x.is_cuda and x.dim() == 4 and w.dim() == 4 and w.shape[1] == x.shape[1]):
        return False
    d, _, _ = _conv_desc(x, w, _int1(stride), _int1(padding))
    return bool(_lib.load().evae_conv2d_cl_res_supported(C.byref(d)))


def res_block(x, w, b):
    return ResBlockFn.apply(x, w, b)


def conv2d(x, w, b, stride=1, padding=0, act=ACT_NONE, lo=0.0, hi=0.0):
    return Conv2dFn.apply(x, w, b, None, None, _int1(stride), _int1(padding), act, lo, hi)


def gated_conv2d(x, wh, bh, wg, bg, stride=1, padding=0):
    return Conv2dFn.apply(x, wh, bh, wg, bg, _int1(stride), _int1(padding), ACT_NONE, 0.0, 0.0)


# ------------------------------------------------------------------------------------------------
# a stack of gated convolutions on pre-split pixel images (csrc/evae_conv_win.h)
# ------------------------------------------------------------------------------------------------
CONV_STACK_MIN_IMAGES = int(os.environ.get("EVAE_CONV_STACK_MIN", "1024"))     # below: the layer-by-layer path (batch rows)
CONV_STACK_ON = os.environ.get("EVAE_CONV_STACK", "1") != "0"


def _pad32(c):
    return (int(c) + 31) // 32 * 32


def conv_stack_depth(x_shape, layers):
    """How many leading layers of a stack of gated convolutions `layers` = [(wh, stride, pad), ...] the image pipeline takes:
    layer 0 on the channels-last kernels (an input that is data: no gradient), layers 1 .. b - 1 on the window kernels with their
    activations as pixel images.  0 = not worth it / not supported."""
    lib = _lib.load()
    N, Cc, H, W = x_shape
    if len(layers) < 2:
        return 0
    # ok_inner[i]: layer i can be an INNER layer of the run (its output feeds the next layer as an image: Co % 16 == 0, real width);
    # ok_last[i]: it can be the LAST TAKEN layer -- GatedConvStackFn zero-pads that one's filters to a multiple of 32 output
    # channels whenever Co % 32 != 0 (a 6-channel layer as 32: five times the matrix work of a layer that has 1 % of the stack's), so
    # the padded geometry is what has to be supported.  Every layer >= 1 needs a weight-gradient path: the window kernel, or
    # the channels-last one (the truncated-depth case checked the unpadded width, and no weight-gradient fallback)
    ok_inner, ok_last = [], []
    for i, (wh, st, pd) in enumerate(layers):
        Co, Ci, KH, KW = wh.shape
        if Ci != Cc:
            break

        def supported(co):
            d = _lib.ConvDesc(N, Cc, H, W, co, KH, KW, int(st), int(pd))
            if i == 0:
                return bool(lib.evae_conv2d_cl_supported(C.byref(d), 0, 1) and lib.evae_conv2d_cl_supported(C.byref(d), 2, 1))
            return bool(lib.evae_cw_supported(C.byref(d), 0) and lib.evae_cw_supported(C.byref(d), 1)
                        and (lib.evae_cw_supported(C.byref(d), 2) or lib.evae_conv2d_cl_supported(C.byref(d), 2, 1)))
        ok_inner.append(Co % 16 == 0 and supported(Co))
        ok_last.append(i >= 1 and (supported(Co) if Co % 32 == 0 else supported(_pad32(Co))))
        if not ok_inner[-1]:
            break
        Cc, H, W = Co, (H + 2 * pd - KH) // st + 1, (W + 2 * pd - KW) // st + 1
    # the longest prefix whose inner layers are all fine and whose last layer can close the run
    for b in range(len(ok_last), 1, -1):
        if ok_last[b - 1] and all(ok_inner[:b - 1]):
            return b
    return 0


def _pad_last_layer(layer, padc, biases):
    """(wh, bh, wg, bg) of the last layer the image pipeline takes, with padc zero output channels behind the real ones: the layer
    runs at a multiple of 32 output channels (conv_stack_depth).  biases: pad them too (the forward pass; the backward pass reads
    the filters only)."""
    wh, bh, wg, bg = layer
    zw = wh.new_zeros((padc,) + tuple(wh.shape[1:]))

    def bias(t):
        return t if (t is None or not biases) else torch.cat((t.float(), t.new_zeros(padc)))
    return [torch.cat((_f32(wh), zw)), bias(bh), torch.cat((_f32(wg), zw)), bias(bg)]


class GatedConvStackFn(torch.autograd.Function):
    """Layers 0 .. b - 1 of a stack of gated convolutions act(h(x)) * sigmoid(g(x)) (reference utils/nn.py:72-97, as
    models/convHVAE_2level.py:21-46 chains them) with every activation between two layers as a pre-split pixel image
    (include/evae_hip.h, evae_cw_*): a layer's epilogue writes the image the next layer's window loads read; in the backward pass a
    layer's data gradient applies the gate derivative of the layer below in its epilogue and writes the merged [dh | dg] image
    that layer's own gradients read -- no elementwise pass, no patch matrix, no fp32 activation except where a kernel outside
    the family still wants one.  Layer 0 reads the data itself (evae_cw_first_*: exact fp32 from a window of the input in LDS, no
    patch matrix).  x is data (no gradient).  args: x, n, cfg = ((stride, pad), ...), then wh, bh, wg, bg per layer."""

    @staticmethod
    def forward(ctx, x, cfg, *params):
        lib = _lib.load()
        b = len(cfg)
        L = [list(params[4 * i:4 * i + 4]) for i in range(b)]
        _need_cuda(x, *[t for t in params if t is not None])
        co_real = [int(L[i][0].shape[0]) for i in range(b)]
        if b >= 2 and co_real[b - 1] % 32:
            L[b - 1] = _pad_last_layer(L[b - 1], _pad32(co_real[b - 1]) - co_real[b - 1], biases=True)
        x = _cl(x.float())
        dev = x.device
        need_grad = any(ctx.needs_input_grad[2:])
        N = x.shape[0]
        ds, shp = [], []
        Cc, H, W = x.shape[1], x.shape[2], x.shape[3]
        for i in range(b):
            Co, Ci, KH, KW = L[i][0].shape
            st, pd = cfg[i]
            ds.append(_lib.ConvDesc(N, Cc, H, W, Co, KH, KW, int(st), int(pd)))
            Cc, H, W = Co, (H + 2 * pd - KH) // st + 1, (W + 2 * pd - KW) // st + 1
            shp.append((Co, H, W))
        wg_cw = [i >= 1 and bool(lib.evae_cw_supported(C.byref(ds[i]), 2)) for i in range(b)]     # weight gradient on the window kernels
        planar = [i + 1 < b and cfg[i + 1][0] == 2 for i in range(b)]                                # row order of layer i's output image
        fmt = dict(device=dev, memory_format=CL)

        def image(rows, ch):
            return torch.empty(int(lib.evae_cw_image_bytes(rows, ch)), dtype=torch.uint8, device=dev)

        # layer 0 on the data: the first-layer kernel (fp32 window in LDS -> image + gate), or the channels-last kernels + a packing pass
        d0 = ds[0]
        Co0, H0, W0 = shp[0]
        wh0, bh0, wg0, bg0 = L[0]
        first_fwd = bool(lib.evae_cw_supported(C.byref(d0), 3))
        first_wg = bool(lib.evae_cw_supported(C.byref(d0), 4))
        need_out0 = need_grad and not wg_cw[1]
        imgs = [image(N * H0 * W0, Co0)]
        s0 = torch.empty((N, Co0, H0, W0), **fmt) if (need_grad or not first_fwd) else None
        out0 = torch.empty((N, Co0, H0, W0), **fmt) if (need_out0 or not first_fwd) else None
        if first_fwd:
            _lib.check(lib.evae_cw_first_fwd(_p(x), C.byref(d0), _p(_f32(wh0)), _p(bh0), _p(_f32(wg0)), _p(bg0), _p(imgs[0]), int(planar[0]),
                                             _p(s0), _p(out0), _stream()), "evae_cw_first_fwd")
        else:
            ws = _workspace("conv", lib.evae_conv2d_cl_workspace_bytes(C.byref(d0), 0, 1), dev)
            _lib.check(lib.evae_conv2d_cl_fwd(_p(x), C.byref(d0), _p(_f32(wh0)), _p(bh0), _p(_f32(wg0)), _p(bg0), ACT_NONE, 0.0, 0.0,
                                              _p(out0), None, _p(s0), _p(ws), ws.numel(), _stream()), "evae_conv2d_cl_fwd")
            _lib.check(lib.evae_cw_pack_image(_p(out0), N, H0, W0, Co0, int(planar[0]), _p(imgs[0]), _stream()), "evae_cw_pack_image")
        outf = [out0 if need_out0 else None]         # fp32 copies: the input of a layer whose weight gradient runs outside the family
        gates = [s0 if need_grad else None]
        for i in range(1, b):
            Co, Hh, Ww = shp[i]
            wh, bh, wg, bg = L[i]
            oimg = image(N * Hh * Ww, Co)
            last = i == b - 1
            s = torch.empty((N, Co, Hh, Ww), **fmt) if need_grad else None
            of = torch.empty((N, Co, Hh, Ww), **fmt) if (last or (need_grad and not wg_cw[i + 1])) else None
            ws = _workspace("cw", lib.evae_cw_workspace_bytes(C.byref(ds[i]), 0), dev)
            _lib.check(lib.evae_cw_fwd_gated(_p(imgs[i - 1]), C.byref(ds[i]), _p(_f32(wh)), _p(bh), _p(_f32(wg)), _p(bg), _p(oimg), int(planar[i]),
                                             _p(s), _p(of), _p(ws), ws.numel(), _stream()), "evae_cw_fwd_gated")
            imgs.append(oimg); gates.append(s); outf.append(of)
            if not need_grad:
                imgs[i - 1] = None
        out = outf[b - 1]
        if need_grad:
            ctx.save_for_backward(x, *[t for t in params if t is not None])
            ctx.keep = (imgs, gates, outf[:b - 1], ds, shp, planar, wg_cw, [[t is not None for t in params[4 * i:4 * i + 4]] for i in range(b)], first_wg,
                        co_real)
        return out if co_real[b - 1] == shp[b - 1][0] else out[:, :co_real[b - 1]]

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        imgs, gates, outf, ds, shp, planar, wg_cw, has, first_wg, co_real = ctx.keep
        saved = list(ctx.saved_tensors)
        x = saved.pop(0)
        b = len(ds)
        L = []
        for i in range(b):
            L.append([saved.pop(0) if h else None for h in has[i]])
        dev = dout.device
        N = x.shape[0]
        if co_real[b - 1] != shp[b - 1][0]:       # the padded last layer: its missing channels have no upstream gradient
            full = torch.empty((N, shp[b - 1][0], dout.shape[2], dout.shape[3]), device=dev, memory_format=CL).zero_()
            full[:, :co_real[b - 1]] = dout
            dout = full
            L[b - 1] = _pad_last_layer(L[b - 1], shp[b - 1][0] - co_real[b - 1], biases=False)    # (the data gradient reads the filters only)
        dout = _cl(dout.float())
        grads = [None] * (4 * b)

        def image(rows, ch):
            return torch.empty(int(lib.evae_cw_image_bytes(rows, ch)), dtype=torch.uint8, device=dev)

        def put(i, dw, db):
            Co, Cr = shp[i][0], co_real[i]
            wshape = (Cr,) + tuple(L[i][0].shape[1:])
            grads[4 * i] = dw[:Cr].reshape(wshape)
            grads[4 * i + 2] = dw[Co:Co + Cr].reshape(wshape)
            if has[i][1]:
                grads[4 * i + 1] = db[:Cr]
            if has[i][3]:
                grads[4 * i + 3] = db[Co:Co + Cr]

        # exit of the stack: gate derivative of the last layer from the fp32 upstream gradient
        Co, Hh, Ww = shp[b - 1]
        dyimg = image(N * Hh * Ww, 2 * Co)
        dyf = torch.empty((N, 2 * Co, Hh, Ww), device=dev, memory_format=CL) if not wg_cw[b - 1] else None
        _lib.check(lib.evae_cw_gate_bwd_image(_p(dout), _p(imgs[b - 1]), 0, _p(gates[b - 1]), N, Hh, Ww, Co, _p(dyimg), _p(dyf), _stream()),
                   "evae_cw_gate_bwd_image")
        imgs[b - 1] = None; gates[b - 1] = None
        for i in range(b - 1, 0, -1):
            d = ds[i]
            Co = shp[i][0]
            K = d.C * d.KH * d.KW
            dw = torch.empty((2 * Co, K), device=dev); db = torch.empty(2 * Co, device=dev)
            if wg_cw[i]:
                ws = _workspace("cw", lib.evae_cw_workspace_bytes(C.byref(d), 2), dev)
                _lib.check(lib.evae_cw_bwd_weight(_p(dyimg), int(planar[i]), _p(imgs[i - 1]), C.byref(d), _p(dw), _p(db), _p(ws), ws.numel(),
                                                  _stream()), "evae_cw_bwd_weight")
            else:
                ws = _workspace("conv", lib.evae_conv2d_cl_workspace_bytes(C.byref(d), 2, 1), dev)
                _lib.check(lib.evae_conv2d_cl_bwd_weight(_p(dyf), _p(outf[i - 1]), C.byref(d), 1, _p(dw), _p(db), _p(ws), ws.numel(), _stream()),
                           "evae_conv2d_cl_bwd_weight")
            put(i, dw, db)
            # data gradient + gate derivative of layer i - 1
            Cp, Hp, Wp = shp[i - 1]
            want_img = i - 1 >= 1
            want_f = (i - 1 == 0) or not wg_cw[i - 1]
            nimg = image(N * Hp * Wp, 2 * Cp) if want_img else None
            nf = torch.empty((N, 2 * Cp, Hp, Wp), device=dev, memory_format=CL) if want_f else None
            ws = _workspace("cw", lib.evae_cw_workspace_bytes(C.byref(d), 1), dev)
            _lib.check(lib.evae_cw_bwd_data_gate(_p(dyimg), int(planar[i]), C.byref(d), _p(_f32(L[i][0])), _p(_f32(L[i][2])), _p(imgs[i - 1]),
                                                 _p(gates[i - 1]), _p(nimg), _p(nf), _p(ws), ws.numel(), _stream()), "evae_cw_bwd_data_gate")
            imgs[i - 1] = None; gates[i - 1] = None
            dyimg, dyf = nimg, nf
        # layer 0: weight gradient on the channels-last kernels from the merged fp32 gradient
        d0 = ds[0]
        Co0 = shp[0][0]
        K0 = d0.C * d0.KH * d0.KW
        dw = torch.empty((2 * Co0, K0), device=dev); db = torch.empty(2 * Co0, device=dev)
        if first_wg:
            ws = _workspace("cw", lib.evae_cw_first_workspace_bytes(), dev)
            _lib.check(lib.evae_cw_first_bwd_weight(_p(dyf), _p(x), C.byref(d0), _p(dw), _p(db), _p(ws), ws.numel(), _stream()),
                       "evae_cw_first_bwd_weight")
        else:
            ws = _workspace("conv", lib.evae_conv2d_cl_workspace_bytes(C.byref(d0), 2, 1), dev)
            _lib.check(lib.evae_conv2d_cl_bwd_weight(_p(dyf), _p(x), C.byref(d0), 1, _p(dw), _p(db), _p(ws), ws.numel(), _stream()),
                       "evae_conv2d_cl_bwd_weight")
        put(0, dw, db)
        ctx.keep = None
        return (None, None) + tuple(grads)


def _cup(c, m):
    return (c + m - 1) // m * m


def plain_conv_supported(x, w, stride, padding, need_dx=None, upsample=False):
    """A 3 x 3 'same' convolution (stride 1 or 2, any channel counts <= 128) on the window kernels?  (enough pixels to fill the machine;
    upsample: x is the half-resolution tensor in front of nn.Upsample(scale_factor=2))"""
    if not (CONV_STACK_ON and x.is_cuda and x.dim() == 4 and w.dim() == 4):
        return False
    N, Cc, H, W = x.shape
    if upsample:
        H, W = 2 * H, 2 * W
    Co, Ci, KH, KW = w.shape
    st = stride[0] if isinstance(stride, (tuple, list)) else stride
    pd = padding[0] if isinstance(padding, (tuple, list)) else padding
    if Ci != Cc or KH != 3 or KW != 3 or pd != 1 or st not in (1, 2) or N * H * W < RES_STACK_MIN_PIXELS // 4:
        return False
    lib = _lib.load()
    d = _lib.ConvDesc(N, Cc, H, W, Co, 3, 3, st, 1)
    need_dx = x.requires_grad if need_dx is None else need_dx
    grads = torch.is_grad_enabled() and (x.requires_grad or w.requires_grad)
    ok = bool(lib.evae_cw_plain_supported(C.byref(d), 0))
    if ok and grads:
        ok = bool(lib.evae_cw_plain_supported(C.byref(d), 2)) and (not need_dx or bool(lib.evae_cw_plain_supported(C.byref(d), 1)))
    return ok


class PlainConvFn(torch.autograd.Function):
    """y = conv2d(x, w, b) (3 x 3, 'same', stride 1 or 2), optionally ELU(y), on the window kernels over pixel images: the weight-normed
    convolutions outside fully_conv's residual runs and its 3-channel output head (reference models/fully_conv.py:41-58).  The input is
    split into its image once (parity-planar rows for stride 2) and kept for the weight gradient; the gradient arrives in whatever
    layout autograd hands it (NCHW from the likelihood) and is packed -- times ELU'(y) when the ELU was fused -- into the image both
    gradients read."""

    @staticmethod
    def forward(ctx, x, w, b, stride, elu, upsample=False):
        lib = _lib.load()
        w = _f32(w)
        _need_cuda(x, w)
        x = x.float()
        nchw = 1 if (x.is_contiguous() and not x.is_contiguous(memory_format=CL)) else 0       # (the data arrives as NCHW planes)
        if not nchw:
            x = _cl(x)
        dev = x.device
        N, Cc, H, W = x.shape
        if upsample:                                   # nn.Upsample(scale_factor=2) in front of the convolution: done by the pack
            H, W = 2 * H, 2 * W
        Co = w.shape[0]
        st = int(stride)
        OH, OW = H // st, W // st
        d = _lib.ConvDesc(N, Cc, H, W, Co, 3, 3, st, 1)
        Cp, Cop, Co8 = _cup(Cc, 16), _cup(Co, 16), _cup(Co, 8)
        ximg = torch.empty(int(lib.evae_cw_image_bytes(N * H * W, Cp)), dtype=torch.uint8, device=dev)
        _lib.check(lib.evae_cw_pack_image_ex(_p(x), Cc, Cc, nchw, None, 0, N, H, W, Cp, (1 if st == 2 else 0) | (4 if upsample else 0), _p(ximg),
                                             _stream()), "evae_cw_pack_image_ex")
        out = torch.empty((N, OH, OW, Co8), device=dev)
        ws = _workspace("cw", lib.evae_cw_plain_workspace_bytes(C.byref(d), 0), dev)
        _lib.check(lib.evae_cw_plain_fwd(_p(ximg), C.byref(d), _p(w), _p(b), 1 if elu else 0, _p(out), Co8, None, 0, _p(ws), ws.numel(), _stream()),
                   "evae_cw_plain_fwd")
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(w)
            ctx.keep = (ximg, d, out if elu else None, b is not None, (Cp, Cop, Co8), bool(upsample))
        return out.permute(0, 3, 1, 2)[:, :Co]

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        (w,) = ctx.saved_tensors
        ximg, d, act, has_b, (Cp, Cop, Co8), upsample = ctx.keep
        ctx.keep = None
        dev = dy.device
        N, Cc, H, W, Co, st = d.N, d.C, d.H, d.W, d.Co, d.stride
        OH, OW = H // st, W // st
        dy = dy.float()
        if dy.is_contiguous():
            nchw, ldy = 1, 0
        elif dy.permute(0, 2, 3, 1).is_contiguous():
            nchw, ldy = 0, Co
        else:
            dy, nchw, ldy = dy.contiguous(), 1, 0
        dyimg = torch.empty(int(lib.evae_cw_image_bytes(N * OH * OW, Cop)), dtype=torch.uint8, device=dev)
        _lib.check(lib.evae_cw_pack_image_ex(_p(dy), ldy, Co, nchw, _p(act), Co8, N, OH, OW, Cop, 0, _p(dyimg), _stream()), "evae_cw_pack_image_ex(dy)")
        gw = gb = gx = None
        if ctx.needs_input_grad[1] or (has_b and ctx.needs_input_grad[2]):
            r = _lib.ConvDesc(N, Cp, H, W, Cop, 3, 3, st, 1)
            dwp = torch.empty((Cop, Cp, 3, 3), device=dev); dbp = torch.empty(Cop, device=dev)
            ws = _workspace("cw", lib.evae_cw_plain_workspace_bytes(C.byref(d), 2), dev)
            _lib.check(lib.evae_cw_bwd_weight_plain(_p(dyimg), _p(ximg), C.byref(r), _p(dwp), _p(dbp), _p(ws), ws.numel(), _stream()),
                       "evae_cw_bwd_weight_plain")
            gw = dwp[:Co, :Cc].contiguous() if (Cop != Co or Cp != Cc) else dwp
            gb = dbp[:Co] if has_b else None
        if ctx.needs_input_grad[0]:
            C8 = _cup(Cc, 8)
            dx = torch.empty((N, H, W, C8), device=dev)
            ws = _workspace("cw", lib.evae_cw_plain_workspace_bytes(C.byref(d), 1), dev)
            _lib.check(lib.evae_cw_plain_bwd_data(_p(dyimg), 0, C.byref(d), _p(w), _p(dx), C8, None, _p(ws), ws.numel(), _stream()),
                       "evae_cw_plain_bwd_data")
            if upsample:
                lo = torch.empty((N, H // 2, W // 2, C8), device=dev)
                _lib.check(lib.evae_cw_upsample2_bwd(_p(dx), C8, N, H, W, C8, _p(lo), _stream()), "evae_cw_upsample2_bwd")
                dx = lo
            gx = dx.permute(0, 3, 1, 2)[:, :Cc]
        return gx, gw, gb, None, None, None


def plain_conv(x, w, b, stride=1, elu=False, upsample=False):
    return PlainConvFn.apply(x, w, b, int(stride[0] if isinstance(stride, (tuple, list)) else stride), bool(elu), bool(upsample))


def _ptr_array(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


class WeightNormSetFn(torch.autograd.Function):
    """w_i = v_i * (g_i / ||v_i||) (norm over all but dim 0: torch.nn.utils.weight_norm as reference models/fully_conv.py:18,41-58
    wraps its convolutions) for a SET of filters in ONE launch, and one more for all their (dv_i, dg_i).  args: v_0, g_0, v_1, g_1, ..."""

    @staticmethod
    def forward(ctx, *vg):
        lib = _lib.load()
        vs = [_f32(t) for t in vg[0::2]]
        gs = [_f32(t) for t in vg[1::2]]
        _need_cuda(*vs, *gs)
        ws = [torch.empty_like(v) for v in vs]
        rows = (C.c_int * len(vs))(*[v.shape[0] for v in vs])
        cols = (C.c_int * len(vs))(*[v.numel() // v.shape[0] for v in vs])
        for k in range(0, len(vs), 32):
            n = min(32, len(vs) - k)
            _lib.check(lib.evae_weight_norm_set_fwd(n, _ptr_array(vs[k:k + n]), _ptr_array(gs[k:k + n]), _ptr_array(ws[k:k + n]),
                                                    C.byref(rows, 4 * k), C.byref(cols, 4 * k), _stream()), "evae_weight_norm_set_fwd")
        ctx.save_for_backward(*vs, *gs)
        return tuple(ws)

    @staticmethod
    def backward(ctx, *dws):
        lib = _lib.load()
        saved = ctx.saved_tensors
        n_all = len(saved) // 2
        vs, gs = list(saved[:n_all]), list(saved[n_all:])
        dws = [torch.zeros_like(v) if d is None else _f32(d) for d, v in zip(dws, vs)]
        dvs = [torch.empty_like(v) for v in vs]
        dgs = [torch.empty_like(g) for g in gs]
        rows = (C.c_int * n_all)(*[v.shape[0] for v in vs])
        cols = (C.c_int * n_all)(*[v.numel() // v.shape[0] for v in vs])
        for k in range(0, n_all, 32):
            n = min(32, n_all - k)
            _lib.check(lib.evae_weight_norm_set_bwd(n, _ptr_array(vs[k:k + n]), _ptr_array(gs[k:k + n]), _ptr_array(dws[k:k + n]),
                                                    _ptr_array(dvs[k:k + n]), _ptr_array(dgs[k:k + n]), C.byref(rows, 4 * k), C.byref(cols, 4 * k),
                                                    _stream()), "evae_weight_norm_set_bwd")
        out = []
        for dv, dg in zip(dvs, dgs):
            out += [dv, dg]
        return tuple(out)


def weight_norm_set(pairs):
    """pairs = [(v, g), ...] -> [w, ...]   (one launch; autograd through to every v and g)"""
    flat = []
    for v, g in pairs:
        flat += [v, g]
    return list(WeightNormSetFn.apply(*flat))


RES_STACK_MIN_PIXELS = int(os.environ.get("EVAE_RES_STACK_MIN_PIXELS", "16384"))


def res_stack_supported(x, weights):
    """A run of residual blocks x + conv(ELU(x)) (models/fully_conv.py:13-23) on the window kernels?  (same channel count in and
    out, stride 1, enough pixels to fill the machine)"""
    if not (CONV_STACK_ON and x.is_cuda and x.dim() == 4 and 1 <= len(weights) <= 16):      # (evae_cw_res_run_*: at most 16 blocks a call)
        return False
    N, Cc, H, W = x.shape
    if N * H * W < RES_STACK_MIN_PIXELS:
        return False
    lib = _lib.load()
    for w in weights:
        Co, Ci, KH, KW = w.shape
        if Ci != Cc or Co != Cc:
            return False
        d = _lib.ConvDesc(N, Cc, H, W, Co, KH, KW, 1, (KH - 1) // 2)
        if not lib.evae_cw_res_supported(C.byref(d)):
            return False
    return True


class ResStackFn(torch.autograd.Function):
    """A run of residual blocks x_{k+1} = x_k + conv(ELU(x_k), w_k) + b_k (reference models/fully_conv.py:13-23) on pixel images: every
    block's convolution reads the image of ELU(x_k) that the block before wrote in its epilogue (the entry packs it once), adds bias
    and residual in its own; in the backward pass one launch per block forms dx_k = dx_{k+1} + ELU'(x_k) conv_transpose(dx_{k+1}, w_k)
    -- ELU' from the saved image -- and writes it as fp32 and as the image the next block's two gradients read.  No ELU launch, no
    fp32 activation kept for the backward.  The filter images of the whole run are packed in one launch and each direction is ONE
    call into the library (evae_cw_res_run_fwd / _bwd): an eager fully_conv step waits for its host.  args: x, then (w, b) per block."""

    @staticmethod
    def forward(ctx, x, *params):
        lib = _lib.load()
        nb = len(params) // 2
        ws_ = [_f32(params[2 * k]) for k in range(nb)]
        bs_ = [params[2 * k + 1] for k in range(nb)]
        _need_cuda(x, *ws_)
        x = _cl(x.float())
        dev = x.device
        N, Cc, H, W = x.shape
        need_grad = any(ctx.needs_input_grad)
        st = _stream()
        d = _lib.ConvDesc(N, Cc, H, W, Cc, ws_[0].shape[2], ws_[0].shape[3], 1, (ws_[0].shape[2] - 1) // 2)
        assert nb <= 16 and all(tuple(w.shape) == tuple(ws_[0].shape) for w in ws_), "a run: <= 16 blocks of one shape"
        ib = int(lib.evae_cw_image_bytes(N * H * W, Cc))
        fb = int(lib.evae_cw_workspace_bytes(C.byref(d), 5))
        imgs = torch.empty((nb, ib), dtype=torch.uint8, device=dev)           # images of ELU(x_0) .. ELU(x_{nb-1})
        # x_1 .. x_nb, channels-last: block k reads x_k and writes x_{k+1}, only the last is returned -- two scratch buffers take turns for
        # the ones in between (a 6-block run at 10 000 rows of cache_z kept 2.9 GB alive through the returned view)
        y_last = torch.empty((N, H, W, Cc), device=dev)
        y_tmp = torch.empty((min(2, nb - 1), N, H, W, Cc), device=dev) if nb > 1 else None
        ys = [y_last if k == nb - 1 else y_tmp[k & 1] for k in range(nb)]
        filt = torch.empty(((2 if need_grad else 1), nb, fb), dtype=torch.uint8, device=dev)
        _lib.check(lib.evae_cw_pack_image(_p(x), N, H, W, Cc, 2, _p(imgs[0]), st), "evae_cw_pack_image(ELU)")
        _lib.check(lib.evae_cw_res_pack_filters(C.byref(d), nb, _ptr_array(ws_), _p(filt[0]), _p(filt[1]) if need_grad else None, st),
                   "evae_cw_res_pack_filters")
        VP = C.c_void_p * nb
        bias = VP(*[None if b is None else b.data_ptr() for b in bs_])
        outf = VP(*[ys[k].data_ptr() for k in range(nb)])
        oimg = VP(*[imgs[k + 1].data_ptr() if k + 1 < nb else None for k in range(nb)])
        _lib.check(lib.evae_cw_res_run_fwd(C.byref(d), nb, _p(filt[0]), bias, _p(imgs[0]), _p(x), outf, oimg, st), "evae_cw_res_run_fwd")
        if need_grad:
            ctx.save_for_backward(*ws_)
            ctx.keep = (imgs, d, [b is not None for b in bs_], filt[1])
        return y_last.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        imgs, d, has_b, bimg = ctx.keep
        ctx.keep = None
        ws_ = list(ctx.saved_tensors)
        nb = len(ws_)
        dev = dout.device
        dy = _cl(dout.float())
        N, Cc, H, W = dy.shape
        st = _stream()
        ib = imgs.shape[1]
        # image of the incoming gradient, and of dx_k (k >= 1): block k reads dx_{k+1} (fp32 and image) and writes dx_k -- two of each
        # take turns, dx_0 (the one returned) has its own fp32 buffer and no image
        dtop = torch.empty((ib,), dtype=torch.uint8, device=dev)
        _lib.check(lib.evae_cw_pack_image(_p(dy), N, H, W, Cc, 0, _p(dtop), st), "evae_cw_pack_image")
        dimg2 = torch.empty((min(2, nb - 1), ib), dtype=torch.uint8, device=dev) if nb > 1 else None
        dimgs = [None if k == 0 else dimg2[(k - 1) & 1] for k in range(nb)]
        dx0 = torch.empty((N, H, W, Cc), device=dev)
        dx_tmp = torch.empty((min(2, nb - 1), N, H, W, Cc), device=dev) if nb > 1 else None
        dxs = [dx0 if k == 0 else dx_tmp[(k - 1) & 1] for k in range(nb)]
        dws = torch.empty((nb,) + tuple(ws_[0].shape), device=dev)
        dbs = torch.empty((nb, Cc), device=dev)
        ws = _workspace("cw", lib.evae_cw_workspace_bytes(C.byref(d), 7), dev)
        VP = C.c_void_p * nb
        aim = VP(*[imgs[k].data_ptr() for k in range(nb)])
        dxf = VP(*[dxs[k].data_ptr() for k in range(nb)])
        dxi = VP(*[dimgs[k].data_ptr() if k >= 1 else None for k in range(nb)])
        dwp = VP(*[dws[k].data_ptr() for k in range(nb)])
        dbp = VP(*[dbs[k].data_ptr() for k in range(nb)])
        _lib.check(lib.evae_cw_res_run_bwd(C.byref(d), nb, _p(bimg), aim, _p(dtop), _p(dy), dxf, dxi, dwp, dbp, _p(ws), ws.numel(), st),
                   "evae_cw_res_run_bwd")
        grads = []
        for k in range(nb):
            grads += [dws[k], dbs[k] if has_b[k] else None]
        return (dx0.permute(0, 3, 1, 2) if ctx.needs_input_grad[0] else None,) + tuple(grads)


def res_stack(x, blocks):
    """blocks = [(w, b), ...] -> x after the run of residual blocks"""
    flat = []
    for w, b in blocks:
        flat += [w, b]
    return ResStackFn.apply(x, *flat)


def res_window_probe(N, Cc, H, K=3, seed=0):
    """Launch closures {fwd, dgrad, wgrad} of ONE residual block x + conv(ELU(x)) (Cc channels, H x H) on the window kernels, on
    random images prepared once (bench.py's c5 roofline timing, tools/kernel_probe.py)."""
    lib = _lib.load()
    dev = torch.device("cuda")
    g = torch.Generator(device=dev); g.manual_seed(seed)
    d = _lib.ConvDesc(N, Cc, H, H, Cc, K, K, 1, (K - 1) // 2)
    x = torch.randn((N, H, H, Cc), device=dev, generator=g)
    w = torch.randn((Cc, Cc, K, K), device=dev, generator=g) * 0.03; b = torch.zeros(Cc, device=dev)
    img = lambda: torch.empty(int(lib.evae_cw_image_bytes(N * H * H, Cc)), dtype=torch.uint8, device=dev)
    a, o, dyimg, dximg = img(), img(), img(), img()
    _lib.check(lib.evae_cw_pack_image(_p(x), N, H, H, Cc, 2, _p(a), _stream()), "evae_cw_pack_image")
    dy = torch.randn((N, H, H, Cc), device=dev, generator=g) * 0.1
    _lib.check(lib.evae_cw_pack_image(_p(dy), N, H, H, Cc, 0, _p(dyimg), _stream()), "evae_cw_pack_image")
    y = torch.empty_like(x); dx = torch.empty_like(x)
    dw = torch.empty((Cc, Cc * K * K), device=dev); db = torch.empty(Cc, device=dev)
    w5 = _workspace("cw", lib.evae_cw_workspace_bytes(C.byref(d), 5), dev)
    w7 = _workspace("cw_wgrad", lib.evae_cw_workspace_bytes(C.byref(d), 7), dev)
    return {"desc": d,
            "fwd": lambda: _lib.check(lib.evae_cw_res_fwd(_p(a), C.byref(d), _p(w), _p(b), _p(x), _p(y), _p(o), _p(w5), w5.numel(), _stream()), "evae_cw_res_fwd"),
            "dgrad": lambda: _lib.check(lib.evae_cw_res_bwd_data(_p(dyimg), C.byref(d), _p(w), _p(a), _p(dy), _p(dx), _p(dximg), _p(w5), w5.numel(),
                                                                 _stream()), "evae_cw_res_bwd_data"),
            "wgrad": lambda: _lib.check(lib.evae_cw_bwd_weight_plain(_p(dyimg), _p(a), C.byref(d), _p(dw), _p(db), _p(w7), w7.numel(), _stream()),
                                        "evae_cw_bwd_weight_plain")}


def conv_window_probe(N, Cc, H, Co, K, stride, out_planar=False, seed=0):
    """Launch closures {fwd, dgrad, wgrad} of ONE gated layer (Cc -> Co, K x K, H x H input) on the window kernels, on random
    images prepared once (bench.py's roofline timing, tools/kernel_probe.py's PMC passes): the launches a stack issues for it."""
    lib = _lib.load()
    dev = torch.device("cuda")
    g = torch.Generator(device=dev); g.manual_seed(seed)
    pad, OH = (K - 1) // 2, H // stride
    d = _lib.ConvDesc(N, Cc, H, H, Co, K, K, stride, pad)
    x = torch.randn((N, H, H, Cc), device=dev, generator=g)
    wh = torch.randn((Co, Cc, K, K), device=dev, generator=g) * 0.03; wg = torch.randn((Co, Cc, K, K), device=dev, generator=g) * 0.03
    b = torch.zeros(Co, device=dev)
    img = lambda rows, ch: torch.empty(int(lib.evae_cw_image_bytes(rows, ch)), dtype=torch.uint8, device=dev)
    ximg = img(N * H * H, Cc)
    _lib.check(lib.evae_cw_pack_image(_p(x), N, H, H, Cc, int(stride == 2), _p(ximg), _stream()), "evae_cw_pack_image")
    oimg = img(N * OH * OH, Co); s = torch.empty((N, OH, OH, Co), device=dev)
    dy = torch.randn((N, OH, OH, 2 * Co), device=dev, generator=g) * 0.1
    dyimg = img(N * OH * OH, 2 * Co)
    _lib.check(lib.evae_cw_pack_image(_p(dy), N, OH, OH, 2 * Co, int(out_planar), _p(dyimg), _stream()), "evae_cw_pack_image")
    es = torch.rand((N, H, H, Cc), device=dev, generator=g)
    dimg = img(N * H * H, 2 * Cc)
    dw = torch.empty((2 * Co, Cc * K * K), device=dev); db = torch.empty(2 * Co, device=dev)
    del x, dy
    ws = {w: _workspace("cw", lib.evae_cw_workspace_bytes(C.byref(d), w), dev) for w in (0, 1, 2) if lib.evae_cw_supported(C.byref(d), w)}
    out = {"desc": d}
    if 0 in ws:
        out["fwd"] = lambda: _lib.check(lib.evae_cw_fwd_gated(_p(ximg), C.byref(d), _p(wh), _p(b), _p(wg), _p(b), _p(oimg), int(out_planar), _p(s),
                                                              None, _p(ws[0]), ws[0].numel(), _stream()), "evae_cw_fwd_gated")
    if 1 in ws:
        out["dgrad"] = lambda: _lib.check(lib.evae_cw_bwd_data_gate(_p(dyimg), int(out_planar), C.byref(d), _p(wh), _p(wg), _p(ximg), _p(es), _p(dimg),
                                                                    None, _p(ws[1]), ws[1].numel(), _stream()), "evae_cw_bwd_data_gate")
    if 2 in ws:
        out["wgrad"] = lambda: _lib.check(lib.evae_cw_bwd_weight(_p(dyimg), int(out_planar), _p(ximg), C.byref(d), _p(dw), _p(db), _p(ws[2]),
                                                                 ws[2].numel(), _stream()), "evae_cw_bwd_weight")
    return out


def gated_conv_stack(x, layers):
    """layers = [(wh, bh, wg, bg, stride, pad), ...] -> output of the last one (logical NCHW, channels-last storage)"""
    cfg = tuple((_int1(l[4]), _int1(l[5])) for l in layers)
    flat = []
    for l in layers:
        flat += [l[0], l[1], l[2], l[3]]
    return GatedConvStackFn.apply(x, cfg, *flat)


# ------------------------------------------------------------------------------------------------
# latent sampling / log-densities
# ------------------------------------------------------------------------------------------------
class ReparamLogQ(torch.autograd.Function):
    """(mu, logvar, eps) -> (z = mu + eps*exp(logvar/2), log q(z|x))."""

    @staticmethod
    def forward(ctx, mu, logvar, eps):
        lib = _lib.load()
        _need_cuda(mu, logvar, eps)
        mu, logvar, eps = _f32(mu), _f32(logvar), _f32(eps)
        B, zd = mu.shape
        z = torch.empty_like(mu); logq = torch.empty(B, device=mu.device)
        _lib.check(lib.evae_reparam_logq_fwd(_p(mu), _p(logvar), _p(eps), B, zd, _p(z), _p(logq), _stream()),
                   "evae_reparam_logq_fwd")
        ctx.save_for_backward(mu, logvar, eps, z)
        return z, logq

    @staticmethod
    def backward(ctx, dz, dlogq):
        lib = _lib.load()
        mu, logvar, eps, z = ctx.saved_tensors
        B, zd = mu.shape
        dz = None if dz is None else _f32(dz)
        dlogq = None if dlogq is None else _f32(dlogq)
        dmu = torch.empty_like(mu); dlv = torch.empty_like(mu)
        _lib.check(lib.evae_reparam_logq_bwd(_p(mu), _p(logvar), _p(eps), _p(z), _p(dz), _p(dlogq), B, zd,
                                             _p(dmu), _p(dlv), _stream()), "evae_reparam_logq_bwd")
        return dmu, dlv, None


class HeadsReparamFn(torch.autograd.Function):
    """(h, wm, bm, wl, bl, eps) -> (z, z_mean, logvar, log q(z | .)): the mean head, the Hardtanh(lo, hi) log-variance head, the
    sample and its log-density (reference models/VAE.py:24-26 / AbsHModel.py:22-29, BaseModel.py:79-82, utils/distributions.py:
    28-33) as evae_heads_reparam_fwd's two launches (separately: 2 linear layers x 2, the sample, the density = 6), and a
    backward of four (evae_reparam_logq_bwd_hardtanh, one data gradient over both heads, one grouped weight gradient)
    where the separate Functions take thirteen."""

    @staticmethod
    def forward(ctx, h, wm, bm, wl, bl, eps, lo, hi):
        lib = _lib.load()
        _need_cuda(h, wm, wl, eps)
        h, wm, wl, eps = _f32(h), _f32(wm), _f32(wl), _f32(eps)
        if h.stride(1) != 1:
            h = h.contiguous()
        M, K = h.shape
        Z = wm.shape[0]
        assert wl.shape == wm.shape and wm.shape[1] == K and eps.shape == (M, Z) and eps.is_contiguous()
        z_mean = torch.empty((M, Z), device=h.device); lv_pre = torch.empty_like(z_mean); logvar = torch.empty_like(z_mean)
        z = torch.empty_like(z_mean); logq = torch.empty(M, device=h.device)
        ws = _workspace("heads", lib.evae_heads_reparam_fwd_workspace_bytes(M, K, Z), h.device)
        _lib.check(lib.evae_heads_reparam_fwd(_p(h), M, K, h.stride(0), _p(wm), _p(bm), _p(wl), _p(bl), Z, float(lo), float(hi),
                                              _p(eps), _p(z_mean), _p(lv_pre), _p(logvar), _p(z), _p(logq), _p(ws), ws.numel(),
                                              _stream()), "evae_heads_reparam_fwd")
        ctx.save_for_backward(h, wm, wl, z_mean, lv_pre, logvar, eps, z)
        ctx.set_materialize_grads(False)           # unused outputs (the moments, on the training path) arrive as None, not as zeros
        ctx.clamp = (float(lo), float(hi))
        ctx.has_bias = (bm is not None, bl is not None)
        return z, z_mean, logvar, logq

    @staticmethod
    def backward(ctx, dz, dmean, dlogvar, dlogq):
        lib = _lib.load()
        h, wm, wl, z_mean, lv_pre, logvar, eps, z = ctx.saved_tensors
        lo, hi = ctx.clamp
        M, K = h.shape
        Z = wm.shape[0]
        if dz is None and dmean is None and dlogvar is None and dlogq is None:
            return (None,) * 8
        dz = None if dz is None else _f32(dz)
        dlogq = None if dlogq is None else _f32(dlogq)
        dmu = torch.empty_like(z_mean); dlvp = torch.empty_like(z_mean)
        _lib.check(lib.evae_reparam_logq_bwd_hardtanh(_p(z_mean), _p(logvar), _p(eps), _p(z), _p(dz), None, _p(dlogq), _p(lv_pre),
                                                      lo, hi, M, Z, _p(dmu), _p(dlvp), _stream()), "evae_reparam_logq_bwd_hardtanh")
        if dmean is not None:                       # a consumer of the moments themselves (none on the training path)
            dmu = dmu + dmean
        if dlogvar is not None:
            dlvp = dlvp + dlogvar * ((lv_pre > lo) & (lv_pre < hi))
        return _heads_bwd(h, wm, wl, dmu, dlvp, ctx.needs_input_grad[0], ctx.has_bias) + (None, None, None)


def heads_reparam(h, wm, bm, wl, bl, eps, lo, hi):
    return HeadsReparamFn.apply(h, wm, bm, wl, bl, eps, lo, hi)


def _heads_bwd(h, wm, wl, dmu, dlvp, want_dh, has_bias):
    """what the two heads' backward shares: dh over both heads in one data gradient, both weight gradients in one grouped launch"""
    M, K = h.shape
    Z = wm.shape[0]
    dh = _bwd_data(dmu, wm, dlvp, wl, M, Z, Z, h.device) if want_dh else None
    if M <= 128 and Z % 4 == 0 and K % 4 == 0 and h.stride(0) % 4 == 0:
        # each head on its own: deferred behind the backward pass when its weight allows (ops.deferred_wgrads; the mean head of
        # q(z2 | x) also encodes the exemplar rows and does not), what is left as one grouped launch here
        res, now = {}, []
        for name, dy_, w_ in (("m", dmu, wm), ("l", dlvp, wl)):
            d = _try_defer(dy_, h, K, w_.data_ptr())
            if d is not None:
                res[name] = d
            else:
                dw_ = torch.empty((Z, K), device=h.device); db_ = torch.empty(Z, device=h.device)
                res[name] = (dw_, db_); now.append((dy_, M, Z, dy_.stride(0), h, K, h.stride(0), dw_, db_))
        if now:
            launch.Launcher(h.device).bwd_weight_group(now)
        (dwm, dbm), (dwl, dbl) = res["m"], res["l"]
    else:
        dwm, dbm = _bwd_weight(dmu, h, None, K)
        dwl, dbl = _bwd_weight(dlvp, h, None, K)
    return dh, dwm, (dbm if has_bias[0] else None), dwl, (dbl if has_bias[1] else None)


class HeadsDensityFn(torch.autograd.Function):
    """(h, wm, bm, wl, bl, zq) -> (z_mean, logvar, log N(zq | z_mean, exp(logvar))): the conditional p(z1 | z2) of the 2-level models
    (reference models/AbsHModel.py:17-20) with the density term of kl_loss (:99-100) -- evae_heads_density_fwd's two launches
    forward (two linear layers x 2 + the density = 5 separately), evae_log_normal_diag_bwd_hardtanh + one data gradient + one
    grouped weight gradient backward (10 separately)."""

    @staticmethod
    def forward(ctx, h, wm, bm, wl, bl, zq, lo, hi):
        lib = _lib.load()
        _need_cuda(h, wm, wl, zq)
        h, wm, wl, zq = _f32(h), _f32(wm), _f32(wl), _f32(zq)
        M, K = h.shape
        Z = wm.shape[0]
        assert wl.shape == wm.shape and wm.shape[1] == K and zq.shape == (M, Z)
        z_mean = torch.empty((M, Z), device=h.device); lv_pre = torch.empty_like(z_mean); logvar = torch.empty_like(z_mean)
        logp = torch.empty(M, device=h.device)
        ws = _workspace("heads", lib.evae_heads_reparam_fwd_workspace_bytes(M, K, Z), h.device)
        _lib.check(lib.evae_heads_density_fwd(_p(h), M, K, h.stride(0), _p(wm), _p(bm), _p(wl), _p(bl), Z, float(lo), float(hi), _p(zq),
                                              _p(z_mean), _p(lv_pre), _p(logvar), _p(logp), _p(ws), ws.numel(), _stream()),
                   "evae_heads_density_fwd")
        ctx.save_for_backward(h, wm, wl, z_mean, lv_pre, logvar, zq)
        ctx.set_materialize_grads(False)
        ctx.clamp = (float(lo), float(hi))
        ctx.has_bias = (bm is not None, bl is not None)
        return z_mean, logvar, logp

    @staticmethod
    def backward(ctx, dmean, dlogvar, dlogp):
        lib = _lib.load()
        if dmean is None and dlogvar is None and dlogp is None:
            return (None,) * 8
        h, wm, wl, z_mean, lv_pre, logvar, zq = ctx.saved_tensors
        lo, hi = ctx.clamp
        M, Z = z_mean.shape
        dz = None
        if dlogp is not None:
            dmu = torch.empty_like(z_mean); dlvp = torch.empty_like(z_mean)
            dz = torch.empty_like(z_mean) if ctx.needs_input_grad[5] else None
            _lib.check(lib.evae_log_normal_diag_bwd_hardtanh(_p(zq), _p(z_mean), _p(logvar), _p(lv_pre), lo, hi, _p(_f32(dlogp)), M, Z,
                                                             _p(dz), _p(dmu), _p(dlvp), _stream()), "evae_log_normal_diag_bwd_hardtanh")
        else:
            dmu = torch.zeros_like(z_mean); dlvp = torch.zeros_like(z_mean)
        if dmean is not None:
            dmu = dmu + dmean
        if dlogvar is not None:
            dlvp = dlvp + dlogvar * ((lv_pre > lo) & (lv_pre < hi))
        dh, dwm, dbm, dwl, dbl = _heads_bwd(h, wm, wl, dmu, dlvp, ctx.needs_input_grad[0], ctx.has_bias)
        return dh, dwm, dbm, dwl, dbl, dz, None, None


def heads_density(h, wm, bm, wl, bl, zq, lo, hi):
    return HeadsDensityFn.apply(h, wm, bm, wl, bl, zq, lo, hi)


class ElboFn(torch.autograd.Function):
    """(RE, log q1, log p1[, log q2, log p2], beta) -> KL = (log q1 - log p1) [+ (log q2 - log p2)], loss = beta KL - RE, and with
    `average` their batch means (reference models/BaseModel.py:71-77, AbsHModel.py:88-106): one launch each way (evae_elbo_fwd /
    evae_elbo2_fwd, evae_elbo_bwd) where the tensor expressions take eight and ten.  Returns (loss, KL) per row, or the three
    means (loss, RE, KL) as 0-d tensors.  beta: a number, or a one-element device tensor (captured steps); no gradient."""

    @staticmethod
    def forward(ctx, RE, lq1, lp1, lq2, lp2, beta, average):
        lib = _lib.load()
        _need_cuda(RE, lq1, lp1)
        RE, lq1, lp1 = _f32(RE).contiguous(), _f32(lq1).contiguous(), _f32(lp1).contiguous()
        two = lq2 is not None
        if two:
            lq2, lp2 = _f32(lq2).contiguous(), _f32(lp2).contiguous()
        B = RE.numel()
        assert RE.dim() == 1 and all(t is None or t.shape == RE.shape for t in (lq1, lp1, lq2, lp2))
        beta_dev = beta if torch.is_tensor(beta) else None
        beta_host = 0.0 if beta_dev is not None else float(beta)
        loss = torch.empty(B, device=RE.device); KL = torch.empty_like(loss)
        means = torch.empty(3, device=RE.device) if average else None
        if two:
            _lib.check(lib.evae_elbo2_fwd(_p(RE), _p(lq1), _p(lp1), _p(lq2), _p(lp2), _p(beta_dev), beta_host, B, _p(loss), _p(KL),
                                          _p(means), _stream()), "evae_elbo2_fwd")
        else:
            _lib.check(lib.evae_elbo_fwd(_p(RE), _p(lq1), _p(lp1), _p(beta_dev), beta_host, B, _p(loss), _p(KL), _p(means),
                                         _stream()), "evae_elbo_fwd")
        ctx.meta = (B, two, bool(average), beta_host)
        ctx.set_materialize_grads(False)
        ctx.beta_dev = beta_dev
        if average:
            return means[0], means[1], means[2]
        return loss, KL

    @staticmethod
    def backward(ctx, *grads):
        lib = _lib.load()
        B, two, average, beta_host = ctx.meta
        if average:
            gl, gr, gk = (None if g is None else _f32(g).contiguous() for g in grads)
        else:
            gl, gk = (None if g is None else _f32(g).contiguous() for g in grads)
            gr = None
        if gl is None and gr is None and gk is None:
            return (None,) * 7
        dev = next(g for g in (gl, gr, gk) if g is not None).device
        coef = torch.empty((3, B), device=dev)
        n = lambda g: 0 if g is None else g.numel()
        _lib.check(lib.evae_elbo_bwd(_p(gl), n(gl), _p(gr), n(gr), _p(gk), n(gk), _p(ctx.beta_dev), beta_host, B, _p(coef[0]),
                                     _p(coef[1]), _p(coef[2]), _stream()), "evae_elbo_bwd")
        need = ctx.needs_input_grad
        pick = lambda i, row: coef[row] if need[i] else None
        return (pick(0, 0), pick(1, 1), pick(2, 2), pick(3, 1) if two else None, pick(4, 2) if two else None, None, None)


def elbo(RE, logq, logp, beta, average, logq2=None, logp2=None):
    """-> (loss, RE, KL) of models/BaseModel.py:71-77, per row or as batch means"""
    if average:
        return ElboFn.apply(RE, logq, logp, logq2, logp2, beta, True)
    loss, KL = ElboFn.apply(RE, logq, logp, logq2, logp2, beta, False)
    return loss, RE, KL


class LogNormalDiag(torch.autograd.Function):
    """utils/distributions.py:28-33 summed over dim=1 for [B x z] inputs."""

    @staticmethod
    def forward(ctx, x, mu, logvar):
        lib = _lib.load()
        _need_cuda(x, mu, logvar)
        x, mu, logvar = _f32(x), _f32(mu), _f32(logvar)
        B, zd = x.shape
        out = torch.empty(B, device=x.device)
        _lib.check(lib.evae_log_normal_diag_fwd(_p(x), _p(mu), _p(logvar), B, zd, _p(out), _stream()),
                   "evae_log_normal_diag_fwd")
        ctx.save_for_backward(x, mu, logvar)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        x, mu, logvar = ctx.saved_tensors
        B, zd = x.shape
        g = _f32(g)
        need = ctx.needs_input_grad
        dx = torch.empty_like(x) if need[0] else None
        dmu = torch.empty_like(x) if need[1] else None
        dlv = torch.empty_like(x) if need[2] else None
        _lib.check(lib.evae_log_normal_diag_bwd(_p(x), _p(mu), _p(logvar), _p(g), B, zd, _p(dx), _p(dmu), _p(dlv),
                                                _stream()), "evae_log_normal_diag_bwd")
        return dx, dmu, dlv


class LogNormalStandard(torch.autograd.Function):
    """utils/distributions.py:36-41 summed over dim=1 for [B x z] inputs: LogNormalDiag with mean = logvar = 0, without the zeros."""

    @staticmethod
    def forward(ctx, x):
        lib = _lib.load()
        _need_cuda(x)
        x = _f32(x)
        B, zd = x.shape
        out = torch.empty(B, device=x.device)
        _lib.check(lib.evae_log_normal_std_fwd(_p(x), B, zd, _p(out), _stream()), "evae_log_normal_std_fwd")
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        x, = ctx.saved_tensors
        B, zd = x.shape
        g = _f32(g)
        dx = torch.empty_like(x)
        _lib.check(lib.evae_log_normal_std_bwd(_p(x), _p(g), B, zd, _p(dx), _stream()), "evae_log_normal_std_bwd")
        return dx


class BernoulliLL(torch.autograd.Function):
    """utils/distributions.py:44-51 summed over dim=1: x [B x D] (no grad), mean [B x D]."""

    @staticmethod
    def forward(ctx, x, mean):
        lib = _lib.load()
        _need_cuda(x, mean)
        x, mean = _f32(x), _f32(mean)
        B, D = mean.shape
        out = torch.empty(B, device=mean.device)
        _lib.check(lib.evae_bernoulli_ll_fwd(_p(x), _p(mean), B, D, _p(out), _stream()), "evae_bernoulli_ll_fwd")
        ctx.save_for_backward(x, mean)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        x, mean = ctx.saved_tensors
        B, D = mean.shape
        g = _f32(g)
        dmean = torch.empty_like(mean)
        _lib.check(lib.evae_bernoulli_ll_bwd(_p(x), _p(mean), _p(g), B, D, _p(dmean), _stream()),
                   "evae_bernoulli_ll_bwd")
        return None, dmean


class LogLogistic256(torch.autograd.Function):
    """utils/distributions.py:54-66 summed over dim=1: x [B x D] (no grad), mean [B x D], logvar [B x D] or one value."""

    @staticmethod
    def forward(ctx, x, mean, logvar):
        lib = _lib.load()
        _need_cuda(x, mean, logvar)
        x, mean, logvar = _f32(x), _f32(mean), _f32(logvar)
        B, D = mean.shape
        scalar = logvar.numel() == 1
        assert scalar or logvar.shape == mean.shape
        out = torch.empty(B, device=mean.device)
        _lib.check(lib.evae_log_logistic256_fwd(_p(x), _p(mean), _p(logvar), int(scalar), B, D, _p(out), _stream()),
                   "evae_log_logistic256_fwd")
        ctx.save_for_backward(x, mean, logvar)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        x, mean, logvar = ctx.saved_tensors
        B, D = mean.shape
        scalar = logvar.numel() == 1
        g = _f32(g)
        dmean = torch.empty_like(mean) if ctx.needs_input_grad[1] else None
        dlv = torch.empty_like(logvar) if ctx.needs_input_grad[2] else None
        rows = torch.empty(B, device=mean.device) if (scalar and dlv is not None) else None
        _lib.check(lib.evae_log_logistic256_bwd(_p(x), _p(mean), _p(logvar), int(scalar), _p(g), B, D, _p(dmean), _p(dlv),
                                                _p(rows), _stream()), "evae_log_logistic256_bwd")
        return None, dmean, dlv


# ------------------------------------------------------------------------------------------------
# AdamNormGrad
# ------------------------------------------------------------------------------------------------
def adam_step_size(step, lr, beta1, beta2):
    """lr * sqrt(1 - beta2^t) / (1 - beta1^t)  (reference utils/optimizer.py:74-76)."""
    return lr * (1.0 - beta2 ** step) ** 0.5 / (1.0 - beta1 ** step)


def step_stats_add(loss, re, kl, step3, totals3=None):
    """step3 <- (loss, -re, kl); totals3 += step3 (the per-epoch sums of utils/training.py:41-46, kept on the device)."""
    _need_cuda(loss, re, kl, step3, totals3)
    _lib.check(_lib.load().evae_step_stats_add(_p(loss), _p(re), _p(kl), _p(step3), _p(totals3), _stream()), "step_stats_add")
    return step3


def batch_prologue(data, idx, binarize, seed_ctr, x_out, eps_out=None):
    """Head of a training step in one launch: x_out[b] = (binarised) data[idx[b]], eps_out ~ N(0, 1).
    seed_ctr: device int64 [2] = (seed, step counter) of the counter-based generator."""
    lib = _lib.load()
    _need_cuda(data, idx, seed_ctr, x_out)
    B, D = x_out.shape
    assert data.dtype == torch.float32 and x_out.dtype == torch.float32 and data.stride(1) == 1 and x_out.stride(1) == 1
    assert idx.dtype == torch.int64 and idx.is_contiguous() and idx.numel() == B and seed_ctr.dtype == torch.int64
    zd = 0
    if eps_out is not None:
        assert eps_out.is_contiguous() and eps_out.dtype == torch.float32 and eps_out.shape[0] == B
        zd = eps_out.shape[1]
    _lib.check(lib.evae_batch_prologue(_p(data), data.stride(0), _p(idx), B, D, 1 if binarize else 0, _p(seed_ctr),
                                       _p(x_out), x_out.stride(0), _p(eps_out), zd, _stream()), "evae_batch_prologue")
    return x_out, eps_out


def batch_prologue_u8(data_u8, idx, binarize, seed_ctr, x_div, x_out, stage_u8, eps_out=None, prepare=None, ctl_job=None, packs=None):
    """batch_prologue on the uint8-resident store: x_out [B x D] fp32 and the batch's bytes into stage_u8 [B x D].
    prepare = (wh, wg, out): the same launch also splits the first layer's weights (u8_prepare) into `out`.
    ctl_job = (stage0, stage1, ctl, state, idx_word, seed_word): the same launch hands over a captured step's control block
    (evae_batch_prologue_u8_step): idx / seed_ctr are then read from the staging block the device-side parity names.
    packs (with ctl_job only) = [(cols, x, x2 or None, R, K, ld, flag, nks, img)]: weight images of the pre-split GEMMs built by the
    same launch (evae_p6_pack_rows / _cols)."""
    lib = _lib.load()
    _need_cuda(data_u8, idx, seed_ctr, x_out, stage_u8)
    B, D = x_out.shape
    assert data_u8.dtype == torch.uint8 and stage_u8.dtype == torch.uint8 and data_u8.stride(1) == 1 and stage_u8.stride(1) == 1
    assert x_out.dtype == torch.float32 and x_out.stride(1) == 1 and tuple(stage_u8.shape) == (B, D)
    assert idx.dtype == torch.int64 and idx.is_contiguous() and idx.numel() == B and seed_ctr.dtype == torch.int64
    zd = 0
    if eps_out is not None:
        assert eps_out.is_contiguous() and eps_out.dtype == torch.float32 and eps_out.shape[0] == B
        zd = eps_out.shape[1]
    wh = wg = out = None
    jobs, arr = [], None
    if prepare is not None:
        wh, wg, out = prepare[:3]
        jobs = prepare[3] if len(prepare) > 3 else []        # [(w1, w2 or None, dst)]: transposed weights for the data gradients
        _need_cuda(wh, wg, out)
        assert wh.dtype == torch.float32 and wh.is_contiguous() and wg.is_contiguous() and wh.shape == wg.shape
        arr = (_lib.WtJob * max(len(jobs), 1))()
        for i, (w1, w2, dst) in enumerate(jobs):
            assert w1.is_contiguous() and (w2 is None or (w2.is_contiguous() and w2.shape == w1.shape))
            arr[i].w1 = w1.data_ptr(); arr[i].w2 = None if w2 is None else w2.data_ptr(); arr[i].dst = dst.data_ptr()
            arr[i].N, arr[i].K = w1.shape
            arr[i].ldt = lib.evae_dense_bwd_data_wt_ld(w1.shape[0])
            assert dst.numel() * dst.element_size() >= lib.evae_dense_bwd_data_wt_bytes(w1.shape[0], w1.shape[1], 1 if w2 is None else 2)
    N, K = (wh.shape if wh is not None else (0, 0))
    if ctl_job is not None:
        s0, s1, ctl, state, idx_word, seed_word = ctl_job
        _need_cuda(s0, s1, ctl, state)
        assert s0.dtype == s1.dtype == ctl.dtype == torch.int64 and s0.numel() == s1.numel() == ctl.numel() and ctl.numel() % 2 == 0
        assert state.dtype == torch.int32 and state.numel() >= 2 and s0.is_contiguous() and s1.is_contiguous() and ctl.is_contiguous()
        cj = _lib.CtlJob(s0.data_ptr(), s1.data_ptr(), ctl.data_ptr(), ctl.numel() * 8, state.data_ptr(), int(idx_word), int(seed_word))
        packs = packs or []
        parr = (_lib.P6PackJob * max(len(packs), 1))()
        for i, (cols, px, px2, pr, pk, pld, pflag, pnks, pimg) in enumerate(packs):
            _need_cuda(px, px2, pimg)
            assert px.dtype == torch.float32 and px.is_contiguous() and (px2 is None or px2.is_contiguous())
            parr[i].x = px.data_ptr(); parr[i].x2 = None if px2 is None else px2.data_ptr(); parr[i].img = pimg.data_ptr()
            parr[i].img_bytes = pimg.numel() * pimg.element_size(); parr[i].ld = int(pld); parr[i].cols = 1 if cols else 0
            parr[i].R, parr[i].K, parr[i].flag, parr[i].nks = int(pr), int(pk), int(pflag), int(pnks)
        _lib.check(lib.evae_batch_prologue_u8_step(_p(data_u8), data_u8.stride(0), B, D, 1 if binarize else 0, float(x_div), _p(x_out),
                                                   x_out.stride(0), _p(stage_u8), stage_u8.stride(0), _p(eps_out), zd, _p(wh), _p(wg),
                                                   N, K, _p(out), out.numel() if out is not None else 0,
                                                   C.cast(arr, C.c_void_p) if jobs else None, len(jobs), C.addressof(cj),
                                                   C.cast(parr, C.c_void_p) if packs else None, len(packs), _stream()),
                   "evae_batch_prologue_u8_step")
        return x_out, eps_out
    assert not packs, "batch_prologue_u8: image jobs ride with the control block's hand-over only"
    if prepare is not None:
        _lib.check(lib.evae_batch_prologue_u8_prepare(_p(data_u8), data_u8.stride(0), _p(idx), B, D, 1 if binarize else 0,
                                                      _p(seed_ctr), float(x_div), _p(x_out), x_out.stride(0), _p(stage_u8),
                                                      stage_u8.stride(0), _p(eps_out), zd, _p(wh), _p(wg), N, K,
                                                      _p(out), out.numel(), C.cast(arr, C.c_void_p) if jobs else None, len(jobs),
                                                      _stream()), "evae_batch_prologue_u8_prepare")
        return x_out, eps_out
    _lib.check(lib.evae_batch_prologue_u8(_p(data_u8), data_u8.stride(0), _p(idx), B, D, 1 if binarize else 0, _p(seed_ctr),
                                          float(x_div), _p(x_out), x_out.stride(0), _p(stage_u8), stage_u8.stride(0),
                                          _p(eps_out), zd, _stream()), "evae_batch_prologue_u8")
    return x_out, eps_out


def adam_flush_tables(table_caches):
    """Upload the pointer tables that adam_normgrad_step prepared while a hipGraph was being captured (call after the
    capture has ended and before the first replay)."""
    for tc in table_caches:
        if tc.get("pending"):
            tc["table"].copy_(tc["pinned"])
            tc["pending"] = False


def adam_normgrad_step(params, grads, exp_avgs, exp_avg_sqs, step, lr, beta1, beta2, eps, weight_decay,
                       table_cache=None, step_size_dev=None, stats=None):
    """One multi-tensor AdamNormGrad update (utils/optimizer.py:32-80).  `table_cache` (a dict) lets the
    caller reuse the device pointer table while the tensor addresses stay the same.  `stats` = (loss, re, kl, step3, totals3[, toggle]):
    the update's last launch also does step_stats_add's work (the captured training step: one launch less at its tail)."""
    lib = _lib.load()
    n = len(params)
    if n == 0:
        return
    dev = params[0].device
    _need_cuda(*params)
    key = tuple(t.data_ptr() for ts in (params, grads, exp_avgs, exp_avg_sqs) for t in ts)
    if table_cache is None:
        table_cache = {}
    nbytes = C.sizeof(_lib.AdamTensor) * n
    if "table" not in table_cache:
        # device table + a pinned staging buffer, both allocated eagerly (allocation is illegal while a
        # hipGraph is being captured; the copies below are not)
        table_cache["table"] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        table_cache["pinned"] = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        table_cache["key"] = None
    table = table_cache["table"]
    if table_cache["key"] != key:
        arr = (_lib.AdamTensor * n)()
        for i in range(n):
            assert grads[i].is_contiguous() and params[i].is_contiguous()
            arr[i].param = params[i].data_ptr(); arr[i].grad = grads[i].data_ptr()
            arr[i].exp_avg = exp_avgs[i].data_ptr(); arr[i].exp_avg_sq = exp_avg_sqs[i].data_ptr()
            arr[i].numel = params[i].numel()
        if torch.cuda.is_current_stream_capturing():
            # the captured launches read the table at replay time and its content (the addresses of this capture's
            # buffers) never changes afterwards: keep the bytes in the pinned buffer and let the caller upload them ONCE
            # after the capture (adam_flush_tables) instead of capturing a memcpy node that every replay would pay for
            C.memmove(table_cache["pinned"].data_ptr(), C.addressof(arr), nbytes)
            table_cache["pending"] = True
        else:
            # eager steps: autograd hands out fresh gradient tensors every step, so the table changes every step.  A copy
            # from pageable memory would hold the host until the stream has drained (the whole backward pass); a small
            # ring of pinned staging buffers keeps the upload asynchronous, and a slot is reused only after its copy ran.
            ring = table_cache.setdefault("ring", [])
            slot = table_cache.get("ring_next", 0)
            if len(ring) <= slot:
                ring.append([torch.empty(nbytes, dtype=torch.uint8).pin_memory(), None])
            pinned, ev = ring[slot]
            if ev is not None:
                ev.synchronize()
            C.memmove(pinned.data_ptr(), C.addressof(arr), nbytes)
            table.copy_(pinned, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            ring[slot][1] = ev
            table_cache["ring_next"] = (slot + 1) % 4
        table_cache["key"] = key
    nb = lib.evae_adam_normgrad_workspace_bytes(n)
    ws = _workspace("adam", nb, dev)
    if stats is not None:
        loss, re, kl, step3, totals3 = stats[:5]
        toggle = stats[5] if len(stats) > 5 else None       # int32 device word the launch XORs with 1 (evae/graph.py's hand-over)
        assert toggle is None or (toggle.dtype == torch.int32 and toggle.is_cuda)
        _lib.check(lib.evae_adam_normgrad_step_stats(_p(table), n, max(p.numel() for p in params), int(step), float(lr),
                                                     float(beta1), float(beta2), float(eps), float(weight_decay),
                                                     _p(step_size_dev), _p(ws), ws.numel(), _p(loss), _p(re), _p(kl), _p(step3),
                                                     _p(totals3), _p(toggle), _stream()), "evae_adam_normgrad_step_stats")
        return
    _lib.check(lib.evae_adam_normgrad_step(_p(table), n, max(p.numel() for p in params), int(step), float(lr),
                                           float(beta1), float(beta2), float(eps), float(weight_decay),
                                           _p(step_size_dev), _p(ws), ws.numel(), _stream()),
               "evae_adam_normgrad_step")


# ------------------------------------------------------------------------------------------------
# PixelSNAIL decoder (utils/nn.py: CausalAttention, GatedResBlock): csrc/evae_attn.hip
# ------------------------------------------------------------------------------------------------
_DROPOUT_CALLS = [0]
_DROPOUT_SALT = [0]        # added to the seed of every eager mask of this process; 0: the masks of torch.manual_seed alone
RANK_SALT = 0x9E3779B97F4A7C15      # per-rank noise: seed + RANK_SALT * (rank + 1), the fold of the captured runner (evae/graph.py)


def dropout_salt(salt=None):
    """The process-level salt of dropout_rng(); with an argument, set it first.  Data-parallel batches (args.shard_batch) set
    rank_salt(rank): torch.initial_seed() has to be the same on every rank (the common exemplar draw), and ranks that hold different
    images must not drop the same elements.  Replicated batches keep 0: their ranks need identical masks."""
    if salt is not None:
        _DROPOUT_SALT[0] = int(salt) & 0xFFFFFFFFFFFFFFFF
    return _DROPOUT_SALT[0]


def rank_salt(rank):
    return (RANK_SALT * (int(rank) + 1)) & 0xFFFFFFFFFFFFFFFF


def dropout_rng():
    """(seed, offset) of the next dropout mask: the seed of torch.manual_seed (plus the process's salt, dropout_salt), and a
    per-process counter that every dropout call advances (it is the high half of the Philox counter, so no two calls of a
    process share a mask)."""
    off = _DROPOUT_CALLS[0]
    _DROPOUT_CALLS[0] = off + 1
    return (int(torch.initial_seed()) + _DROPOUT_SALT[0]) & 0xFFFFFFFFFFFFFFFF, off


class StepRng(collections.namedtuple("StepRng", "seed_ctr ordinal")):
    """A dropout mask whose Philox words come from DEVICE memory (the *_dev launches of csrc/evae_attn.hip): `seed_ctr`, an int64
    device tensor [seed, step counter] -- the field of that name in a step runner's control block (evae/graph.py) --, and the
    ordinal of the mask within the step.  The mask is that of the host pair (seed, dropout_step_offset(counter, ordinal))."""
    __slots__ = ()


def dropout_step_offset(counter, ordinal):
    """the Philox offset of mask `ordinal` of step `counter`: the library's evae_dropout_step_offset, the one statement of it"""
    if not 0 <= int(ordinal) < 65536:
        raise _lib.EvaeError("dropout ordinal %d does not fit the step offset (< 65536)" % int(ordinal))
    return int(_lib.load().evae_dropout_step_offset(int(counter) & 0xFFFFFFFFFFFFFFFF, int(ordinal)))


def _rng_args(p_drop, rng):
    """(p_drop, seed, offset, seed_ctr) of one dropout call.  p_drop = 0 draws nothing (and leaves every counter alone).  Inside a
    step whose runner installed a dropout source (evae/handoff.py) a call without an explicit rng takes the source's next ordinal:
    seed_ctr is its device block, `offset` carries the ordinal, and the process counter of dropout_rng() stays where it is.  An
    explicit rng is a host pair (seed, offset) or a StepRng."""
    p_drop = float(p_drop)
    if p_drop == 0.0:
        return 0.0, 0, 0, None
    if rng is None:
        h = handoff.current()
        if h is not None and h.dropout is not None:
            rng = StepRng(h.dropout.seed_ctr, h.dropout.take())
    if isinstance(rng, StepRng):
        return p_drop, 0, int(rng.ordinal), rng.seed_ctr
    seed, offset = dropout_rng() if rng is None else rng
    return p_drop, int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFFFFFFFFFF, None


def _seed_ctr_ptr(seed_ctr):
    if not (seed_ctr.is_cuda and seed_ctr.dtype == torch.int64 and seed_ctr.numel() >= 2 and seed_ctr.is_contiguous()):
        raise _lib.EvaeError("dropout: seed_ctr must be a contiguous int64 device tensor [seed, step counter]")
    return _p(seed_ctr)


def causal_attn_max_len():
    return int(_lib.load().evae_causal_attn_max_len())


class CausalAttnFn(torch.autograd.Function):
    """Causal attention of reference utils/nn.py:351-359 on projected rows: q, k, v [B*L, H*dh] -> out [B*L, H*dh].  Saves q, k, v,
    out and one log-sum-exp per row; the dropout mask is regenerated in the backward pass from (seed, offset), or, with a device
    source, from the same seed_ctr block and the SAME ordinal (kept in ctx: it is never drawn again)."""

    @staticmethod
    def forward(ctx, q, k, v, B, L, H, p_drop, seed, offset, seed_ctr):
        lib = _lib.load()
        _need_cuda(q, k, v)
        q, k, v = _f32(q), _f32(k), _f32(v)
        if not (q.dim() == 2 and q.shape == k.shape == v.shape and q.shape[0] == B * L and q.shape[1] % H == 0):
            raise _lib.EvaeError("causal_attn: q, k, v must be [B*L, H*dh] rows of one shape")
        dh = q.shape[1] // H
        out = torch.empty_like(q)
        lse = torch.empty((B, H, L), device=q.device)
        if seed_ctr is None:
            _lib.check(lib.evae_causal_attn_fwd(_p(q), _p(k), _p(v), B, H, L, dh, p_drop, seed, offset, _p(out), _p(lse), _stream()),
                       "evae_causal_attn_fwd")
        else:
            _lib.check(lib.evae_causal_attn_fwd_dev(_p(q), _p(k), _p(v), B, H, L, dh, p_drop, _seed_ctr_ptr(seed_ctr), offset, _p(out),
                                                    _p(lse), _stream()), "evae_causal_attn_fwd_dev")
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.cfg = (B, L, H, dh, p_drop, seed, offset, seed_ctr)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        q, k, v, out, lse = ctx.saved_tensors
        B, L, H, dh, p_drop, seed, offset, seed_ctr = ctx.cfg
        dout = _f32(dout)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
        delta = torch.empty_like(lse)                # scratch: the row pass hands delta_i to the column pass
        if seed_ctr is None:
            _lib.check(lib.evae_causal_attn_bwd(_p(q), _p(k), _p(v), _p(out), _p(lse), _p(dout), B, H, L, dh, p_drop, seed, offset,
                                                _p(delta), _p(dq), _p(dk), _p(dv), _stream()), "evae_causal_attn_bwd")
        else:
            _lib.check(lib.evae_causal_attn_bwd_dev(_p(q), _p(k), _p(v), _p(out), _p(lse), _p(dout), B, H, L, dh, p_drop,
                                                    _seed_ctr_ptr(seed_ctr), offset, _p(delta), _p(dq), _p(dk), _p(dv), _stream()),
                       "evae_causal_attn_bwd_dev")
        return dq, dk, dv, None, None, None, None, None, None, None


def causal_attn(q, k, v, B, L, H, p_drop=0.0, rng=None):
    """rng = (seed, offset) or a StepRng: an explicit mask (tests); None: the step's dropout source, else dropout_rng()"""
    return CausalAttnFn.apply(q, k, v, int(B), int(L), int(H), *_rng_args(p_drop, rng))


def _dense(t):
    """a tensor whose storage is one dense block (any permutation of a contiguous tensor: NCHW or channels-last)"""
    if t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=CL)):
        return t
    return t.contiguous()


class EluDropoutFn(torch.autograd.Function):
    """dropout(ELU(x)) in one launch, the mask over the flat storage index; the output keeps x's layout"""

    @staticmethod
    def forward(ctx, x, p_drop, seed, offset, seed_ctr):
        lib = _lib.load()
        _need_cuda(x)
        x = _dense(x.float())
        out = torch.empty_like(x)                    # (preserve_format: the same strides)
        if seed_ctr is None:
            _lib.check(lib.evae_elu_dropout_fwd(_p(x), x.numel(), p_drop, seed, offset, _p(out), _stream()), "evae_elu_dropout_fwd")
        else:
            _lib.check(lib.evae_elu_dropout_fwd_dev(_p(x), x.numel(), p_drop, _seed_ctr_ptr(seed_ctr), offset, _p(out), _stream()),
                       "evae_elu_dropout_fwd_dev")
        ctx.save_for_backward(x)
        ctx.cfg = (p_drop, seed, offset, seed_ctr)
        return out

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, = ctx.saved_tensors
        p_drop, seed, offset, seed_ctr = ctx.cfg
        dy = dy.float()
        if dy.stride() != x.stride():
            dy = torch.empty_like(x).copy_(dy)
        dx = torch.empty_like(x)
        if seed_ctr is None:
            _lib.check(lib.evae_elu_dropout_bwd(_p(dy), _p(x), x.numel(), p_drop, seed, offset, _p(dx), _stream()), "evae_elu_dropout_bwd")
        else:
            _lib.check(lib.evae_elu_dropout_bwd_dev(_p(dy), _p(x), x.numel(), p_drop, _seed_ctr_ptr(seed_ctr), offset, _p(dx), _stream()),
                       "evae_elu_dropout_bwd_dev")
        return dx, None, None, None, None


def elu_dropout(x, p_drop=0.0, rng=None):
    return EluDropoutFn.apply(x, *_rng_args(p_drop, rng))


class GluResFn(torch.autograd.Function):
    """a * sigmoid(b) + x with (a, b) the channel halves of `ab` (nn.GLU(1) + the residual of GatedResBlock): ab [N, 2C, H, W] and
    x [N, C, H, W] as channels-last tensors (or [M, 2C] and [M, C] rows); the output has x's shape, channels-last."""

    @staticmethod
    def forward(ctx, ab, x):
        lib = _lib.load()
        _need_cuda(ab, x)
        if ab.dim() == 4:
            ab, x = _cl(ab.float()), _cl(x.float())
            M, Cc = x.shape[0] * x.shape[2] * x.shape[3], x.shape[1]
        else:
            ab, x = _f32(ab), _f32(x)
            M, Cc = x.shape
        if ab.shape[1] != 2 * Cc or ab.numel() != 2 * x.numel():
            raise _lib.EvaeError("glu_res: ab must have twice the channels of x")
        out = torch.empty_like(x)
        _lib.check(lib.evae_glu_res_fwd(_p(ab), _p(x), M, Cc, _p(out), _stream()), "evae_glu_res_fwd")
        ctx.save_for_backward(ab)
        ctx.cfg = (M, Cc)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        ab, = ctx.saved_tensors
        M, Cc = ctx.cfg
        dout = _cl(dout.float()) if ab.dim() == 4 else _f32(dout)
        dab = torch.empty_like(ab)
        _lib.check(lib.evae_glu_res_bwd(_p(dout), _p(ab), M, Cc, _p(dab), _stream()), "evae_glu_res_bwd")
        return dab, dout


def glu_res(ab, x):
    return GluResFn.apply(ab, x)


# ------------------------------------------------------------------------------------------------
# cached ancestral sampler of the pixelcnn decoder: csrc/evae_pixel_decode.hip
# ------------------------------------------------------------------------------------------------
PIXEL_DECODE_MAGIC = 0x50584443
_PD_BLOCK = "pixelcnn.blocks.0."


def _pd_slots():
    """The slots of the packed buffer in the order of csrc/evae_pixel_decode.hip::PdSlot: (name, modules, kind, join).  kind 'w':
    the weight as [inputs][outputs] with the inputs ordered (filter row, filter column, channel); 'w7': the same of a causal 3 x 3
    filter, its 7 live taps only; 'b': the bias; 'buffer': a buffer as it is.  Several modules are joined along the inputs ('rows')
    or the outputs ('cols')."""
    hor, ver = "pixelcnn.horizontal.conv.conv", "pixelcnn.vertical.conv.conv"
    s = [("in_w", [hor, ver], "w", "rows"), ("hor_b", [hor], "b", "cols"), ("ver_b", [ver], "b", "cols")]
    for r in range(4):
        for c in ("conv1", "conv2"):
            m = "%sresblocks.%d.%s.conv.conv" % (_PD_BLOCK, r, c)
            s += [("res%d_%s_w" % (r, c), [m], "w7", "rows"), ("res%d_%s_b" % (r, c), [m], "b", "cols")]
    for blk in ("key_resblock", "query_resblock"):
        for c in ("conv1", "conv2"):
            m = "%s%s.%s.conv" % (_PD_BLOCK, blk, c)
            s += [("%s_%s_w" % (blk, c), [m], "w", "rows"), ("%s_%s_b" % (blk, c), [m], "b", "cols")]
    att = _PD_BLOCK + "causal_attention."
    s += [("attn_q_w", [att + "query"], "w", "rows"), ("attn_q_b", [att + "query"], "b", "cols"),
          ("attn_kv_w", [att + "key", att + "value"], "w", "cols"), ("attn_kv_b", [att + "key", att + "value"], "b", "cols")]
    o = _PD_BLOCK + "out_resblock."
    s += [("out_res_conv1_aux_w", [o + "conv1.conv", o + "aux_conv.conv"], "w", "rows"), ("out_res_conv1_b", [o + "conv1.conv"], "b", "cols"),
          ("out_res_aux_b", [o + "aux_conv.conv"], "b", "cols"), ("out_res_conv2_w", [o + "conv2.conv"], "w", "rows"),
          ("out_res_conv2_b", [o + "conv2.conv"], "b", "cols")]
    s += [("out_w", ["pixelcnn.out.1.conv"], "w", "rows"), ("out_b", ["pixelcnn.out.1.conv"], "b", "cols"),
          ("mean_w", ["p_x_mean.conv"], "w", "rows"), ("mean_b", ["p_x_mean.conv"], "b", "cols"),
          ("background", ["pixelcnn"], "buffer", "rows")]
    return s


def _pd_weight_names(shapes, module):
    """state-dict names behind the weight of `module`: weight_g and weight_v of a weight-normed one, else weight"""
    if module + ".weight_v" in shapes:
        return [module + ".weight_g", module + ".weight_v"]
    return [module + ".weight"]


def _numel(shape):
    n = 1
    for d in shape:
        n *= int(d)
    return n


def pixel_decode_images_per_block():
    """images one workgroup of the decode kernel owns (a launch of B images takes ceil(B / this) workgroups)"""
    return int(_lib.load().evae_pixel_decode_images_per_block())


def pixel_decode_layout(shapes, n_head=8):
    """The packed buffer of ops.pixel_decode for a decoder whose state dict has `shapes` {name: shape} (names 'pixelcnn.*' and
    'p_x_mean.conv.*'): {'table': the ints the kernel's entry point takes (header, then one float offset per slot), 'total': floats
    of the buffer, 'entries': one {'slot', 'offset', 'floats', 'shape', 'sources': {state-dict name: elements}} per slot}.  Every
    slot starts on a multiple of 4 floats, the biases form one block at the end (the kernel keeps it in LDS); outputs are padded to a multiple of 4 (the mean head: 1 -> 4).  Host arithmetic only."""
    entries = []
    for name, modules, kind, join in _pd_slots():
        sources, rows, cols = {}, 0, 0
        for m in modules:
            if kind == "buffer":
                names = [m + ".background"]
                shp = shapes[names[0]]
                r, c = _numel(shp[:2]), _numel(shp[2:])
            elif kind == "b":
                names = [m + ".bias"]
                r, c = 1, _numel(shapes[names[0]])
            else:
                names = _pd_weight_names(shapes, m)
                shp = shapes[names[-1]]
                c, r = int(shp[0]), _numel(shp[1:])
                if kind == "w7":
                    if tuple(shp[2:]) != (3, 3):
                        raise _lib.EvaeError("pixel_decode: %s is not a 3 x 3 filter" % m)
                    r = r // 9 * 7
            for n in names:
                sources[n] = _numel(shapes[n])
            if join == "rows" or kind == "buffer":
                if cols not in (0, c):
                    raise _lib.EvaeError("pixel_decode: the outputs of %s do not match" % (modules,))
                rows, cols = rows + r, c
            else:
                if rows not in (0, r):
                    raise _lib.EvaeError("pixel_decode: the inputs of %s do not match" % (modules,))
                rows, cols = r, cols + c
        if kind != "buffer":
            cols = (cols + 3) // 4 * 4
        entries.append(dict(slot=name, offset=None, floats=rows * cols, shape=(rows, cols), kind=kind, join=join, modules=modules,
                            sources=sources))
    off = 0
    for bias in (False, True):                  # the matrices (and the background) first, then all biases as one block
        for e in entries:
            if (e["kind"] == "b") == bias:
                e["offset"] = off
                off += (e["floats"] + 3) // 4 * 4
    attn = int(shapes[_PD_BLOCK + "causal_attention.query.weight_v"][0])
    n_res = len([k for k in shapes if k.startswith(_PD_BLOCK + "resblocks.") and k.endswith(".conv1.conv.conv.bias")])
    bg = shapes["pixelcnn.background"]
    header = [PIXEL_DECODE_MAGIC, int(shapes["pixelcnn.horizontal.conv.conv.bias"][0]),
              int(shapes[_PD_BLOCK + "resblocks.0.conv1.conv.conv.bias"][0]), int(bg[2]), int(bg[3]), n_res, int(n_head), attn // int(n_head), off]
    return dict(table=header + [e["offset"] for e in entries], total=off, entries=entries)


class PixelDecodeWeights:
    """the packed weights of one generation: `buffer` (device floats), `table` (host ints), `entries` (pixel_decode_layout)"""

    def __init__(self, buffer, table, entries):
        self.buffer, self.table, self.entries = buffer, list(table), entries


class PixelDecodeCache:
    """what ops.pixel_decode keeps between the pixels of B images: `planes` [B, evae_pixel_decode_cache_floats()] and the means
    written so far, `mean` [B, 784] (zeros where no launch has been yet)"""

    def __init__(self, B, device):
        self.planes = torch.zeros((B, int(_lib.load().evae_pixel_decode_cache_floats())), device=device)
        self.mean = torch.zeros((B, 784), device=device)

    def rows(self, n, mean=None):
        """the cache of this one's first n images as a view, its means kept in `mean` [n, 784] when that is given: a launch over
        [0, t1) reads what it wrote itself (pixel t reads positions < t), so the planes of one finished batch serve the next"""
        view = PixelDecodeCache.__new__(PixelDecodeCache)
        view.planes, view.mean = self.planes[:n], self.mean[:n] if mean is None else mean
        return view


def pixel_decode_pack(pixelsnail, mean_head):
    """PixelSNAIL module + the mean head (models/PixelCNN.py: self.pixelcnn, self.p_x_mean) -> PixelDecodeWeights, once per generation:
    the causal filters are masked as on every forward call, all weight-normed filters come from ONE weight_norm_set launch, and
    every matrix is stored transposed in the layout of pixel_decode_layout."""
    lib = _lib.load()
    with torch.no_grad():
        named = {"pixelcnn" + ("." + n if n else ""): m for n, m in pixelsnail.named_modules()}
        named["p_x_mean.conv"] = mean_head.conv
        state = {"pixelcnn." + k: v for k, v in pixelsnail.state_dict().items()}
        state.update({"p_x_mean.conv." + k: v for k, v in mean_head.conv.state_dict().items()})
        _need_cuda(*state.values())
        for m in named.values():
            if hasattr(m, "mask_weight"):
                m.mask_weight()
        normed = [n for n, m in named.items() if hasattr(m, "weight_v") and hasattr(m, "weight_g")]
        ws = weight_norm_set([(named[n].weight_v.detach(), named[n].weight_g.detach()) for n in normed])
        weight = dict(zip(normed, ws))
        n_head = named[_PD_BLOCK + "causal_attention"].n_head
        lay = pixel_decode_layout({k: tuple(v.shape) for k, v in state.items()}, n_head=n_head)
        if len(lay["table"]) != lib.evae_pixel_decode_table_len():
            raise _lib.EvaeError("pixel_decode_pack: the layout has %d table entries, the kernel takes %d"
                                 % (len(lay["table"]), lib.evae_pixel_decode_table_len()))
        buf = torch.zeros(lay["total"], device=ws[0].device)
        for s, e in enumerate(lay["entries"]):
            if e["floats"] != lib.evae_pixel_decode_slot_floats(s):
                raise _lib.EvaeError("pixel_decode_pack: %s holds %d floats, the kernel is built for %d (another decoder configuration)"
                                     % (e["slot"], e["floats"], lib.evae_pixel_decode_slot_floats(s)))
            parts = []
            for m in e["modules"]:
                if e["kind"] == "buffer":
                    parts.append(state[m + ".background"].float().reshape(e["shape"]))
                elif e["kind"] == "b":
                    parts.append(state[m + ".bias"].float().reshape(1, -1))
                else:
                    w = weight[m] if m in weight else state[m + ".weight"].float()
                    if w.dim() == 2:
                        w = w.view(w.shape[0], w.shape[1], 1, 1)
                    wt = w.permute(2, 3, 1, 0).reshape(-1, w.shape[1], w.shape[0])           # [taps][inputs][outputs]
                    if e["kind"] == "w7":
                        wt = wt[:7]
                    parts.append(wt.reshape(-1, w.shape[0]))
            mat = torch.cat(parts, 0 if (e["join"] == "rows" or e["kind"] == "buffer") else 1)
            rows, cols = e["shape"]
            out = buf[e["offset"]:e["offset"] + rows * cols].view(rows, cols)
            out[:, :mat.shape[1]] = mat
        return PixelDecodeWeights(buf, lay["table"], lay["entries"])


def pixel_decode_choose_images(B):
    """images per workgroup the library picks for a launch of B images (evae_pixel_decode_choose_images: host arithmetic)"""
    return int(_lib.load().evae_pixel_decode_choose_images(int(B)))


def pixel_decode_cache_bytes(B):
    """device bytes of the PixelDecodeCache of B images: its planes and its means"""
    return int(B) * 4 * (int(_lib.load().evae_pixel_decode_cache_floats()) + 784)


def pixel_decode(packed, latent, x, u=None, t0=0, t1=784, cache=None, start=None, images_per_block=None):
    """The eval-mode pixelcnn decoder at the pixels t0 <= t < t1 in raster order, one launch (csrc/evae_pixel_decode.hip).
    packed: pixel_decode_pack(...); latent [B, 2, 28, 28]; x [B, 784] float32; u [B, 784] uniforms or None; cache: the
    PixelDecodeCache of earlier launches over the same images (None: a fresh one, for t0 = 0).
    Returns (mean, x, cache): mean = cache.mean [B, 784], written at the pixels of every launch so far.  With u, x[:, t] is set IN
    PLACE to (u[:, t] < mean[:, t]) before pixel t + 1 is evaluated (x must then be a contiguous float32 tensor); without u the
    call is teacher-forced and x is only read.  No gradients: raises if an input requires grad while grad is enabled.
    start: with u, image b keeps x[b, :start[b]] as given and is drawn from pixel start[b] on (<= 0: all of it, >= 784: none of
    it; the means are written either way) -- an int32 or int64 device tensor [B], or an int for the whole batch; None: 0.  Without u
    it is ignored.  images_per_block: 1, 2 or 4 images to a workgroup, None: the build's default, 'auto':
    pixel_decode_choose_images(B).  The cache does not depend on it; the means do, at rounding level."""
    lib = _lib.load()
    ts = (packed.buffer, latent, x, u)
    _need_cuda(*ts)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts):
        raise _lib.EvaeError("pixel_decode is a no-grad operator: an input requires grad (call it under torch.no_grad())")
    B = x.shape[0]
    if x.dim() != 2 or x.shape[1] != 784 or tuple(latent.shape) != (B, 2, 28, 28) or (u is not None and u.shape != x.shape):
        raise _lib.EvaeError("pixel_decode: x and u must be [B, 784] and latent [B, 2, 28, 28]")
    if u is not None:
        if x.dtype != torch.float32 or not x.is_contiguous():
            raise _lib.EvaeError("pixel_decode: sampling writes x in place: it must be a contiguous float32 tensor")
        u = _f32(u)
    else:
        x = _f32(x)
    latent = _f32(latent)
    if start is not None:
        if isinstance(start, torch.Tensor):
            if start.device != x.device or tuple(start.shape) != (B,) or start.dtype not in (torch.int32, torch.int64):
                raise _lib.EvaeError("pixel_decode: start must be an int32 or int64 tensor [%d] on %s (got %s %s on %s)"
                                     % (B, x.device, start.dtype, tuple(start.shape), start.device))
            if start.dtype != torch.int32:
                start = start.clamp(-1, 784).to(torch.int32)                     # (outside [0, 784] only the side matters)
            start = start.contiguous()
        else:
            start = torch.full((B,), min(max(int(start), -1), 784), dtype=torch.int32, device=x.device)
    if images_per_block is None:
        G = int(lib.evae_pixel_decode_images_per_block())
    elif isinstance(images_per_block, str):
        if images_per_block != 'auto':
            raise _lib.EvaeError("pixel_decode: images_per_block must be 1, 2, 4, None or 'auto' (got %r)" % (images_per_block,))
        G = int(lib.evae_pixel_decode_choose_images(B))
    else:
        G = int(images_per_block)
    if cache is None:
        cache = PixelDecodeCache(B, x.device)
    if cache.mean.shape[0] != B or cache.planes.shape[0] != B:
        raise _lib.EvaeError("pixel_decode: the cache was made for %d images, not %d" % (cache.mean.shape[0], B))
    table = (C.c_int * len(packed.table))(*packed.table)
    if start is None and images_per_block is None:
        _lib.check(lib.evae_pixel_decode(_p(packed.buffer), table, len(packed.table), _p(latent), _p(x), _p(u), _p(cache.mean),
                                         _p(cache.planes), B, int(t0), int(t1), _stream()), "evae_pixel_decode")
    else:
        _lib.check(lib.evae_pixel_decode_ex(_p(packed.buffer), table, len(packed.table), _p(latent), _p(x), _p(u), _p(start),
                                            _p(cache.mean), _p(cache.planes), B, int(t0), int(t1), G, _stream()), "evae_pixel_decode_ex")
    return cache.mean, x, cache
