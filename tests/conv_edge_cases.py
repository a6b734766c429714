"""The rows of tests/test_gpu_conv_edges.py and tests/test_conv_edges_host.py: the layer-by-layer convolutions (evae.ops.Conv2dFn over
csrc/evae_conv.hip and csrc/evae_conv_cl.hip) on every branch of Conv2dFn.backward and at the corners of the kernels' index
arithmetic, each with its float64 reference.

A row is one layer: a geometry (N, C, H, W, Co, KH, KW, stride, pad), gated or plain, an optional activation, which inputs require a
gradient, which biases exist, how the upstream gradient and the input are laid out -- and the kernel family it DECLARES for its
forward, weight gradient and data gradient ("cl" the channels-last GEMM instances, "patch" their patch-matrix form for thin layers,
"nchw" the NCHW implicit-GEMM kernels, "none" no launch).  family_rule() restates the library's selection (evae_conv2d_cl_supported,
csrc/evae_conv_cl.hip, and Conv2dFn.backward's cl_w / cl_d) in Python; the host test holds every declaration to it, the GPU test
holds the recorded C-ABI calls to the declaration.

The reference is torch CPU float64 F.conv2d (+ sigmoid gate | sigmoid | F.hardtanh) and its autograd on the float32 inputs, as
tests/test_gpu_conv.py::test_conv2d_fwd_bwd_matches_torch builds it.  structural_zeros() names the entries whose reference value
is zero by construction, not by rounding: input pixels no tap reaches, and the filter / bias gradients of channels Hardtanh clamps
everywhere."""
import collections
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

LO, HI = -4.5, 0.0                       # the Hardtanh of the reference's log-variance heads
TOL = 1e-5                               # of the reference tensor's largest entry: the bar of tests/test_gpu_conv.py
f32 = np.float32
LO_IN = np.nextafter(f32(LO), f32(np.inf))         # the float32 just inside the lower bound

Row = collections.namedtuple("Row", "id geom gated act fam grads bh bg gout x_layout poison per_pass raises small_filter")


def R(id, geom, fam, gated=False, act=None, grads="xwb", bh=True, bg=True, gout="nchw", x_layout="nchw", poison=False,
      per_pass=None, raises=False, small_filter=False):
    """grads: which of x, the filters (w) and the biases (b) require a gradient; bg is ignored on a plain layer"""
    return Row(id, tuple(geom), bool(gated), act, tuple(fam.split("/")), grads, bh, bg and gated, gout, x_layout, poison, per_pass,
               raises, small_filter)


# ------------------------------------------------------------------------------------------------ A. the activation's derivative
# plain layers with sigmoid / Hardtanh(LO, HI): evae_act_bwd written straight into dy (ldy == ctot), through the zero-padded copy
# (ctot = 1 | 6 -> ldy = 32; weight gradient on the NCHW kernels, data gradient channels-last: the mean head of convHVAE_2level),
# on the NCHW family, and behind a patch-matrix forward.  Hardtanh rows plant channels 0 / 1 / 2 on LO, HI and just inside LO.
ACT_ROWS = [
    R("act-cl-sigmoid", (3, 32, 8, 8, 8, 3, 3, 1, 1), "cl/cl/cl", act="sigmoid"),
    R("act-cl-sigmoid-nodx", (3, 32, 8, 8, 8, 3, 3, 1, 1), "cl/cl/none", act="sigmoid", grads="wb"),
    R("act-cl-hardtanh", (3, 32, 8, 8, 8, 3, 3, 1, 1), "cl/cl/cl", act="hardtanh"),
    R("act-cl-hardtanh-nodx", (3, 32, 8, 8, 8, 3, 3, 1, 1), "cl/cl/none", act="hardtanh", grads="wb"),
    R("act-mixed-sigmoid", (3, 64, 7, 7, 1, 3, 3, 1, 1), "cl/nchw/cl", act="sigmoid", poison=True),      # (the padding of dy must be
    R("act-mixed-hardtanh", (3, 64, 7, 7, 6, 3, 3, 1, 1), "cl/nchw/cl", act="hardtanh", poison=True),    #  zero, not what was there)
    R("act-nchw-sigmoid", (4, 8, 10, 10, 5, 3, 3, 1, 1), "nchw/nchw/nchw", act="sigmoid"),
    R("act-nchw-hardtanh", (4, 8, 10, 10, 5, 3, 3, 1, 1), "nchw/nchw/nchw", act="hardtanh"),
    R("act-patch-sigmoid", (3, 1, 9, 11, 8, 3, 3, 2, 1), "patch/patch/nchw", act="sigmoid"),
    R("act-patch-hardtanh", (3, 1, 9, 11, 8, 3, 3, 2, 1), "patch/patch/nchw", act="hardtanh"),
]


# ------------------------------------------------------------------------------------------------ B. gradient subsets, biases, layouts
# one base layer per family, gated and plain; every variant of needs_input_grad, of the biases and of the two layouts
_BASES = (("cl", (3, 32, 8, 8, 8, 3, 3, 2, 1), "cl/cl/cl"),
          ("nchw", (4, 8, 10, 10, 6, 3, 3, 2, 1), "nchw/nchw/nchw"),
          ("patch", (3, 1, 9, 11, 8, 3, 3, 2, 1), "patch/patch/nchw"))


def _subset_rows():
    rows = []
    for name, geom, fam in _BASES:
        nodx = fam.rsplit("/", 1)[0] + "/none"
        for gated in (False, True):
            tag = "sub-%s-%s-" % (name, "gated" if gated else "plain")
            kw = dict(gated=gated)
            rows += [R(tag + "x-frozen", geom, nodx, grads="wb", **kw),          # dx is None, no data-gradient launch
                     R(tag + "only-x", geom, fam, grads="x", **kw),              # (Conv2dFn still launches the weight gradient)
                     R(tag + "w-frozen", geom, fam, grads="xb", **kw),
                     R(tag + "no-bh", geom, fam, bh=False, **kw)]
            if gated:
                rows += [R(tag + "no-biases", geom, fam, bh=False, bg=False, **kw),
                         R(tag + "no-bg", geom, fam, bg=False, **kw)]
            rows += [R(tag + "gout-" + g, geom, fam, gout=g, **kw) for g in ("nchw", "cl", "slice", "expand")]
            rows += [R(tag + "x-" + l, geom, fam, x_layout=l, **kw) for l in ("cl", "slice")]
    return rows


SUBSET_ROWS = _subset_rows()


# ------------------------------------------------------------------------------------------------ C. geometry
# (name, geometry, family of the plain layer, family of the gated layer (None: as plain), which of the two run, flags)
_P, _G, _PG = "p", "g", "pg"
_GEOMS = [
    # a filter smaller than the stride: whole rows / columns of dx that no tap reaches.  32 channels, even width: the pixel-pair
    # form (memset row by row); 64 and 20 channels: the general form (memset of all of dx); 16 x 2 x 2 = 64 and 8 x 1 x 1 columns
    # are patch matrices, whose data gradient is the NCHW kernel's (classes without a tap: a zero-length contraction); 66
    # channels: NCHW throughout
    ("small-pair", (2, 32, 8, 8, 8, 1, 1, 2, 0), "cl/cl/cl", None, _PG, dict(poison=True, small_filter=True)),
    ("small-general", (2, 64, 8, 8, 8, 1, 1, 2, 0), "cl/cl/cl", None, _PG, dict(poison=True, small_filter=True)),
    ("small-pair-passes", (5, 32, 8, 8, 8, 1, 1, 2, 0), "cl/cl/cl", None, _PG, dict(poison=True, small_filter=True, per_pass=2)),
    ("small-general-passes", (5, 64, 8, 8, 8, 1, 1, 2, 0), "cl/cl/cl", None, _PG, dict(poison=True, small_filter=True, per_pass=2)),
    ("small-2x2-s3-c16", (2, 16, 9, 9, 4, 2, 2, 3, 0), "patch/patch/nchw", None, _PG, dict(poison=True, small_filter=True)),
    ("small-2x2-s3-c20", (2, 20, 9, 9, 4, 2, 2, 3, 0), "cl/cl/cl", None, _PG, dict(poison=True, small_filter=True)),
    ("small-1x1-s2-c8", (2, 8, 9, 9, 4, 1, 1, 2, 0), "patch/patch/nchw", None, _PG, dict(poison=True, small_filter=True)),
    ("small-1x1-s2-c66", (2, 66, 9, 9, 4, 1, 1, 2, 0), "nchw/nchw/nchw", None, _PG, dict(poison=True, small_filter=True)),
    # strides 3 and 4 (stride 4 with a 3 x 3 filter leaves rows 2 and 6 of 9 without a tap)
    ("stride3-cl", (2, 16, 10, 10, 8, 3, 3, 3, 1), "cl/cl/cl", None, _PG, {}),
    ("stride4-cl", (2, 16, 9, 9, 4, 3, 3, 4, 1), "cl/cl/cl", None, _PG, dict(poison=True)),
    ("stride3-nchw", (2, 8, 10, 10, 4, 3, 3, 3, 1), "nchw/nchw/nchw", None, _PG, {}),
    ("stride4-nchw-refused", (2, 8, 9, 9, 4, 3, 3, 4, 1), "nchw/nchw/nchw", None, _PG, dict(raises=True)),
    ("stride4-nchw-nodx", (2, 8, 9, 9, 4, 3, 3, 4, 1), "nchw/nchw/none", None, _PG, dict(grads="wb")),
    # 32 channels: odd width (no pixel pairs: the general path at C = 32), the pair form at 5 x 5 stride 2 and 7 x 7 stride 1, and
    # 8 x 8 where KH (KW + 1) = 72 > 64 sends it back to the general path
    ("c32-oddw-s1", (3, 32, 9, 7, 8, 3, 3, 1, 1), "cl/cl/cl", None, _PG, {}),
    ("c32-oddw-s2", (3, 32, 9, 7, 8, 3, 3, 2, 1), "cl/cl/cl", None, _PG, {}),
    ("c32-pair-5x5-s2", (2, 32, 10, 12, 8, 5, 5, 2, 2), "cl/cl/cl", None, _PG, {}),
    ("c32-pair-7x7", (2, 32, 8, 8, 4, 7, 7, 1, 3), "cl/cl/cl", None, _PG, {}),
    ("c32-8x8-general", (2, 32, 10, 10, 4, 8, 8, 1, 3), "cl/cl/cl", None, _PG, {}),
    # padding: none (every PixelSNAIL causal convolution behind its ZeroPad2d), more than (k - 1) / 2, a single output pixel, one row
    ("pad0-c64", (2, 64, 6, 6, 128, 3, 3, 1, 0), "cl/cl/cl", None, _PG, {}),
    ("overpad", (2, 16, 6, 6, 8, 3, 3, 1, 2), "cl/cl/cl", None, _PG, {}),
    ("one-output-pixel", (2, 16, 5, 5, 4, 5, 5, 1, 0), "cl/cl/cl", None, _PG, {}),
    ("one-row-c16", (2, 16, 1, 9, 4, 1, 3, 2, 0), "patch/patch/nchw", None, _PG, {}),          # 16 x 1 x 3 = 48 columns: a patch matrix
    ("one-row-c24", (2, 24, 1, 9, 4, 1, 3, 2, 0), "cl/cl/cl", None, _PG, {}),
    # rectangular filters (PixelSNAIL's `horizontal` 1 x 3 and `vertical` 2 x 1 on 3 channels)
    ("rect-1x3-c3", (2, 3, 9, 10, 64, 1, 3, 1, 0), "patch/patch/nchw", None, _PG, {}),
    ("rect-2x1-c3", (2, 3, 10, 9, 64, 2, 1, 1, 0), "patch/patch/nchw", None, _PG, {}),
    ("rect-2x3-c16", (2, 16, 7, 9, 8, 2, 3, 1, 0), "cl/cl/cl", None, _PG, {}),
    ("rect-3x2-s2-c32", (2, 32, 6, 8, 8, 3, 2, 2, 0), "cl/cl/cl", None, _PG, dict(poison=True)),   # input row 5 of 6 is never read
    ("rect-2x3-c8", (2, 8, 7, 9, 4, 2, 3, 1, 0), "patch/patch/nchw", None, _PG, {}),             # 8 x 2 x 3 = 48 columns
    ("rect-2x3-c12", (2, 12, 7, 9, 4, 2, 3, 1, 0), "nchw/nchw/nchw", None, _PG, {}),
    # odd, non-square images at stride 2 on the general path
    ("odd-image-s2", (2, 48, 9, 11, 8, 3, 3, 2, 1), "cl/cl/cl", None, _PG, {}),
    # thresholds: C KH KW = 64 is a patch matrix, 100 is not; 64 taps are channels-last, 81 are not
    ("patch-64-c4", (2, 4, 8, 8, 8, 4, 4, 1, 1), "patch/patch/nchw", None, _PG, {}),
    ("patch-64-c1", (2, 1, 12, 12, 8, 8, 8, 1, 3), "patch/patch/nchw", None, _PG, {}),
    ("no-patch-100", (2, 4, 9, 9, 8, 5, 5, 1, 2), "nchw/nchw/nchw", None, _PG, {}),
    ("taps-64", (2, 16, 12, 12, 4, 8, 8, 1, 3), "cl/cl/cl", None, _PG, {}),
    ("taps-81", (2, 16, 12, 12, 4, 9, 9, 1, 4), "nchw/nchw/nchw", None, _PG, {}),
    # the gradient buffer's stride: 33 and 34 channels round up to 64 (weight gradient on the NCHW kernels), 4 stays 4
    ("ldy-33", (2, 16, 6, 6, 33, 3, 3, 1, 1), "cl/nchw/cl", None, _P, dict(poison=True)),
    ("ldy-34", (2, 16, 6, 6, 17, 3, 3, 1, 1), None, "cl/nchw/cl", _G, dict(poison=True)),
    ("ldy-4", (2, 16, 6, 6, 4, 3, 3, 1, 1), "cl/cl/cl", None, _PG, {}),
    # one image
    ("n1-cl", (1, 32, 8, 8, 8, 3, 3, 2, 1), "cl/cl/cl", None, _PG, {}),
    ("n1-nchw", (1, 8, 10, 10, 6, 3, 3, 2, 1), "nchw/nchw/nchw", None, _PG, {}),
    ("n1-patch", (1, 1, 9, 11, 8, 3, 3, 2, 1), "patch/patch/nchw", None, _PG, {}),
]


def _geom_rows():
    rows = []
    for name, geom, fam_p, fam_g, which, kw in _GEOMS:
        if "p" in which:
            rows.append(R("geo-%s-plain" % name, geom, fam_p, **kw))
        if "g" in which:
            rows.append(R("geo-%s-gated" % name, geom, fam_g or fam_p, gated=True, **kw))
    return rows


GEOM_ROWS = _geom_rows()
ALL_ROWS = ACT_ROWS + SUBSET_ROWS + GEOM_ROWS
BY_ID = {r.id: r for r in ALL_ROWS}


# ------------------------------------------------------------------------------------------------ the library's selection, restated
def out_dims(geom):
    N, C, H, W, Co, KH, KW, s, p = geom
    return (H + 2 * p - KH) // s + 1, (W + 2 * p - KW) // s + 1


def family_rule(geom, gated, x_grad):
    """(forward, weight gradient, data gradient) as evae_conv2d_cl_supported (csrc/evae_conv_cl.hip) and Conv2dFn.backward pick
    them: patch mode <=> C % 32 != 0 and C KH KW <= 64 (forward yes, weight gradient iff ctot % 4 == 0, data gradient never);
    otherwise forward iff C % 4 == 0 and C >= 16, data gradient iff C % 4 == 0, weight gradient iff C % 4 == 0 and ctot % 4 == 0;
    more than 64 taps are never channels-last; a gradient is channels-last only if the forward was."""
    N, C, H, W, Co, KH, KW, s, p = geom
    ctot = Co * (2 if gated else 1)
    if KH * KW > 64:
        fam = ("nchw", "nchw", "nchw")
    elif C % 32 != 0 and C * KH * KW <= 64:
        fam = ("patch", "patch" if ctot % 4 == 0 else "nchw", "nchw")
    elif C % 4 == 0 and C >= 16:
        fam = ("cl", "cl" if ctot % 4 == 0 else "nchw", "cl")
    else:
        fam = ("nchw", "nchw", "nchw")
    return fam if x_grad else fam[:2] + ("none",)


def dy_stride(ctot):
    """evae_conv2d_cl_dy_stride: channels per pixel of the merged gradient buffer"""
    return ctot if ctot % 4 == 0 else (ctot + 31) // 32 * 32


_ENTRY = {("fwd", "cl"): "evae_conv2d_cl_fwd", ("fwd", "patch"): "evae_conv2d_cl_fwd", ("fwd", "nchw"): "evae_conv2d_fwd",
          ("w", "cl"): "evae_conv2d_cl_bwd_weight", ("w", "patch"): "evae_conv2d_cl_bwd_weight", ("w", "nchw"): "evae_conv2d_bwd_weight",
          ("d", "cl"): "evae_conv2d_cl_bwd_data", ("d", "nchw"): "evae_conv2d_bwd_data"}
# every launch entry point a layer of Conv2dFn / ResBlockFn can issue: the trace of a row holds exactly its expected ones, once each
LAUNCHES = sorted(set(_ENTRY.values()) | {"evae_act_bwd", "evae_gated_dense_bwd_input", "evae_elu_fwd", "evae_conv2d_cl_fwd_res",
                                          "evae_conv2d_cl_bwd_data_res"})


def expected_calls(row):
    """entry point -> number of calls of one forward and one backward of the row"""
    names = [_ENTRY["fwd", row.fam[0]], _ENTRY["w", row.fam[1]]]
    if row.fam[2] != "none":
        names.append(_ENTRY["d", row.fam[2]])
    if row.act:
        names.append("evae_act_bwd")
    if row.gated:
        names.append("evae_gated_dense_bwd_input")
    return {n: 1 for n in names}


# ------------------------------------------------------------------------------------------------ inputs and the float64 reference
def inputs(row):
    """float32 CPU tensors x, wh, bh, wg, bg, gout of a row (seeded by its id).  Hardtanh rows: channels 0 / 1 / 2 have all-zero
    filters and the biases LO, HI and the float32 just above LO, so their pre-activations are those values exactly, in any
    arithmetic.  gout is all ones for the row whose upstream gradient is y.sum()'s."""
    N, C, H, W, Co, KH, KW, s, p = row.geom
    rs = np.random.RandomState(zlib.crc32(row.id.encode()) & 0x7FFFFFFF)
    sc = 1.0 / np.sqrt(C * KH * KW)
    t = {"x": rs.standard_normal((N, C, H, W)).astype(f32),
         "wh": (rs.standard_normal((Co, C, KH, KW)) * sc).astype(f32), "bh": (rs.standard_normal(Co) * 0.1).astype(f32),
         "wg": (rs.standard_normal((Co, C, KH, KW)) * sc).astype(f32), "bg": (rs.standard_normal(Co) * 0.1).astype(f32)}
    OH, OW = out_dims(row.geom)
    t["gout"] = np.ones((N, Co, OH, OW), f32) if row.gout == "expand" else rs.standard_normal((N, Co, OH, OW)).astype(f32)
    if row.act == "hardtanh":
        assert Co >= 4 and row.bh and not row.gated
        t["wh"][:3] = 0.0
        t["bh"][:3] = (f32(LO), f32(HI), LO_IN)
    if not row.gated:
        t["wg"] = t["bg"] = None
    if not row.bh:
        t["bh"] = None
    if not row.bg:
        t["bg"] = None
    return {k: None if v is None else torch.from_numpy(v) for k, v in t.items()}


def _requires(row, name):
    return {"x": "x", "wh": "w", "wg": "w", "bh": "b", "bg": "b"}[name] in row.grads


@functools.lru_cache(maxsize=None)
def reference(row_id):
    """float64 tensors y, pre (the plain layer's pre-activation) and dx, dwh, dbh, dwg, dbg (None where the row asks for no gradient
    or passes no such tensor).  Computed once per row; callers must not modify it."""
    row = BY_ID[row_id]
    N, C, H, W, Co, KH, KW, s, p = row.geom
    t = inputs(row)
    leaf = {k: None if t[k] is None else t[k].double().requires_grad_(_requires(row, k)) for k in ("x", "wh", "bh", "wg", "bg")}
    pre = F.conv2d(leaf["x"], leaf["wh"], leaf["bh"], s, p)
    if row.gated:
        y = pre * torch.sigmoid(F.conv2d(leaf["x"], leaf["wg"], leaf["bg"], s, p))
    elif row.act == "sigmoid":
        y = torch.sigmoid(pre)
    elif row.act == "hardtanh":
        y = F.hardtanh(pre, LO, HI)
    else:
        y = pre
    y.backward(t["gout"].double())
    out = {"y": y.detach(), "pre": pre.detach()}
    for k, g in (("x", "dx"), ("wh", "dwh"), ("bh", "dbh"), ("wg", "dwg"), ("bg", "dbg")):
        out[g] = None if leaf[k] is None else leaf[k].grad
    return out


def _reached(L, K, s, p, OL):
    """which of L input positions at least one tap of one of OL output positions reads"""
    return np.array([any((i + p - k) >= 0 and (i + p - k) % s == 0 and (i + p - k) // s < OL for k in range(K)) for i in range(L)])


def structural_zeros(row):
    """name -> boolean mask (shape of the reference tensor) of the entries that are zero by construction"""
    N, C, H, W, Co, KH, KW, s, p = row.geom
    OH, OW = out_dims(row.geom)
    z = {}
    hit = _reached(H, KH, s, p, OH)[:, None] & _reached(W, KW, s, p, OW)[None, :]
    if not hit.all():
        z["dx"] = torch.from_numpy(np.broadcast_to(~hit, (N, C, H, W)).copy())
    if row.act == "hardtanh":                     # channels 0 (on LO) and 1 (on HI) pass no gradient anywhere
        m = torch.zeros((Co, C, KH, KW), dtype=torch.bool)
        m[:2] = True
        z["dwh"] = m
        z["dbh"] = torch.tensor([True, True] + [False] * (Co - 2))
    return z
