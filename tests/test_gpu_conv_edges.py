"""The layer-by-layer convolutions (evae.ops.Conv2dFn / ResBlockFn over csrc/evae_conv.hip and csrc/evae_conv_cl.hip) held to float64
on every branch of their backward and at the corners of the kernels' index arithmetic.  The rows, their references and the
kernel family each row declares live in tests/conv_edge_cases.py (tests/test_conv_edges_host.py checks, without a GPU, that
every row really holds the edge it is there for).

For each row, on both matrix pipes:
  * y, dx, dwh, dbh, dwg, dbg within 1e-5 of the float64 reference's largest entry (torch CPU F.conv2d + autograd on the same float32
    inputs: the bar and the reference of tests/test_gpu_conv.py);
  * where the reference is zero by construction (an input pixel no tap reaches, the filter and bias gradients of a channel that
    Hardtanh clamps everywhere) the device value is exactly 0.0 -- not small, not NaN;
  * a gradient the row does not ask for is None;
  * the C-ABI calls of the forward and the backward, recorded with step_trace.StepTrace, are exactly the entry points of the family the
    row declares, once each: a row cannot pass by quietly taking another path.
Rows whose data gradient has pixels without a tap, and rows whose gradient buffer is zero-padded, run with torch.empty / empty_like / Tensor.new_empty returning NaN-filled
tensors (the fill of tools/poison_empty.py; a layer runs on one stream, where that fill is reliable) behind fresh workspaces, so a
row the kernels forget to write shows whatever the allocator handed out before.

Run on a real MI355X:  python -m pytest tests -m gpu"""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_edge_cases as ce
from step_trace import StepTrace

pytestmark = pytest.mark.gpu

CL = torch.channels_last


def _close(name, got, ref, zero=None):
    """got within TOL of ref's largest entry; exactly 0.0 where `zero` marks a structural zero"""
    assert got is not None, name
    g = got.detach().double().cpu()
    assert g.shape == ref.shape, (name, g.shape, ref.shape)
    big = float(ref.abs().max())
    err = float((g - ref).abs().max()) / max(big, 1e-30)
    print("%-4s rel %.3g" % (name, err))
    assert err < ce.TOL, (name, err)                # (a NaN anywhere makes err NaN, and NaN < TOL is False)
    if zero is not None:
        assert bool((g[zero] == 0).all()), (name, "structural zeros", int((g[zero] != 0).sum()))


def _layout(t, how):
    """the same values as a contiguous, a channels-last, a sliced (non-contiguous) or -- never built here -- an expanded tensor"""
    t = t.cuda()
    if how == "cl":
        return t.contiguous(memory_format=CL)
    if how == "slice":
        big = torch.zeros(t.shape[:3] + (t.shape[3] + 3,), device="cuda")
        big[..., 1:-2] = t
        v = big[..., 1:-2]
        assert not v.is_contiguous() and torch.equal(v, t)
        return v
    return t.contiguous()


def _poison(monkeypatch):
    from evae import ops
    e, el, ne = torch.empty, torch.empty_like, torch.Tensor.new_empty

    def fill(t):
        if t.is_cuda and t.numel() > 0:
            if t.is_floating_point():
                t.fill_(float("nan"))
            elif t.dtype == torch.uint8:
                t.fill_(255)
        return t
    monkeypatch.setattr(torch, "empty", lambda *a, **k: fill(e(*a, **k)))
    monkeypatch.setattr(torch, "empty_like", lambda *a, **k: fill(el(*a, **k)))
    monkeypatch.setattr(torch.Tensor, "new_empty", lambda self, *a, **k: fill(ne(self, *a, **k)))
    # fresh (poisoned) named workspaces: the ones in use are retired, not freed (tests/step_trace.py::record)
    ops._ws_retired.extend(ops._ws.values())
    ops._ws.clear()


def _counts(records, names):
    n = {}
    for r in records:
        if r[0] == "call" and r[1] in names:
            n[r[1]] = n.get(r[1], 0) + 1
    return n


def _run_row(row, monkeypatch):
    from evae import ops, _lib
    N, C, H, W, Co, KH, KW, s, p = row.geom
    ref = ce.reference(row.id)
    t = ce.inputs(row)
    if row.per_pass:
        monkeypatch.setenv("EVAE_CL_IMAGES_PER_PASS", str(row.per_pass))
    x = _layout(t["x"], row.x_layout).detach().requires_grad_("x" in row.grads)
    prm = {k: None if t[k] is None else t[k].cuda().requires_grad_(ce._requires(row, k)) for k in ("wh", "bh", "wg", "bg")}
    gout = None if row.gout == "expand" else _layout(t["gout"], row.gout)
    if row.poison:
        _poison(monkeypatch)
    torch.cuda.synchronize()
    with StepTrace() as tr:
        if row.gated:
            y = ops.gated_conv2d(x, prm["wh"], prm["bh"], prm["wg"], prm["bg"], s, p)
        else:
            act = {None: (), "sigmoid": (ops.ACT_SIGMOID,), "hardtanh": (ops.ACT_HARDTANH, ce.LO, ce.HI)}[row.act]
            y = ops.conv2d(x, prm["wh"], prm["bh"], s, p, *act)

        def backward():
            if row.gout == "expand":
                y.sum().backward()              # the stride-0 expanded gradient of a sum
            else:
                y.backward(gout)
        if row.raises:
            with pytest.raises(_lib.EvaeError, match="evae_conv2d_bwd_data"):
                backward()
        else:
            backward()
    torch.cuda.synchronize()
    # the family the row declares is the one that ran
    got = _counts(tr.records, set(ce.LAUNCHES))
    assert got == ce.expected_calls(row), (row.fam, got)
    _close("y", y, ref["y"])
    grads = {"dx": x.grad, "dwh": prm["wh"].grad, "dbh": None if prm["bh"] is None else prm["bh"].grad,
             "dwg": None if prm["wg"] is None else prm["wg"].grad, "dbg": None if prm["bg"] is None else prm["bg"].grad}
    if row.raises:                      # a refused data gradient leaves nothing behind
        assert all(g is None for g in grads.values()), {k: g is not None for k, g in grads.items()}
        return
    zeros = ce.structural_zeros(row)
    for name, g in grads.items():
        if ref[name] is None:
            assert g is None, name
        else:
            _close(name, g, ref[name], zeros.get(name))


@pytest.mark.parametrize("rid", [r.id for r in ce.ACT_ROWS])
def test_activation_derivative_on_a_convolution(rid, gemm_pipe, monkeypatch):
    """evae_act_bwd feeding a convolution's gradients: written into dy, through the zero-padded copy, on the NCHW family, behind a
    patch-matrix forward; Hardtanh with whole channels exactly on LO, on HI and one float32 inside LO"""
    _run_row(ce.BY_ID[rid], monkeypatch)


@pytest.mark.parametrize("rid", [r.id for r in ce.SUBSET_ROWS])
def test_gradient_subsets_biases_and_layouts(rid, gemm_pipe, monkeypatch):
    """needs_input_grad subsets, missing biases, the upstream gradient as NCHW / channels-last / slice / expanded, the input as
    channels-last / slice -- on one layer per kernel family, gated and plain"""
    _run_row(ce.BY_ID[rid], monkeypatch)


@pytest.mark.parametrize("rid", [r.id for r in ce.GEOM_ROWS])
def test_geometry_corners(rid, gemm_pipe, monkeypatch):
    """filters smaller than the stride, strides 3 and 4, 32 channels off and on the pixel-pair form, no / too much padding, single
    output pixels and rows, rectangular filters, the patch-matrix and 64-tap thresholds, padded gradient buffers, single images"""
    _run_row(ce.BY_ID[rid], monkeypatch)


# ------------------------------------------------------------------------------------------------ the composed module path
def _module_case(kind, cin, co, stride, act_name, seed):
    from utils.nn import Conv2d, GatedConv2d
    acts = {"sigmoid": torch.nn.Sigmoid, "hardtanh": lambda: torch.nn.Hardtanh(ce.LO, ce.HI), "elu": torch.nn.ELU}
    torch.manual_seed(seed)
    m = (GatedConv2d if kind == "gated" else Conv2d)(cin, co, 3, stride, 1, activation=acts[act_name]())
    with torch.no_grad():
        for prm in m.parameters():
            prm.mul_(3.0)                  # pre-activations of order 1: sigmoid off its linear part, Hardtanh clamping on both sides
    x = torch.randn(3, cin, 8, 8)
    return m, x


@pytest.mark.parametrize("kind,cin,co,stride,act_name", [
    ("gated", 32, 8, 1, "sigmoid"), ("gated", 8, 6, 2, "sigmoid"),           # utils/nn.py GatedConv2d.forward's composed branch
    ("plain", 32, 8, 1, "sigmoid"), ("plain", 32, 8, 1, "hardtanh"), ("plain", 32, 8, 1, "elu"),
    ("plain", 8, 6, 2, "sigmoid"), ("plain", 8, 6, 2, "hardtanh"), ("plain", 64, 6, 1, "hardtanh")])
def test_modules_with_an_activation_match_their_float64_modules(kind, cin, co, stride, act_name, gemm_pipe):
    """utils.nn.GatedConv2d(..., activation=...) (act(h(x)) * sigmoid(g(x)) from two plain convolutions) and utils.nn.Conv2d with each
    activation: output, input gradient AND every parameter gradient against the same modules' torch layers in float64"""
    m, x = _module_case(kind, cin, co, stride, act_name, 17 + cin + co)
    r = copy.deepcopy(m).double()
    xr = x.double().requires_grad_(True)
    if kind == "gated":
        pre = r.h(xr)
        yr = r.activation(pre) * torch.sigmoid(r.g(xr))
    else:
        pre = r.conv(xr)
        yr = r.activation(pre)
    if act_name == "hardtanh":           # no reference pre-activation within float32 rounding of a bound (the rows above plant those)
        p64 = pre.detach()
        assert float(torch.minimum((p64 - ce.LO).abs(), (p64 - ce.HI).abs()).min()) > 1e-4
        assert bool((p64 > ce.HI).any()) and bool((p64 < ce.LO).any()) and bool(((p64 > ce.LO) & (p64 < ce.HI)).any())
    gout = torch.randn(yr.shape)
    yr.backward(gout.double())
    m = m.cuda()
    xd = x.cuda().requires_grad_(True)
    y = m(xd)
    y.backward(gout.cuda())
    _close("y", y, yr.detach())
    _close("dx", xd.grad, xr.grad)
    refp = dict(r.named_parameters())
    for name, prm in m.named_parameters():
        _close(name, prm.grad, refp[name].grad)


# ------------------------------------------------------------------------------------------------ the residual block
_RES = (2, 48, 8, 8, 3)
_RES_NAMES = ("evae_elu_fwd", "evae_conv2d_cl_fwd_res", "evae_conv2d_cl_bwd_weight", "evae_conv2d_cl_bwd_data_res")


@pytest.mark.parametrize("grads,bias", [("x", True), ("w", True), ("b", True), ("xwb", False), ("xwb", True)])
def test_residual_block_gradient_subsets(grads, bias, gemm_pipe):
    """ops.res_block (x + conv(ELU(x), w) + b) with each of x, w, b alone requiring a gradient and without a bias: values against
    float64 autograd, None where nothing was asked for, and no launch for a gradient nobody needs"""
    from evae import ops
    N, C, H, W, k = _RES
    rs = np.random.RandomState(48)
    x = torch.from_numpy((rs.standard_normal((N, C, H, W)) * 1.5).astype(np.float32))
    w = torch.from_numpy((rs.standard_normal((C, C, k, k)) / np.sqrt(C * k * k)).astype(np.float32))
    b = torch.from_numpy((rs.standard_normal(C) * 0.1).astype(np.float32)) if bias else None
    gout = torch.from_numpy(rs.standard_normal((N, C, H, W)).astype(np.float32))
    need = {"x": "x" in grads, "w": "w" in grads, "b": "b" in grads and bias}
    xr, wr = x.double().requires_grad_(need["x"]), w.double().requires_grad_(need["w"])
    br = None if b is None else b.double().requires_grad_(need["b"])
    yr = xr + F.conv2d(F.elu(xr), wr, br, 1, k // 2)
    yr.backward(gout.double())
    xd, wd = x.cuda().requires_grad_(need["x"]), w.cuda().requires_grad_(need["w"])
    bd = None if b is None else b.cuda().requires_grad_(need["b"])
    assert ops.res_block_supported(xd, wd, 1, k // 2)
    torch.cuda.synchronize()
    with StepTrace() as tr:
        y = ops.res_block(xd, wd, bd)
        y.backward(gout.cuda())
    torch.cuda.synchronize()
    want = {"evae_elu_fwd": 1, "evae_conv2d_cl_fwd_res": 1}
    if need["w"] or need["b"]:
        want["evae_conv2d_cl_bwd_weight"] = 1
    if need["x"]:
        want["evae_conv2d_cl_bwd_data_res"] = 1
    assert _counts(tr.records, set(ce.LAUNCHES)) == want
    _close("y", y, yr.detach())
    for name, dev, ref in (("dx", xd, xr), ("dw", wd, wr), ("db", bd, br)):
        if ref is None:
            continue
        if ref.grad is None:
            assert dev.grad is None, name
        else:
            _close(name, dev.grad, ref.grad)


def test_fully_conv_block_at_32_channels_runs_unfused_and_matches_float64(gemm_pipe):
    """res_block_supported refuses 32 channels (the data gradient's pixel-pair form has no residual epilogue): models.fully_conv.block
    (32, 32) runs as x + conv(ELU(x)) on the plain layer -- output, input gradient and the gradients of weight_g, weight_v and the
    bias against the float64 composition"""
    from evae import ops
    from models.fully_conv import block
    torch.manual_seed(32)
    m = block(32, 32)
    with torch.no_grad():
        m.conv1.weight_g.mul_(torch.rand_like(m.conv1.weight_g) + 0.5)
    x = torch.randn(2, 32, 8, 8) * 1.5
    gout = torch.randn(2, 32, 8, 8)
    v64, g64, b64 = (t.detach().double().requires_grad_(True) for t in (m.conv1.weight_v, m.conv1.weight_g, m.conv1.bias))
    xr = x.double().requires_grad_(True)
    yr = xr + F.conv2d(F.elu(xr), torch._weight_norm(v64, g64, 0), b64, 1, 1)
    yr.backward(gout.double())
    m = m.cuda()
    xd = x.cuda().requires_grad_(True)
    assert not ops.res_block_supported(xd, m.conv1.weight_v, 1, 1)
    torch.cuda.synchronize()
    with StepTrace() as tr:
        y = m(xd)
        y.backward(gout.cuda())
    torch.cuda.synchronize()
    assert _counts(tr.records, set(ce.LAUNCHES)) == {"evae_conv2d_cl_fwd": 1, "evae_conv2d_cl_bwd_weight": 1, "evae_conv2d_cl_bwd_data": 1}
    _close("y", y, yr.detach())
    _close("dx", xd.grad, xr.grad)
    for name, dev, ref in (("weight_v", m.conv1.weight_v, v64), ("weight_g", m.conv1.weight_g, g64), ("bias", m.conv1.bias, b64)):
        _close(name, dev.grad, ref.grad)
