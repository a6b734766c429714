"""Layer modules with the reference's names, constructor arguments and state_dict keys
(reference utils/nn.py:12-114), computing through the HIP dense kernels (evae.ops).

GatedDense / NonLinear / Linear run on the fp32-MFMA GEMM of libevae_hip.so with the bias, activation and
gate fused into the epilogue.  GatedConv2d / Conv2d / HipConv2d run as channels-last convolutions on the same GEMM kernel
(csrc/evae_conv_cl.hip: a K-slab is 32 channels of one filter tap, so the im2col gather is the dense tile with a per-slab
offset; one pass over x computes both filter banks of a gated layer and applies the gate in the epilogue; any channel
count >= 16 that is a multiple of 4) -- thin first layers through a patch matrix, data gradients into 1/3-channel inputs
through the NCHW implicit-GEMM kernels of csrc/evae_conv.hip.

The PixelSNAIL layers of the reference (utils/nn.py:148-562: wn_linear ... PixelSNAIL) are at the end of this file, on the
kernels of csrc/evae_attn.hip (fused causal attention, ELU -> dropout, GLU residual) and the ones above."""
from functools import lru_cache, partial

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from evae import ops


def he_init(m):
    """N(0, sqrt(2 / fan_in)) on m.weight  (reference utils/nn.py:12-14)."""
    m.weight.data.normal_(0, float(np.sqrt(2.0 / m.in_features)))


def xavier_init(m):
    m.weight.data.normal_(0, float(np.sqrt(2.0 / (m.in_features + m.out_features))))


def normal_init(m, mean=0., std=0.01):
    m.weight.data.normal_(mean, std)


def _act_code(activation):
    """Map an nn activation module onto an epilogue code; None if it has to run as a separate op."""
    if activation is None:
        return ops.ACT_NONE, 0.0, 0.0
    if isinstance(activation, nn.Sigmoid):
        return ops.ACT_SIGMOID, 0.0, 0.0
    if isinstance(activation, nn.Hardtanh):
        return ops.ACT_HARDTANH, float(activation.min_val), float(activation.max_val)
    return None


def dense(x, linear_module, activation=None, rows=None):
    """activation(linear_module(x)) through evae_linear_fwd; x may be row-gathered by `rows`."""
    x2 = x if x.dim() == 2 else x.reshape(-1, x.shape[-1])
    code = _act_code(activation)
    if code is None:
        y = ops.linear(x2, linear_module.weight, linear_module.bias, rows=rows)
        y = activation(y)
    else:
        y = ops.linear(x2, linear_module.weight, linear_module.bias, code[0], code[1], code[2], rows=rows)
    if rows is None and x.dim() != 2:
        y = y.reshape(*x.shape[:-1], y.shape[-1])
    return y


class HipLinear(nn.Linear):
    """torch.nn.Linear parameters (same state_dict keys), forward on the HIP GEMM."""

    def forward(self, x, rows=None):
        return dense(x, self, None, rows=rows)


class NonLinear(nn.Module):
    def __init__(self, input_size, output_size, bias=True, activation=None):
        super().__init__()
        self.activation = activation
        self.linear = nn.Linear(int(input_size), int(output_size), bias=bias)

    def forward(self, x, rows=None):
        return dense(x, self.linear, self.activation, rows=rows)


class GatedDense(nn.Module):
    """h(x) * sigmoid(g(x)); with no_attention=True the reference degenerates to ReLU(h(x)) and builds
    no gate (utils/nn.py:44-69)."""

    def __init__(self, input_size, output_size, activation=None, no_attention=False):
        super().__init__()
        self.activation = activation
        self.no_attention = no_attention
        self.sigmoid = nn.Sigmoid()
        self.h = nn.Linear(input_size, output_size)
        if no_attention is False:
            self.g = nn.Linear(input_size, output_size)
        else:
            self.activation = nn.ReLU()

    def forward(self, x, rows=None, x_scale=None):
        if self.no_attention is False and self.activation is None:
            x2 = x if x.dim() == 2 else x.reshape(-1, x.shape[-1])
            leaf = ops.active_leaf_stream()
            if leaf is not None and rows is None and x_scale is None and torch.is_grad_enabled() and self.h.weight.requires_grad:
                return ops.gated_dense_split(x2, self.h.weight, self.h.bias, self.g.weight, self.g.bias, leaf)
            # x_scale: x is the uint8 image store (models/BaseModel.py::resident_u8), pixel = byte * x_scale
            return ops.gated_dense(x2, self.h.weight, self.h.bias, self.g.weight, self.g.bias, rows=rows, x_scale=x_scale)
        h = dense(x, self.h, None, rows=rows)
        if self.activation is not None:
            h = self.activation(h)
        if self.no_attention is False:
            return h * dense(x, self.g, self.sigmoid, rows=rows)
        return h


class GatedConv2d(nn.Module):
    """act(h(x)) * sigmoid(g(x)) with two convolutions sharing the input (utils/nn.py:72-97).
    Like the reference, no_attention=True cannot run (no `g` is built there either)."""

    def __init__(self, input_channels, output_channels, kernel_size, stride, padding, dilation=1,
                 activation=None, no_attention=False):
        super().__init__()
        self.no_attention = no_attention
        self.activation = activation
        self.sigmoid = nn.Sigmoid()
        self.h = nn.Conv2d(input_channels, output_channels, kernel_size, stride, padding, dilation)
        if no_attention is False:
            self.g = nn.Conv2d(input_channels, output_channels, kernel_size, stride, padding, dilation)
        else:
            self.activation = nn.ELU()

    def forward(self, x):
        assert self.h.dilation == (1, 1) and self.h.groups == 1
        if self.activation is None:
            # both filter banks in one implicit GEMM over x, gate applied in its epilogue
            return ops.gated_conv2d(x, self.h.weight, self.h.bias, self.g.weight, self.g.bias,
                                    self.h.stride, self.h.padding)
        h = self.activation(ops.conv2d(x, self.h.weight, self.h.bias, self.h.stride, self.h.padding))
        return h * ops.conv2d(x, self.g.weight, self.g.bias, self.g.stride, self.g.padding, ops.ACT_SIGMOID)


class GatedConvStack(nn.Sequential):
    """nn.Sequential of GatedConv2d layers (same children, same state_dict keys) whose leading layers run as ONE operator over
    pre-split pixel images when the batch is large (evae.ops.GatedConvStackFn: the exemplar rows of a training step, cache_z);
    small batches and anything the image kernels do not take go layer by layer as before."""

    def forward(self, x):
        mods = list(self)
        if (ops.CONV_STACK_ON and x.is_cuda and x.dim() == 4 and x.shape[0] >= ops.CONV_STACK_MIN_IMAGES and not x.requires_grad
                and all(isinstance(m, GatedConv2d) and m.no_attention is False and m.activation is None and m.h.dilation == (1, 1)
                        and m.h.groups == 1 for m in mods)):
            spec = [(m.h.weight, ops._int1(m.h.stride), ops._int1(m.h.padding)) for m in mods]
            b = ops.conv_stack_depth(tuple(x.shape), spec)
            if b:
                h = ops.gated_conv_stack(x, [(m.h.weight, m.h.bias, m.g.weight, m.g.bias, m.h.stride, m.h.padding) for m in mods[:b]])
                for m in mods[b:]:
                    h = m(h)
                return h
        return super().forward(x)


class Conv2d(nn.Module):
    def __init__(self, input_channels, output_channels, kernel_size, stride, padding, dilation=1,
                 activation=None, bias=True):
        super().__init__()
        self.activation = activation
        self.conv = nn.Conv2d(input_channels, output_channels, kernel_size, stride, padding, dilation, bias=bias)

    def forward(self, x):
        c = self.conv
        assert c.dilation == (1, 1) and c.groups == 1
        code = _act_code(self.activation)
        if code is None:
            return self.activation(ops.conv2d(x, c.weight, c.bias, c.stride, c.padding))
        return ops.conv2d(x, c.weight, c.bias, c.stride, c.padding, code[0], code[1], code[2])


class HipConv2d(nn.Conv2d):
    """torch.nn.Conv2d parameters / state_dict keys (weight-norm hooks included), forward on the HIP kernels."""

    def forward(self, x):
        assert self.dilation == (1, 1) and self.groups == 1 and self.padding_mode == 'zeros'
        return ops.conv2d(x, self.weight, self.bias, self.stride, self.padding)


# ----------------------------------------------------------------------------------------------------------------------
# PixelSNAIL (reference utils/nn.py:148-562, itself a port of github.com/neocxi/pixelsnail-public): names, constructor
# signatures and state_dict keys of the reference.  Activations are logical NCHW tensors in channels-last storage, so
# that a 1x1 convolution is evae.ops.linear over the pixel rows (input widths 66 / 130 / 132 are no multiple of 4: the
# channels-last convolution family does not take them), k x k convolutions are an F.pad in front of a pad-0
# evae.ops.conv2d, and ELU -> dropout, the GLU residual and the attention are the kernels of csrc/evae_attn.hip.
# Weight-normed modules keep torch's weight_g / weight_v parameters; the weights themselves come from
# evae.ops.weight_norm_set -- one launch for a whole PixelSNAIL (two for its gradients), or one per layer when a layer
# is used on its own.
# ----------------------------------------------------------------------------------------------------------------------
_WN_SCOPE = [None]          # id(module) -> weight of this pass (set by PixelSNAIL.forward)


def _is_weight_normed(m):
    return hasattr(m, 'weight_v') and hasattr(m, 'weight_g')


class _wn_scope:
    """with _wn_scope(root): every weight-normed module under `root` gets its weight from ONE weight_norm_set; the causal
    convolutions' weight_v is masked first (CausalConv2d.forward).  Nested scopes are the outer one."""

    def __init__(self, root):
        self.root, self.own = root, False

    def __enter__(self):
        if _WN_SCOPE[0] is None:
            mods = []
            for m in self.root.modules():
                if isinstance(m, CausalConv2d):
                    m.mask_weight()
                if _is_weight_normed(m):
                    mods.append(m)
            ws = ops.weight_norm_set([(m.weight_v, m.weight_g) for m in mods]) if mods else []
            _WN_SCOPE[0] = {id(m): w for m, w in zip(mods, ws)}
            self.own = True
        return self

    def __exit__(self, *exc):
        if self.own:
            _WN_SCOPE[0] = None
        return False


def _wn_weight(m):
    """weight = g * v / ||v|| of a weight-normed module (differentiable through to weight_g and weight_v)"""
    w = _WN_SCOPE[0].get(id(m)) if _WN_SCOPE[0] is not None else None
    if w is None:
        w = ops.weight_norm_set([(m.weight_v, m.weight_g)])[0]
    return w


def _pixel_rows(x):
    """[N, C, H, W] -> the pixel rows [N*H*W, C] (a view of channels-last storage, one copy of anything else)"""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def _from_pixel_rows(rows, n, h, w):
    """[N*H*W, C] rows -> the logical [N, C, H, W] tensor over the same (channels-last) storage"""
    return rows.view(n, h, w, rows.shape[1]).permute(0, 3, 1, 2)


class _WNLinear(HipLinear):
    def forward(self, x, rows=None):
        x2 = x if x.dim() == 2 else x.reshape(-1, x.shape[-1])
        y = ops.linear(x2, _wn_weight(self), self.bias, rows=rows)
        return y if x.dim() == 2 else y.reshape(*x.shape[:-1], y.shape[-1])


def wn_linear(in_dim, out_dim):
    return nn.utils.weight_norm(_WNLinear(in_dim, out_dim))


class WNConv2d(nn.Module):
    def __init__(self, in_channel, out_channel, kernel_size, stride=1, padding=0, bias=True, activation=None):
        super().__init__()
        self.conv = nn.utils.weight_norm(HipConv2d(in_channel, out_channel, kernel_size, stride=stride, padding=padding, bias=bias))
        self.out_channel = out_channel
        if isinstance(kernel_size, int):
            kernel_size = [kernel_size, kernel_size]
        self.kernel_size = kernel_size
        self.activation = activation

    def forward(self, input):
        c = self.conv
        w = _wn_weight(c)
        if tuple(c.kernel_size) == (1, 1) and ops._int1(c.stride) == 1 and ops._int1(c.padding) == 0:
            n, _, h, wd = input.shape
            out = _from_pixel_rows(ops.linear(_pixel_rows(input), w.view(w.shape[0], w.shape[1]), c.bias), n, h, wd)
        else:
            out = ops.conv2d(input, w, c.bias, c.stride, c.padding)
        if self.activation is not None:
            out = self.activation(out)
        return out


def shift_down(input, size=1):
    return F.pad(input, [0, 0, size, 0])[:, :, : input.shape[2], :]


def shift_right(input, size=1):
    return F.pad(input, [size, 0, 0, 0])[:, :, :, : input.shape[3]]


class CausalConv2d(nn.Module):
    def __init__(self, in_channel, out_channel, kernel_size, stride=1, padding='downright', activation=None):
        super().__init__()
        if isinstance(kernel_size, int):
            kernel_size = [kernel_size] * 2
        self.kernel_size = kernel_size
        if padding == 'downright':
            pad = [kernel_size[1] - 1, 0, kernel_size[0] - 1, 0]
        elif padding == 'down' or padding == 'causal':
            pad = kernel_size[1] // 2
            pad = [pad, pad, kernel_size[0] - 1, 0]
        self.causal = 0
        if padding == 'causal':
            self.causal = kernel_size[1] // 2
        self.pad = nn.ZeroPad2d(pad)
        self.conv = WNConv2d(in_channel, out_channel, kernel_size, stride=stride, padding=0, activation=activation)

    def mask_weight(self):
        """the reference zeroes the taps right of the centre in the last filter row IN PLACE on every call: checkpoints
        carry the zeros (utils/nn.py:245-246)"""
        if self.causal > 0:
            self.conv.conv.weight_v.data[:, :, -1, self.causal:].zero_()

    def forward(self, input):
        out = self.pad(input)
        if _WN_SCOPE[0] is None or id(self.conv.conv) not in _WN_SCOPE[0]:     # (a scope masked before it normalised)
            self.mask_weight()
        return self.conv(out)


class HipELU(nn.Module):
    """nn.ELU through evae.ops.elu_dropout (no dropout): forward and backward on the HIP kernels"""

    def forward(self, x):
        return ops.elu_dropout(x)


class GatedResBlock(nn.Module):
    def __init__(self, in_channel, channel, kernel_size, conv='wnconv2d', activation=nn.ELU, dropout=0.1,
                 auxiliary_channel=0, condition_dim=0):
        super().__init__()
        if conv == 'wnconv2d':
            conv_module = partial(WNConv2d, padding=kernel_size // 2)
        elif conv == 'causal_downright':
            conv_module = partial(CausalConv2d, padding='downright')
        elif conv == 'causal':
            conv_module = partial(CausalConv2d, padding='causal')
        self.activation = activation()
        if not (isinstance(self.activation, nn.ELU) and self.activation.alpha == 1.0):
            raise NotImplementedError("GatedResBlock runs ELU (alpha = 1) only: there is no kernel for %r" % (self.activation,))
        self.conv1 = conv_module(in_channel, channel, kernel_size)
        if auxiliary_channel > 0:
            self.aux_conv = WNConv2d(auxiliary_channel, channel, 1)
        self.dropout = nn.Dropout(dropout)
        self.conv2 = conv_module(channel, in_channel * 2, kernel_size)
        if condition_dim > 0:
            self.condition = WNConv2d(condition_dim, in_channel * 2, 1, bias=False)
        self.gate = nn.GLU(1)

    def forward(self, input, aux_input=None, condition=None, rng=None):
        """rng (extension): the (seed, offset) of this call's dropout mask; None draws the next one of the process"""
        if condition is not None:
            raise NotImplementedError("GatedResBlock: the `condition` input is out of scope")
        out = self.conv1(ops.elu_dropout(input))
        if aux_input is not None:
            out = out + self.aux_conv(ops.elu_dropout(aux_input))
        out = ops.elu_dropout(out, self.dropout.p if self.training else 0.0, rng=rng)
        out = self.conv2(out)
        return ops.glu_res(out, input)                 # gate(out) + input


@lru_cache(maxsize=64)
def causal_mask(size):
    """(mask [1, size, size] uint8: 1 where column j < row i; start_mask [size, 1]: 0 for row 0) -- reference
    utils/nn.py:313-323.  The attention kernel applies both itself; this is the reference's helper for callers and tests."""
    shape = [size, size]
    mask = np.triu(np.ones(shape), k=1).astype(np.uint8).T
    start_mask = np.ones(size).astype(np.float32)
    start_mask[0] = 0
    return torch.from_numpy(mask).unsqueeze(0), torch.from_numpy(start_mask).unsqueeze(1)


class CausalAttention(nn.Module):
    def __init__(self, query_channel, key_channel, channel, n_head=8, dropout=0.1):
        super().__init__()
        self.query = wn_linear(query_channel, channel)
        self.key = wn_linear(key_channel, channel)
        self.value = wn_linear(key_channel, channel)
        self.dim_head = channel // n_head
        self.n_head = n_head
        self.dropout = nn.Dropout(dropout)

    def forward(self, query, key, rng=None):
        batch, _, height, width = key.shape
        query_rows, key_rows = _pixel_rows(query), _pixel_rows(key)
        q, k, v = self.query(query_rows), self.key(key_rows), self.value(key_rows)
        out = ops.causal_attn(q, k, v, batch, height * width, self.n_head, self.dropout.p if self.training else 0.0, rng=rng)
        return _from_pixel_rows(out, batch, height, width)


class PixelBlock(nn.Module):
    def __init__(self, in_channel, channel, kernel_size, n_res_block, attention=True, dropout=0.1, condition_dim=0):
        super().__init__()
        resblocks = []
        for i in range(n_res_block):
            resblocks.append(GatedResBlock(in_channel, channel, kernel_size, conv='causal', dropout=dropout,
                                           condition_dim=condition_dim))
        self.resblocks = nn.ModuleList(resblocks)
        self.attention = attention
        if attention:
            self.key_resblock = GatedResBlock(in_channel * 2 + 2, in_channel, 1, dropout=dropout)
            self.query_resblock = GatedResBlock(in_channel + 2, in_channel, 1, dropout=dropout)
            self.causal_attention = CausalAttention(in_channel + 2, in_channel * 2 + 2, in_channel // 2, dropout=dropout)
            self.out_resblock = GatedResBlock(in_channel, in_channel, 1, auxiliary_channel=in_channel // 2, dropout=dropout)
        else:
            self.out = WNConv2d(in_channel + 2, in_channel, 1)

    def forward(self, input, background, condition=None):
        with _wn_scope(self):
            out = input
            for resblock in self.resblocks:
                out = resblock(out, condition=condition)
            if self.attention:
                key = self.key_resblock(torch.cat([input, out, background], 1))
                query = self.query_resblock(torch.cat([out, background], 1))
                attn_out = self.causal_attention(query, key)
                out = self.out_resblock(out, attn_out)
            else:
                out = self.out(torch.cat([out, background], 1))
            return out


class PixelSNAIL(nn.Module):
    def __init__(self, shape, n_class, channel, kernel_size, n_block, n_res_block, res_channel, attention=True, dropout=0.1,
                 n_cond_res_block=0, cond_res_channel=0, cond_res_kernel=3, n_out_res_block=0):
        super().__init__()
        height, width = shape
        self.n_class = n_class
        if n_cond_res_block > 0:
            raise NotImplementedError("PixelSNAIL: the conditioning network (n_cond_res_block > 0) is out of scope")
        kernel = kernel_size + 1 if kernel_size % 2 == 0 else kernel_size
        self.horizontal = CausalConv2d(3, channel, [kernel // 2, kernel], padding='down')
        self.vertical = CausalConv2d(3, channel, [(kernel + 1) // 2, kernel // 2], padding='downright')
        coord_x = (torch.arange(height).float() - height / 2) / height
        coord_x = coord_x.view(1, 1, height, 1).expand(1, 1, height, width)
        coord_y = (torch.arange(width).float() - width / 2) / width
        coord_y = coord_y.view(1, 1, 1, width).expand(1, 1, height, width)
        self.register_buffer('background', torch.cat([coord_x, coord_y], 1))
        self.blocks = nn.ModuleList()
        for i in range(n_block):
            self.blocks.append(PixelBlock(channel, res_channel, kernel_size, n_res_block, attention=attention, dropout=dropout,
                                          condition_dim=cond_res_channel))
        out = []
        for i in range(n_out_res_block):
            out.append(GatedResBlock(channel, res_channel, 1))
        out.extend([HipELU(), WNConv2d(channel, n_class, 1)])
        self.out = nn.Sequential(*out)

    def forward(self, input, condition=None, cache=None):
        if condition is not None:
            raise NotImplementedError("PixelSNAIL: the `condition` input is out of scope")
        batch, _, height, width = input.shape
        with _wn_scope(self):
            horizontal = shift_down(self.horizontal(input))
            vertical = shift_right(self.vertical(input))
            out = horizontal + vertical
            background = self.background[:, :, :height, :].expand(batch, 2, height, width)
            for block in self.blocks:
                out = block(out, background, condition=condition)
            return self.out(out)
