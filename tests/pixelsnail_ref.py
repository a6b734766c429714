"""Restatement (torch on the CPU, any float dtype: float64 is the reference value, float32 the yardstick of a tolerance) of the
PixelSNAIL decoder and of the `pixelcnn` model's loss, written from the formulas of the model it follows (utils/nn.py:148-562,
models/PixelCNN.py, models/AbsHModel.py, utils/distributions.py of the reference) and not from the kernels: the attention
materialises its [L x L] scores, fills the columns j >= i with -1e4, takes the softmax over all L columns and multiplies row 0 by
zero.  Dropout masks are inputs; `attn_keep_mask` / `flat_keep_mask` build them from tests/philox_ref.py in the layout the
kernels document (include/evae_hip.h).

Everything is a function of a state dict {name: tensor} with the reference's names; gradients come from torch.autograd over
these functions."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import philox_ref as pr

LOG_2_PI = math.log(2 * math.pi)


# ---- dropout masks ---------------------------------------------------------------------------------------------------
def flat_keep_mask(n, p_drop, seed, offset, first=0):
    """keep [n] (bool) of the elements first, first + 1, ..., first + n - 1 (first: a multiple of 4, < 2^64): element e takes word
    e % 4 of quad e // 4, counter (quad_lo, quad_hi, offset_lo, offset_hi), key (seed_lo, seed_hi); keep <=> u01(word) >= p_drop
    (compared in float32)"""
    n, first = int(n), int(first)
    assert first >= 0 and first % 4 == 0 and first + n <= 1 << 64, (first, n)
    quad = np.uint64(first // 4) + np.arange((n + 3) // 4, dtype=np.uint64)
    offset = int(offset)
    ctr = (quad & pr.MASK, quad >> np.uint64(32), np.uint64(offset & 0xFFFFFFFF), np.uint64((offset >> 32) & 0xFFFFFFFF))
    words = np.stack(pr.philox4x32_10(ctr, pr.seed_key(seed)), axis=1).reshape(-1)[:n]
    return pr.u01(words) >= np.float32(p_drop)


def attn_keep_mask(BH, L, p_drop, seed, offset):
    """keep [BH, L, L]: element e = ((b H + h) L + i) L + j of the flattened probabilities"""
    return flat_keep_mask(BH * L * L, p_drop, seed, offset).reshape(BH, L, L)


def attn_keep_mask_head(bh, L, p_drop, seed, offset, wrap_bits=None):
    """keep [L, L] of head bh = b H + h alone: attn_keep_mask(...)[bh] without the heads before it.  wrap_bits: the mask a kernel
    would draw that kept only the low `wrap_bits` bits of the element index (a multiple-of-4 boundary: wrap_bits >= 2) -- what a
    test shows its case to differ from, never a reference value."""
    n = L * L
    e0 = int(bh) * n
    lead = e0 % 4                                       # (odd L: the head starts inside a quad)
    if wrap_bits is None:
        return flat_keep_mask(lead + n, p_drop, seed, offset, e0 - lead)[lead:].reshape(L, L)
    period = 1 << wrap_bits
    parts, e = [], e0
    while e < e0 + n:                                   # runs of elements between two multiples of the period
        run = min(e0 + n, (e // period + 1) * period) - e
        skip = (e % period) % 4
        parts.append(flat_keep_mask(skip + run, p_drop, seed, offset, e % period - skip)[skip:])
        e += run
    return np.concatenate(parts).reshape(L, L)


# ---- pieces ----------------------------------------------------------------------------------------------------------------
def elu(x):
    return torch.where(x > 0, x, torch.expm1(torch.clamp(x, max=0)))


def causal_attention_core(q, k, v, keep=None, p_drop=0.0):
    """q, k, v [BH, L, dh] -> out [BH, L, dh].  keep [BH, L, L] (bool / 0-1) or None"""
    BH, L, dh = q.shape
    s = torch.matmul(q, k.transpose(1, 2)) / math.sqrt(dh)
    i = torch.arange(L).view(L, 1)
    j = torch.arange(L).view(1, L)
    s = s.masked_fill((j >= i).unsqueeze(0), -1e4)
    p = torch.softmax(s, 2)
    start = torch.ones(L, 1, dtype=q.dtype)
    start[0] = 0
    p = p * start
    if keep is not None:
        p = p * torch.as_tensor(np.asarray(keep), dtype=q.dtype) / (1.0 - p_drop)
    return torch.matmul(p, v)


def rows_to_heads(x, B, L, H):
    """[B*L, H*dh] rows -> [B*H, L, dh]"""
    return x.view(B, L, H, -1).transpose(1, 2).reshape(B * H, L, -1)


def heads_to_rows(x, B, L, H):
    return x.view(B, H, L, -1).transpose(1, 2).reshape(B * L, -1)


def causal_attention_rows(q, k, v, B, L, H, keep=None, p_drop=0.0):
    """the operator's interface: rows [B*L, H*dh] in and out"""
    out = causal_attention_core(rows_to_heads(q, B, L, H), rows_to_heads(k, B, L, H), rows_to_heads(v, B, L, H), keep, p_drop)
    return heads_to_rows(out, B, L, H)


def wn_weight(sd, prefix):
    """weight normalisation over all dimensions but the first: w = v * g / ||v||"""
    v, g = sd[prefix + ".weight_v"], sd[prefix + ".weight_g"]
    norm = v.reshape(v.shape[0], -1).pow(2).sum(1).sqrt().view(-1, *([1] * (v.dim() - 1)))
    return v * (g / norm)


def wn_linear(sd, prefix, x):
    return F.linear(x, wn_weight(sd, prefix), sd[prefix + ".bias"])


def wn_conv(sd, prefix, x, padding=0):
    return F.conv2d(x, wn_weight(sd, prefix + ".conv"), sd.get(prefix + ".conv.bias"), padding=padding)


def causal_conv(sd, prefix, x, kernel_size, padding):
    kh, kw = kernel_size
    if padding == "downright":
        pad = [kw - 1, 0, kh - 1, 0]
    else:                                # 'down', 'causal'
        pad = [kw // 2, kw // 2, kh - 1, 0]
    if padding == "causal":
        # the taps right of the centre in the last filter row are zeroed IN THE STORED VALUES, outside autograd, as the model does it
        # on every call: the gradient wrt weight_v at those taps is that of an ordinary weight whose value happens to be zero
        sd[prefix + ".conv.conv.weight_v"].data[:, :, -1, kw // 2:] = 0
    return wn_conv(sd, prefix + ".conv", F.pad(x, pad))


def causal_attention(sd, prefix, query, key, n_head=8, keep=None, p_drop=0.0):
    B, _, hh, ww = key.shape
    L = hh * ww
    qf = query.reshape(B, query.shape[1], L).transpose(1, 2).reshape(B * L, -1)
    kf = key.reshape(B, key.shape[1], L).transpose(1, 2).reshape(B * L, -1)
    out = causal_attention_rows(wn_linear(sd, prefix + ".query", qf), wn_linear(sd, prefix + ".key", kf),
                                wn_linear(sd, prefix + ".value", kf), B, L, n_head, keep, p_drop)
    return out.view(B, hh, ww, -1).permute(0, 3, 1, 2)


def gated_resblock(sd, prefix, x, kernel_size, conv="wnconv2d", aux=None, keep=None, p_drop=0.0):
    """keep: the dropout mask over the NCHW-shaped activation (None: eval mode)"""
    def conv_(name, t):
        if conv == "wnconv2d":
            return wn_conv(sd, prefix + "." + name, t, padding=kernel_size // 2)
        return causal_conv(sd, prefix + "." + name, t, [kernel_size, kernel_size], "causal" if conv == "causal" else "downright")
    out = conv_("conv1", elu(x))
    if aux is not None:
        out = out + wn_conv(sd, prefix + ".aux_conv", elu(aux))
    out = elu(out)
    if keep is not None:
        out = out * torch.as_tensor(np.asarray(keep), dtype=x.dtype) / (1.0 - p_drop)
    out = conv_("conv2", out)
    a, b = out.chunk(2, dim=1)
    return a * torch.sigmoid(b) + x


def pixel_block(sd, prefix, x, background, kernel_size, n_res_block):
    out = x
    for r in range(n_res_block):
        out = gated_resblock(sd, "%s.resblocks.%d" % (prefix, r), out, kernel_size, conv="causal")
    key = gated_resblock(sd, prefix + ".key_resblock", torch.cat([x, out, background], 1), 1)
    query = gated_resblock(sd, prefix + ".query_resblock", torch.cat([out, background], 1), 1)
    attn = causal_attention(sd, prefix + ".causal_attention", query, key)
    return gated_resblock(sd, prefix + ".out_resblock", out, 1, aux=attn)


def pixelsnail(sd, x, kernel_size, n_block, n_res_block, prefix=""):
    """eval-mode forward of PixelSNAIL(shape, n_class, channel, kernel_size, n_block, n_res_block, res_channel) with attention and
    no out-resblocks; `shape` is read from the `background` buffer"""
    pre = prefix + "." if prefix else ""
    B, _, hh, ww = x.shape
    kernel = kernel_size + 1 if kernel_size % 2 == 0 else kernel_size
    hor = causal_conv(sd, pre + "horizontal", x, [kernel // 2, kernel], "down")
    ver = causal_conv(sd, pre + "vertical", x, [(kernel + 1) // 2, kernel // 2], "downright")
    out = F.pad(hor, [0, 0, 1, 0])[:, :, :hh, :] + F.pad(ver, [1, 0, 0, 0])[:, :, :, :ww]
    background = sd[pre + "background"][:, :, :hh, :].expand(B, 2, hh, ww)
    for b in range(n_block):
        out = pixel_block(sd, "%sblocks.%d" % (pre, b), out, background, kernel_size, n_res_block)
    return wn_conv(sd, pre + "out.1", elu(out))


# ---- the model ---------------------------------------------------------------------------------------------------------
_ENC_WIDE = ((7, 1, 3), (3, 2, 1), (5, 1, 2), (3, 2, 1), (3, 1, 1))       # (kernel, stride, padding)
_ENC_NARROW = ((3, 1, 1), (3, 2, 1), (3, 1, 1), (3, 2, 1), (3, 1, 1))


def _gated_conv_stack(sd, prefix, x, table):
    for n, (k, s, p) in enumerate(table):
        h = F.conv2d(x, sd["%s.%d.h.weight" % (prefix, n)], sd["%s.%d.h.bias" % (prefix, n)], stride=s, padding=p)
        g = F.conv2d(x, sd["%s.%d.g.weight" % (prefix, n)], sd["%s.%d.g.bias" % (prefix, n)], stride=s, padding=p)
        x = h * torch.sigmoid(g)
    return x


def _gated_dense(sd, prefix, x):
    return F.linear(x, sd[prefix + ".h.weight"], sd[prefix + ".h.bias"]) * torch.sigmoid(F.linear(x, sd[prefix + ".g.weight"], sd[prefix + ".g.bias"]))


def _heads(sd, prefix, h):
    mean = F.linear(h, sd[prefix + "_mean.linear.weight"], sd[prefix + "_mean.linear.bias"])
    logvar = F.linear(h, sd[prefix + "_logvar.linear.weight"], sd[prefix + "_logvar.linear.bias"]).clamp(-6.0, 2.0)
    return mean, logvar


def _log_normal_diag(x, mean, log_var):
    return (-0.5 * (log_var + LOG_2_PI + (x - mean).pow(2) / torch.exp(log_var))).sum(1)


def pixelcnn_decoder_mean(sd, x_img, z1, z2):
    """p(x | z1, z2, x): [B, D] means (binary inputs)"""
    B = x_img.shape[0]
    h = torch.cat((x_img, _gated_dense(sd, "p_x_layers_z1.0", z1).view(x_img.shape), _gated_dense(sd, "p_x_layers_z2.0", z2).view(x_img.shape)), 1)
    top = pixelsnail(sd, h, 3, 1, 4, prefix="pixelcnn")
    return torch.sigmoid(F.conv2d(top, sd["p_x_mean.conv.weight"], sd["p_x_mean.conv.bias"])).reshape(B, -1)


def pixelcnn_posterior(sd, img, eps2, eps1):
    """(z1, q1_mu, q1_lv, z2, q2_mu, q2_lv): the samples of q(z2 | x) and q(z1 | x, z2) for images [B, 1, 28, 28] and their noise"""
    B = img.shape[0]
    q2_mu, q2_lv = _heads(sd, "q_z", _gated_conv_stack(sd, "q_z_layers", img, _ENC_WIDE).reshape(B, -1))
    z2 = q2_mu + eps2 * torch.exp(0.5 * q2_lv)
    joint = torch.cat((_gated_conv_stack(sd, "q_z1_layers_x", img, _ENC_NARROW).reshape(B, -1), _gated_dense(sd, "q_z1_layers_z2.0", z2)), 1)
    q1_mu, q1_lv = _heads(sd, "q_z1", _gated_dense(sd, "q_z1_layers_joint.0", joint))
    z1 = q1_mu + eps1 * torch.exp(0.5 * q1_lv)
    return z1, q1_mu, q1_lv, z2, q2_mu, q2_lv


def pixelcnn_loss(sd, x, eps2, eps1, exemplars, beta=1.0, input_size=(1, 28, 28)):
    """(loss, RE, KL) per row of the eval-mode `pixelcnn` model with the exemplar prior over the encodings of `exemplars` [C, D]
    (no leave-one-out mask: evaluation), binary inputs.  eps2 / eps1: the noise of z2 and of z1."""
    B = x.shape[0]
    img = x.view(B, *input_size)
    z1, q1_mu, q1_lv, z2, q2_mu, q2_lv = pixelcnn_posterior(sd, img, eps2, eps1)
    p1_mu, p1_lv = _heads(sd, "p_z1", _gated_dense(sd, "p_z1_layers_z2.1", _gated_dense(sd, "p_z1_layers_z2.0", z2)))
    mean = pixelcnn_decoder_mean(sd, img, z1, z2)
    probs = mean.clamp(1e-5, 1.0 - 1e-5)
    RE = (x * torch.log(probs) + (1.0 - x) * torch.log(1.0 - probs)).sum(1)
    C = exemplars.shape[0]
    centres = F.linear(_gated_conv_stack(sd, "q_z_layers", exemplars.view(C, *input_size), _ENC_WIDE).reshape(C, -1),
                       sd["q_z_mean.linear.weight"], sd["q_z_mean.linear.bias"])
    lv = sd["prior_log_variance"].reshape(1, 1).expand(1, z2.shape[1])
    dist = ((z2.unsqueeze(1) - centres.unsqueeze(0)).pow(2) / torch.exp(lv).unsqueeze(0)).sum(2)
    prob = -0.5 * (lv + LOG_2_PI).sum(1) - 0.5 * dist - math.log(C)
    log_p_z2 = torch.logsumexp(prob, 1)
    KL = (_log_normal_diag(z1, q1_mu, q1_lv) - _log_normal_diag(z1, p1_mu, p1_lv)) + (_log_normal_diag(z2, q2_mu, q2_lv) - log_p_z2)
    return -RE + beta * KL, RE, KL
