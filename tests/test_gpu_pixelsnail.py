"""The PixelSNAIL decoder of model_name 'pixelcnn' on the HIP path (csrc/evae_attn.hip behind evae.ops.causal_attn / elu_dropout /
glu_res, utils/nn.py's PixelSNAIL layers, models/PixelCNN.py) against the float64 restatement tests/pixelsnail_ref.py and the
reference goldens G27.

Tolerance of every compared tensor: the yardstick is the error of the SAME restatement evaluated in float32 on the CPU against its
float64 value, on the same inputs, as max |a - b| over the tensor; the HIP result gets 4 x that, plus one float32 ulp of the
tensor's largest magnitude (the kernels sum up to 1535 terms in another order, and large GEMMs run split-bf16 at fp32-GEMM accuracy).
Each figure is printed before it is asserted (ratio = HIP error / yardstick)."""
import math

import numpy as np
import pytest
import torch

import golden_inputs as gi
import pixelsnail_ref as psr
import smoke_case

pytestmark = pytest.mark.gpu

ATTN_MAX_LEN = 1536                                                                  # ops.causal_attn_max_len(): asserted below
ATTN_SHAPES = [(2, 8, 784), (3, 1, 1), (1, 3, 2), (5, 1, 65), (1, 1, 257),           # (B, H, L): B*H = 16, 3, 3, 5, 1
               # a thread takes pair p, p + 256, ...: exactly 256 pairs, 257 (odd L: its middle row once), and three full rounds
               # at the LDS limit, 1535 with the middle row in the last one
               (1, 1, 512), (1, 2, 513), (1, 1, ATTN_MAX_LEN - 1), (1, 2, ATTN_MAX_LEN)]
P_DROP, RNG = 0.1, (0x1234567887654321, 0x100000003)                                 # (seed, offset): both halves of each in use


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def close(tag, got, ref64, ref32):
    """|got - ref64| <= 4 |ref32 - ref64| + ulp32(max |ref64|), all as maxima over the tensor"""
    got, ref64, ref32 = (np.asarray(a, np.float64) for a in (got, ref64, ref32))
    assert got.shape == ref64.shape == ref32.shape, (tag, got.shape, ref64.shape)
    assert np.isfinite(got).all(), tag
    err, yard = np.abs(got - ref64).max(initial=0.0), np.abs(ref32 - ref64).max(initial=0.0)
    ulp = float(np.spacing(np.float32(np.abs(ref64).max(initial=0.0))))
    print("%-60s err %.3e  yardstick %.3e  ratio %6.2f  ulp %.1e" % (tag, err, yard, err / max(yard, 1e-300), ulp))
    return err <= 4.0 * yard + ulp, (tag, err, yard, ulp)


def assert_all(results):
    bad = [info for ok, info in results if not ok]
    assert not bad, bad


@pytest.fixture(scope="module")
def ops():
    from evae import ops as o
    return o


# ---- attention ------------------------------------------------------------------------------------------------------------
def _attn_inputs(B, H, L):
    rs = np.random.RandomState(2700 + B * 1000 + H * 100 + L)
    q, k, v, go = (rs.randn(B * L, H * 4).astype(np.float32) for _ in range(4))
    return q, k, v, go


def _attn_ref(dtype, q, k, v, go, B, H, L, keep, p):
    t = [torch.from_numpy(a).to(dtype).requires_grad_(True) for a in (q, k, v)]
    out = psr.causal_attention_rows(*t, B, L, H, keep, p)
    (out * torch.from_numpy(go).to(dtype)).sum().backward()
    return [out.detach().numpy()] + [a.grad.numpy() for a in t]


def _attn_hip(ops, q, k, v, go, B, H, L, p, rng):
    t = [dev(a).requires_grad_(True) for a in (q, k, v)]
    out = ops.causal_attn(*t, B, L, H, p, rng=rng)
    out.backward(dev(go))
    return [host(out)] + [host(a.grad) for a in t]


@pytest.mark.parametrize("B,H,L", ATTN_SHAPES)
@pytest.mark.parametrize("drop", [False, True])
def test_attention_matches_ref(ops, B, H, L, drop):
    q, k, v, go = _attn_inputs(B, H, L)
    s = np.einsum("bihd,bjhd->bhij", q.reshape(B, L, H, 4), k.reshape(B, L, H, 4)) / 2
    assert np.abs(s).max() < 50
    p = P_DROP if drop else 0.0
    keep = psr.attn_keep_mask(B * H, L, p, *RNG) if drop else None
    if drop and L > 2:
        assert 0 < keep.mean() < 1
    r64 = _attn_ref(torch.float64, q, k, v, go, B, H, L, keep, p)
    r32 = _attn_ref(torch.float32, q, k, v, go, B, H, L, keep, p)
    got = _attn_hip(ops, q, k, v, go, B, H, L, p, RNG)
    rows0 = got[0].reshape(B, L, H * 4)[:, 0]
    assert np.abs(rows0).max() == 0.0                                    # row 0: exactly zero
    if L == 1:
        assert all(np.abs(g).max() == 0.0 for g in got)                  # zero output and zero gradients
    assert np.abs(got[1].reshape(B, L, H * 4)[:, 0]).max() == 0.0        # ... and row 0 of dq
    assert np.abs(got[2].reshape(B, L, H * 4)[:, L - 1]).max() == 0.0    # nobody attends to the last position
    assert_all([close("attn B%d H%d L%d drop=%d %s" % (B, H, L, drop, n), g, a, b)
                for n, g, a, b in zip(("out", "dq", "dk", "dv"), got, r64, r32)])


def test_attention_p0_is_bit_equal_to_no_dropout_and_runs_are_bit_identical(ops):
    B, H, L = 2, 8, 65
    q, k, v, go = _attn_inputs(B, H, L)
    plain = _attn_hip(ops, q, k, v, go, B, H, L, 0.0, None)
    p0 = _attn_hip(ops, q, k, v, go, B, H, L, 0.0, RNG)
    assert all(np.array_equal(a, b) for a, b in zip(plain, p0))
    one = _attn_hip(ops, q, k, v, go, B, H, L, P_DROP, RNG)
    two = _attn_hip(ops, q, k, v, go, B, H, L, P_DROP, RNG)
    assert all(np.array_equal(a, b) for a, b in zip(one, two))          # out, dq, dk, dv: bit-identical across runs
    other = _attn_hip(ops, q, k, v, go, B, H, L, P_DROP, (RNG[0], RNG[1] + 1))
    assert not np.array_equal(one[0], other[0]) and not np.array_equal(one[0], plain[0])


def test_attention_dropout_counter_advances(ops):
    """without an explicit rng every call takes the next offset: two calls, two masks; p = 0 and eval leave the counter alone"""
    B, H, L = 1, 2, 33
    q, k, v, go = _attn_inputs(B, H, L)
    t = [dev(a) for a in (q, k, v)]
    n0 = ops._DROPOUT_CALLS[0]
    ops.causal_attn(*t, B, L, H, 0.0)
    assert ops._DROPOUT_CALLS[0] == n0
    a = ops.causal_attn(*t, B, L, H, P_DROP)
    b = ops.causal_attn(*t, B, L, H, P_DROP)
    assert ops._DROPOUT_CALLS[0] == n0 + 2 and not torch.equal(a, b)
    again = ops.causal_attn(*t, B, L, H, P_DROP, rng=(torch.initial_seed(), n0))
    assert torch.equal(a, again)


def _head_rows(t, B, H, L, bh):
    """head bh = b H + h of a device tensor of rows [B*L, H*4] -> host [1, L, 4]"""
    b, h = divmod(bh, H)
    return host(t.view(B, L, H, 4)[b, :, h]).reshape(1, L, 4).copy()


def test_attention_dropout_element_index_is_64_bit(ops):
    """B H L^2 = 1.72e10 probabilities: head 1820 holds element e = 2^32 (in row 682), head 7281 holds e = 2^34, from where on the
    quad's second counter word is 1.  Four heads against the restatement under the mask of THEIR element indices; the two straddling
    heads' masks differ from what an index cut to 32 bits (a quad cut to 32 bits) would draw, so this case tells the two apart."""
    B, H, L = 1821, 4, ATTN_MAX_LEN
    n = L * L
    straddle = {1820: 32, 7281: 34}                                     # head: log2 of the element index it crosses
    for bh, bits in straddle.items():
        assert bh * n < 1 << bits < (bh + 1) * n
    assert ((1 << 32) - 1820 * n) // L == 682 and B * H * n > 1 << 34
    gen = torch.Generator(device="cuda")
    gen.manual_seed(2790)
    q, k, v, go = (torch.randn(B * L, H * 4, generator=gen, device="cuda") for _ in range(4))
    for a in (q, k, v):
        a.requires_grad_(True)
    out = ops.causal_attn(q, k, v, B, L, H, P_DROP, rng=RNG)
    out.backward(go)
    lower = np.tril(np.ones((L, L), bool), -1)                          # the entries j < i: the ones the kernel draws
    res = []
    for bh in (0, 1820, 7281, 7283):
        qh, kh, vh, goh = (_head_rows(a, B, H, L, bh) for a in (q, k, v, go))
        assert np.abs(qh[0] @ kh[0].T).max() / 2 < 50
        keep = psr.attn_keep_mask_head(bh, L, P_DROP, *RNG)
        assert 0 < keep.mean() < 1
        if bh in straddle:
            bits = straddle[bh]
            wrapped = psr.attn_keep_mask_head(bh, L, P_DROP, *RNG, wrap_bits=bits)
            row = ((1 << bits) - bh * n) // L                           # the row that holds the crossing
            differ = int(((wrapped != keep) & lower).sum())
            print("head %d: a %d-bit index draws %d other entries with j < i, all in rows >= %d" % (bh, bits, differ, row))
            assert np.array_equal(wrapped[:row], keep[:row]) and differ > 0

        def ref(dtype):
            t = [torch.from_numpy(a).to(dtype).requires_grad_(True) for a in (qh, kh, vh)]
            o = psr.causal_attention_core(*t, keep[None], P_DROP)
            (o * torch.from_numpy(goh).to(dtype)).sum().backward()
            return [o.detach().numpy()] + [a.grad.numpy() for a in t]

        got = [_head_rows(a, B, H, L, bh) for a in (out, q.grad, k.grad, v.grad)]
        res += [close("attn B%d H%d L%d head %d %s" % (B, H, L, bh, name), g, a, b)
                for name, g, a, b in zip(("out", "dq", "dk", "dv"), got, ref(torch.float64), ref(torch.float32))]
    assert_all(res)


def test_attention_refuses_unsupported_shapes(ops):
    from evae._lib import EvaeError
    x8 = torch.zeros(2 * 16, 2 * 8, device="cuda")
    with pytest.raises(EvaeError, match="head width"):
        ops.causal_attn(x8, x8, x8, 2, 16, 2)                            # dh = 8
    longest = ops.causal_attn_max_len()
    assert longest == ATTN_MAX_LEN
    xl = torch.zeros(longest + 1, 4, device="cuda")
    with pytest.raises(EvaeError, match="LDS"):
        ops.causal_attn(xl, xl, xl, 1, longest + 1, 1)
    ok = ops.causal_attn(xl[:longest], xl[:longest], xl[:longest], 1, longest, 1)        # the longest itself is accepted
    assert ok.shape == (longest, 4) and float(ok.abs().max()) == 0.0


# ---- element-wise operators --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [1, 63, 4097, "cl"])
@pytest.mark.parametrize("drop", [False, True])
def test_elu_dropout_matches_ref(ops, kind, drop):
    rs = np.random.RandomState(2751)
    if kind == "cl":                      # logical [2, 128, 6, 5] over [2, 6, 5, 128] storage: the mask follows the storage
        store = (rs.randn(2, 6, 5, 128) * 2).astype(np.float32)
        x = np.transpose(store, (0, 3, 1, 2))
        go = np.transpose(rs.randn(2, 6, 5, 128).astype(np.float32), (0, 3, 1, 2))
        xt = dev(store).permute(0, 3, 1, 2).requires_grad_(True)
        assert xt.is_contiguous(memory_format=torch.channels_last)
        got = dev(np.ascontiguousarray(go)).contiguous(memory_format=torch.channels_last)
    else:
        x = (rs.randn(kind) * 2).astype(np.float32)
        go = rs.randn(kind).astype(np.float32)
        xt, got = dev(x).requires_grad_(True), dev(go)
    p = P_DROP if drop else 0.0
    keep = None
    if drop:
        keep = psr.flat_keep_mask(x.size, p, *RNG)
        keep = np.transpose(keep.reshape(2, 6, 5, 128), (0, 3, 1, 2)) if kind == "cl" else keep

    def ref(dtype):
        t = torch.from_numpy(np.ascontiguousarray(x)).to(dtype).requires_grad_(True)
        y = psr.elu(t)
        if drop:
            y = y * torch.from_numpy(np.ascontiguousarray(keep)).to(dtype) / (1.0 - p)
        (y * torch.from_numpy(np.ascontiguousarray(go)).to(dtype)).sum().backward()
        return y.detach().numpy(), t.grad.numpy()

    y = ops.elu_dropout(xt, p, rng=RNG)
    assert y.stride() == xt.stride()
    y.backward(got)
    r64, r32 = ref(torch.float64), ref(torch.float32)
    assert_all([close("elu_dropout %s drop=%d %s" % (kind, drop, n), g, a, b)
                for n, g, a, b in zip(("out", "dx"), (host(y), host(xt.grad)), r64, r32)])
    if drop:
        assert (host(y)[~keep] == 0.0).all() and (host(xt.grad)[~keep] == 0.0).all()
    else:
        y0 = ops.elu_dropout(xt.detach())
        assert torch.equal(y0, y.detach())                               # p = 0 is the call without dropout


@pytest.mark.parametrize("M,C", [(1, 1), (7, 9), (17, 241), ("cl", 64)])
def test_glu_res_matches_ref(ops, M, C):
    rs = np.random.RandomState(2760 + C)
    if M == "cl":                         # ab: a [2, 6, 5, 128] channels-last tensor, x: its 64-channel companion
        ab = np.transpose(rs.randn(2, 6, 5, 2 * C).astype(np.float32), (0, 3, 1, 2))
        x = np.transpose(rs.randn(2, 6, 5, C).astype(np.float32), (0, 3, 1, 2))
        go = np.transpose(rs.randn(2, 6, 5, C).astype(np.float32), (0, 3, 1, 2))
        mk = lambda a: dev(np.ascontiguousarray(a)).contiguous(memory_format=torch.channels_last)
    else:
        ab, x, go = (rs.randn(M, n).astype(np.float32) for n in (2 * C, C, C))
        mk = dev
    abt, xt = mk(ab).requires_grad_(True), mk(x).requires_grad_(True)
    out = ops.glu_res(abt, xt)
    out.backward(mk(go))

    def ref(dtype):
        a = torch.from_numpy(np.ascontiguousarray(ab)).to(dtype).requires_grad_(True)
        b = torch.from_numpy(np.ascontiguousarray(x)).to(dtype).requires_grad_(True)
        h, g = a.chunk(2, dim=1)
        y = h * torch.sigmoid(g) + b
        (y * torch.from_numpy(np.ascontiguousarray(go)).to(dtype)).sum().backward()
        return y.detach().numpy(), a.grad.numpy(), b.grad.numpy()

    r64, r32 = ref(torch.float64), ref(torch.float32)
    assert_all([close("glu_res %s x %d %s" % (M, C, n), g, a, b)
                for n, g, a, b in zip(("out", "dab", "dx"), (host(out), host(abt.grad), host(xt.grad)), r64, r32)])


# ---- layers against the reference goldens ---------------------------------------------------------------------------------
def _golden_case(g, module, ref_fn, inputs):
    """module: this project's layer with the golden's float32 parameters; ref_fn(sd, *xs): the restatement.  Outputs, input
    gradients and every parameter gradient against the GOLDEN (the reference's float64), yardstick from the restatement."""
    sd = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("p.")}
    module.load_state_dict(sd)
    module.cuda().eval()
    xs = [dev(g["x." + n]).requires_grad_(True) for n in inputs]
    out = module(*xs)
    out.backward(dev(g["gout"]))

    def ref(dtype):
        s = {k: v.to(dtype).clone().requires_grad_(not k.endswith("background")) for k, v in sd.items()}
        t = [torch.from_numpy(g["x." + n]).to(dtype).requires_grad_(True) for n in inputs]
        y = ref_fn(s, *t)
        (y * torch.from_numpy(g["gout"]).to(dtype)).sum().backward()
        return y.detach().numpy(), [a.grad.numpy() for a in t], {k: v.grad.numpy() for k, v in s.items() if v.grad is not None}

    y64, dx64, gp64 = ref(torch.float64)
    y32, dx32, gp32 = ref(torch.float32)
    assert np.abs(y64 - g["out"]).max() < 1e-9 * np.abs(g["out"]).max()          # (the restatement IS the golden: test_pixelsnail_host.py)
    res = [close("out", host(out), g["out"], y32)]
    for n, x, a in zip(inputs, xs, dx32):
        res.append(close("dx." + n, host(x.grad), g["dx." + n], a))
    named = dict(module.named_parameters())
    names = [k[2:] for k in g.files if k.startswith("g.")]
    assert names and set(names) == set(named)
    for n in names:
        assert named[n].grad is not None, n
        res.append(close("g." + n, host(named[n].grad), g["g." + n], gp32[n]))
    return res


def test_causal_attention_layer_matches_golden(golden):
    from utils.nn import CausalAttention
    g = golden("g27_attention")
    assert_all(_golden_case(g, CausalAttention(66, 130, 32),
                            lambda sd, q, k: psr.causal_attention({"m." + n: v for n, v in sd.items()}, "m", q, k), ["query", "key"]))


def test_gated_resblock_layer_matches_golden(golden):
    from utils.nn import GatedResBlock
    g = golden("g27_gated_resblock")
    assert_all(_golden_case(g, GatedResBlock(16, 16, 3, conv='causal'),
                            lambda sd, x: psr.gated_resblock({"m." + n: v for n, v in sd.items()}, "m", x, 3, conv="causal"), ["input"]))


def test_pixelsnail_matches_golden(golden):
    from utils.nn import PixelSNAIL
    g = golden("g27_pixelsnail")
    assert_all(_golden_case(g, PixelSNAIL([6, 5], 64, 64, 3, 1, 0, 64), lambda sd, x: psr.pixelsnail(sd, x, 3, 1, 0), ["input"]))


def test_layer_dropout_is_reproducible_from_rng():
    """training mode: a GatedResBlock's output under an explicit (seed, offset) is the restatement's under the rebuilt mask"""
    from utils.nn import GatedResBlock
    torch.manual_seed(277)
    blk = GatedResBlock(16, 16, 1, dropout=P_DROP)
    sd = {k: v.clone() for k, v in blk.state_dict().items()}
    blk.cuda().train()
    x = np.random.RandomState(278).randn(2, 16, 6, 5).astype(np.float32)
    xt = dev(x).contiguous(memory_format=torch.channels_last)
    out = blk(xt, rng=RNG)
    # the dropped activation is the channels-last [2, 6, 5, 16] output of conv1: the mask follows that storage
    keep = np.transpose(psr.flat_keep_mask(2 * 6 * 5 * 16, P_DROP, *RNG).reshape(2, 6, 5, 16), (0, 3, 1, 2))
    ref = lambda dt: psr.gated_resblock({"m." + n: v.to(dt) for n, v in sd.items()}, "m", torch.from_numpy(x).to(dt), 1,
                                        keep=np.ascontiguousarray(keep), p_drop=P_DROP).numpy()
    assert_all([close("gated_resblock train", host(out), ref(torch.float64), ref(torch.float32))])
    assert torch.equal(out, blk(xt, rng=RNG)) and not torch.equal(out, blk(xt, rng=(RNG[0], RNG[1] + 1)))


# ---- the model ---------------------------------------------------------------------------------------------------------
B_MODEL, C_MODEL = 2, 6


@pytest.fixture(scope="module")
def model_case():
    """the pixelcnn model at B = 2, 28 x 28, eval mode, seeded weights; the loss and every parameter gradient of the restatement
    in float64 and float32 for the same state dict, images, exemplars and noise (computed once)"""
    from utils.utils import importing_model
    args = smoke_case.vae_args(model_name="pixelcnn", number_components=C_MODEL, training_set_size=C_MODEL)
    torch.manual_seed(271)
    model = importing_model(args)(args)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model.cuda().eval()
    x = gi.binary_images(272, B_MODEL)
    ex = gi.binary_images(273, C_MODEL)
    rs = np.random.RandomState(274)
    eps2, eps1 = rs.randn(B_MODEL, 40).astype(np.float32), rs.randn(B_MODEL, 40).astype(np.float32)

    def ref(dtype):
        s = {k: v.to(dtype).clone().requires_grad_(v.dtype.is_floating_point and not k.endswith("background")) for k, v in sd.items()}
        loss, RE, KL = psr.pixelcnn_loss(s, *(torch.from_numpy(a).to(dtype) for a in (x, eps2, eps1, ex)))
        loss.sum().backward()
        return ([t.detach().numpy() for t in (loss, RE, KL)], {k: v.grad.numpy() for k, v in s.items() if v.grad is not None})

    return dict(args=args, model=model, sd=sd, x=x, ex=ex, eps=(eps2, eps1), r64=ref(torch.float64), r32=ref(torch.float32))


def test_model_loss_and_gradients_match_ref(model_case):
    c = model_case
    model = c["model"]
    draws = iter(dev(e) for e in c["eps"])
    model._draw_eps = lambda like: next(draws)
    try:
        model.zero_grad()
        centres, logvar = model.q_z(dev(c["ex"]), prior=True)
        emb = (centres, logvar, torch.arange(C_MODEL, device="cuda"))
        loss, RE, KL = model.calculate_loss((dev(c["x"]), None), exemplars_embedding=emb)
        loss.sum().backward()
    finally:
        del model._draw_eps
    (l64, re64, kl64), g64 = c["r64"]
    (l32, re32, kl32), g32 = c["r32"]
    res = [close("loss", host(loss), l64, l32), close("RE", host(RE), re64, re32), close("KL", host(KL), kl64, kl32)]
    named = dict(model.named_parameters())
    assert set(named) == set(g64)
    for n, p in named.items():
        assert p.grad is not None, n
        res.append(close("grad " + n, host(p.grad), g64[n], g32[n]))
    assert_all(res)


def test_model_decoder_is_causal(model_case):
    """changing x at flat pixels >= 400 leaves the means of pixels <= 400 bit-equal"""
    c = model_case
    model = c["model"]
    rs = np.random.RandomState(275)
    z1, z2 = dev(rs.randn(B_MODEL, 40).astype(np.float32)), dev(rs.randn(B_MODEL, 40).astype(np.float32))
    x = dev(c["x"])
    x2 = x.clone()
    x2[:, 400:] = 1.0 - x2[:, 400:]
    with torch.no_grad():
        m1, lv = model.p_x(z1, z2, x=x)
        m2, _ = model.p_x(z1, z2, x=x2)
    assert lv == 0. and m1.shape == (B_MODEL, 784)
    assert torch.equal(m1[:, :401], m2[:, :401]) and not torch.equal(m1[:, 401:], m2[:, 401:])


def _decoder_mean_ref(sd, dtype, x, z1, z2):
    """psr.pixelcnn_decoder_mean on whole 28-row images x [B, 784] -> [B, 784] (numpy)"""
    s = {k: v.to(dtype).clone() for k, v in sd.items()}
    with torch.no_grad():
        return psr.pixelcnn_decoder_mean(s, torch.from_numpy(x).to(dtype).view(-1, 1, 28, 28), torch.from_numpy(z1).to(dtype),
                                         torch.from_numpy(z2).to(dtype)).numpy()


@pytest.fixture(scope="module")
def decoder_case(model_case):
    """fixed z1, z2 and a binary x for the decoder alone; the restatement's means on the WHOLE image in float64 and float32"""
    rs = np.random.RandomState(281)
    z1, z2 = rs.randn(B_MODEL, 40).astype(np.float32), rs.randn(B_MODEL, 40).astype(np.float32)
    x = gi.binary_images(282, B_MODEL)
    mean64, mean32 = (_decoder_mean_ref(model_case["sd"], dt, x, z1, z2) for dt in (torch.float64, torch.float32))
    return dict(z1=z1, z2=z2, x=x, mean64=mean64, mean32=mean32)


# B = 1 with one and two rows: 28 and 56 pixel rows, less than any GEMM tile
@pytest.mark.parametrize("B,r", [(2, 1), (2, 2), (2, 3), (2, 14), (2, 27), (2, 28), (1, 1), (1, 2)])
def test_truncated_decoder_matches_full_height_ref(model_case, decoder_case, B, r):
    """the pass pixelcnn_generate runs for a pixel of row r - 1 -- the decoder on the first r rows -- against rows < r of the
    restatement on all 28 rows (not bit-equal to a full pass of the kernels: another geometry may sum in another order)"""
    model, d = model_case["model"], decoder_case
    x = dev(d["x"][:B]).view(B, 1, 28, 28)
    with torch.no_grad():
        latent = model._decoder_images(dev(d["z1"][:B]), dev(d["z2"][:B]))
        got = model.p_x_mean(model.pixelcnn(torch.cat((x[:, :, :r], latent[:, :, :r]), 1)))
    assert got.shape == (B, 1, r, 28)
    rows = lambda m: m.reshape(B_MODEL, 1, 28, 28)[:B, :, :r]
    assert_all([close("decoder on %d of 28 rows, B = %d" % (r, B), host(got), rows(d["mean64"]), rows(d["mean32"]))])


GENERATION_SEED = 284


def test_generation_is_consistent_with_its_draws(model_case, monkeypatch):
    """pixelcnn_generate with torch.bernoulli replaced by thresholds against a fixed table u [B, 784]: the probability it thresholds
    at call t and the means it returns are the restatement's, teacher-forced in ONE full-height pass on the pixels it drew -- so
    every truncated pass saw exactly the draws before it, in raster order -- and every drawn pixel is (u < mean)."""
    model, D = model_case["model"], 784
    rs = np.random.RandomState(283)
    z1, z2 = rs.randn(B_MODEL, 40).astype(np.float32), rs.randn(B_MODEL, 40).astype(np.float32)
    u = np.random.RandomState(GENERATION_SEED).rand(B_MODEL, D).astype(np.float32)
    u_dev = dev(u)
    probs, draws, calls = [], [], [0]

    def threshold(p, *args, **kwargs):
        t = calls[0]
        calls[0] += 1
        if t >= D or args or kwargs or p.numel() != B_MODEL:
            probs.append(None)
            return torch.zeros_like(p)
        probs.append(p.detach().clone().reshape(B_MODEL))
        draws.append((u_dev[:, t].view_as(p) < p).float())
        return draws[-1].clone()

    monkeypatch.setattr(torch, "bernoulli", threshold)
    out = model.pixelcnn_generate(dev(z1), dev(z2))
    monkeypatch.undo()
    assert calls[0] == D and all(p is not None for p in probs)           # one draw per pixel, each from B probabilities
    assert out.shape == (B_MODEL, D) and bool(((out > 0) & (out < 1)).all())
    x_drawn = host(torch.stack([d.reshape(B_MODEL) for d in draws], dim=1))
    p_used = host(torch.stack(probs, dim=1))
    assert set(np.unique(x_drawn)) <= {0.0, 1.0} and 0 < x_drawn.mean() < 1
    mean64, mean32 = (_decoder_mean_ref(model_case["sd"], dt, x_drawn, z1, z2) for dt in (torch.float64, torch.float32))
    res = [close("generate: means returned", host(out), mean64, mean32),
           close("generate: probability thresholded at each of the 784 calls", p_used, mean64, mean32)]
    assert_all(res)
    _, err, yard, ulp = res[1][1]
    bar, gap = 4.0 * yard + ulp, np.abs(u.astype(np.float64) - mean64).min()
    print("generate: smallest |u - mean64| %.3e = %.1f x the bar %.3e" % (gap, gap / bar, bar))
    assert gap > 8.0 * bar                                               # (input condition: no threshold within reach of the error)
    assert np.array_equal(x_drawn, (u.astype(np.float64) < mean64).astype(np.float32))


def test_reconstruct_x_generates_from_the_posterior_sample(model_case):
    """reconstruct_x hands pixelcnn_generate the z1 and z2 that forward() sampled for the injected noise, and returns its result"""
    c = model_case
    model = c["model"]
    draws = iter([dev(e) for e in c["eps"]])
    seen = []
    model._draw_eps = lambda like: next(draws)
    model.pixelcnn_generate = lambda z1, z2: seen.append((z1, z2)) or "generated"
    try:
        with torch.no_grad():
            got = model.reconstruct_x(dev(c["x"]))
    finally:
        del model._draw_eps, model.pixelcnn_generate
    assert got == "generated" and len(seen) == 1 and next(draws, None) is None

    def ref(dtype):
        s = {k: v.to(dtype).clone() for k, v in c["sd"].items()}
        eps2, eps1 = (torch.from_numpy(e).to(dtype) for e in c["eps"])
        with torch.no_grad():
            lat = psr.pixelcnn_posterior(s, torch.from_numpy(c["x"]).to(dtype).view(-1, 1, 28, 28), eps2, eps1)
        return lat[0].numpy(), lat[3].numpy()

    (z1_64, z2_64), (z1_32, z2_32) = ref(torch.float64), ref(torch.float32)
    assert_all([close("reconstruct_x: z1", host(seen[0][0]), z1_64, z1_32), close("reconstruct_x: z2", host(seen[0][1]), z2_64, z2_32)])


# ---- the IWAE estimate: calls of IWAE_CHUNK_ROWS rows ----------------------------------------------------------------------
def test_iwae_chunks_match_ref(model_case, monkeypatch):
    """two images x S = 3 in calls of 4 rows (a full chunk and a ragged one of 2) and in one call: the per-row losses and the
    estimate against the restatement on all six rows, the noise served row by row from two fixed tables"""
    import models.PixelCNN as pixelcnn_module
    from utils.evaluation import calculate_likelihood
    c = model_case
    model, args, S = c["model"], c["args"], 3
    assert type(model).__module__ == pixelcnn_module.__name__ and pixelcnn_module.IWAE_CHUNK_ROWS == 100
    n_rows = B_MODEL * S
    rs = np.random.RandomState(285)
    tables = [rs.randn(n_rows, 40).astype(np.float32) for _ in range(2)]            # eps2, eps1
    tables_dev = [dev(t) for t in tables]
    xs = np.repeat(c["x"], S, axis=0)

    def ref(dtype):
        s = {k: v.to(dtype).clone() for k, v in c["sd"].items()}
        with torch.no_grad():
            loss = psr.pixelcnn_loss(s, *(torch.from_numpy(a).to(dtype) for a in (xs, tables[0], tables[1], c["ex"])))[0]
            est = -(torch.logsumexp(-loss.view(B_MODEL, S), 1) - math.log(S)).mean()
        return loss.numpy(), np.array([est.item()], dtype=loss.numpy().dtype)

    (rows64, est64), (rows32, est32) = ref(torch.float64), ref(torch.float32)

    def served():
        """a noise hook over the two tables: every calculate_loss call draws z2's noise, then z1's, for its own rows"""
        cursor, n_calls = [0, 0], [0]

        def draw(like):
            which = n_calls[0] % 2
            n_calls[0] += 1
            lo, hi = cursor[which], cursor[which] + like.shape[0]
            assert hi <= n_rows and tuple(like.shape[1:]) == (40,), (which, lo, like.shape)
            cursor[which] = hi
            return tables_dev[which][lo:hi]
        return draw, cursor

    def run(fn):
        draw, cursor = served()
        model._draw_eps = draw
        try:
            with torch.no_grad():
                out = fn()
        finally:
            del model._draw_eps
        assert cursor == [n_rows, n_rows]                                # both tables consumed, exactly once
        return out

    with torch.no_grad():
        centres, logvar = model.q_z(dev(c["ex"]), prior=True)
    emb = (centres, logvar, torch.arange(C_MODEL, device="cuda"))
    x = dev(c["x"])
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(torch.from_numpy(c["x"]), torch.arange(B_MODEL)), batch_size=B_MODEL)
    whole = host(run(lambda: model.importance_sample_losses(x, S, emb)))
    monkeypatch.setattr(pixelcnn_module, "IWAE_CHUNK_ROWS", 4)
    chunked = host(run(lambda: model.importance_sample_losses(x, S, emb)))
    estimate = run(lambda: calculate_likelihood(args, model, loader, S=S, exemplars_embedding=emb))
    res = [close("IWAE rows, calls of 4 + 2", chunked, rows64, rows32), close("IWAE rows, one call", whole, rows64, rows32),
           close("IWAE estimate, calls of 4 + 2", np.array([estimate]), est64, est32)]
    _, _, yard, ulp = res[0][1]
    apart = np.abs(chunked.astype(np.float64) - whole).max()
    print("IWAE rows, chunked against one call: %.3e apart, bar %.3e" % (apart, 4.0 * yard + ulp))
    assert_all(res)
    assert apart <= 4.0 * yard + ulp


def test_model_evaluation_entry_points_run(model_case):
    from utils.evaluation import calculate_likelihood, evaluate_loss
    c = model_case
    model, args = c["model"], c["args"]
    train = torch.utils.data.TensorDataset(torch.from_numpy(c["ex"]), torch.arange(C_MODEL))
    test = torch.utils.data.TensorDataset(torch.from_numpy(c["x"]), torch.arange(B_MODEL))
    loader = torch.utils.data.DataLoader(test, batch_size=B_MODEL)
    with torch.no_grad():
        elbo, re, kl = evaluate_loss(args, model, loader, dataset=train)
        centres, logvar = model.cache_z(train)
        ll = calculate_likelihood(args, model, loader, S=3, exemplars_embedding=(centres, logvar, torch.arange(C_MODEL)))
        gen = model.reference_based_generation_x(N=1, reference_image=torch.from_numpy(c["ex"][:1]))
    assert np.isfinite([elbo, re, kl, ll]).all() and abs(elbo - (re + kl)) < 1e-3 * abs(elbo)
    assert gen.shape == (1, 784) and bool(((gen > 0) & (gen < 1)).all())


def test_train_one_epoch_moves_every_parameter():
    from utils.optimizer import AdamNormGrad
    from utils.training import train_one_epoch
    from utils.utils import importing_model
    N, B = 32, 8
    args = smoke_case.vae_args(model_name="pixelcnn", number_components=16, training_set_size=N, batch_size=B, warmup=2)
    torch.manual_seed(279)
    model = importing_model(args)(args).cuda()
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    ds = torch.utils.data.TensorDataset(torch.from_numpy(gi.binary_images(280, N)), torch.arange(N).reshape(-1, 1), torch.arange(N) % 10)
    loader = torch.utils.data.DataLoader(ds, batch_size=B, shuffle=False)
    opt = AdamNormGrad(model.parameters(), lr=5e-4)
    loss, re, kl = train_one_epoch(1, args, loader, model, opt)
    assert np.isfinite([loss, re, kl]).all()
    for k, v in model.named_parameters():
        assert bool(torch.isfinite(v).all()), k
        assert not torch.equal(v, before[k]), k
