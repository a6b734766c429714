"""Row losses, the ELBO assembly and the small element-wise kernels of csrc/evae_loss.hip at the shapes where they can go wrong:
partly filled last blocks (the row kernels run 4 rows = waves per block), row lengths around the 64-lane stride, batch sizes
around the 256-thread stride of the one-block reductions, float4 bodies with scalar tails -- and at the boundary values of the
Bernoulli clamp and of the Hardtanh on the log-variance.

The reference is torch autograd in float64 on the CPU, built from the ops the reference project uses (torch.clamp, F.hardtanh,
F.elu), so the boundary semantics (clamp passes its gradient AT the bounds, Hardtanh does not) are torch's.  Inputs are the
float32 values promoted; the clamp bounds are the float32 roundings of 1e-5 and 1 - 1e-5.  The bars are those of
test_reparam_logq_and_densities, test_elbo_function_and_its_gradients and
test_fused_elementwise_backward_launches_match_their_parts (tests/test_gpu_kernels.py) for the same quantities; wherever the
reference gradient is exactly 0 (clipped entries) the device's must be exactly 0 too.

Run on a real MI355X:  python -m pytest tests -m gpu"""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

LOG2PI = math.log(2.0 * math.pi)
LO, HI = -6.0, 2.0
MIN_EPS, MAX_EPS = np.float32(1e-5), np.float32(1.0) - np.float32(1e-5)
f32 = np.float32
up, down = lambda v: np.nextafter(f32(v), f32(np.inf)), lambda v: np.nextafter(f32(v), f32(-np.inf))
# Bernoulli means on, and one float32 either side of, the clamp bounds, and the two ends of [0, 1]
MEAN_EDGES = np.array([0.0, down(MIN_EPS), MIN_EPS, up(MIN_EPS), down(MAX_EPS), MAX_EPS, up(MAX_EPS), 1.0], dtype=np.float32)
# Hardtanh pre-activations on, and one float32 inside and outside, its bounds
PRE_EDGES = np.array([LO, down(LO), up(LO), HI, down(HI), up(HI)], dtype=np.float32)

# (rows, row length): rows 1, 3, 5 leave the 4-row block partly filled, 257 = 64 full blocks and one row; lengths 1, 63, 64, 65,
# 130 = below, at, above one pass of the 64 lanes and a third pass that is partly used
LATENT_SHAPES = [(1, 130), (3, 1), (5, 64), (257, 1), (257, 65), (3, 63), (5, 130), (1, 64), (257, 63)]
PIXEL_SHAPES = LATENT_SHAPES + [(3, 783), (257, 783)]


@pytest.fixture(scope="module")
def lib():
    from evae import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def ops():
    from evae import ops as o
    o._lib.load()
    return o


def vp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ok(rc, what):
    from evae import _lib
    _lib.check(rc, what)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rel(a, b):
    a = np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, np.float64)
    b = np.asarray(b.detach().cpu().numpy() if torch.is_tensor(b) else b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def same_zeros(a, b):
    """the device's exact zeros are the reference's exact zeros"""
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else a
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else b
    return np.array_equal(a == 0, b == 0)


def scatter(flat, values):
    """values at evenly spread positions of the flattened array (all over the rows and the lanes); a short array takes the first
    of them.  Returns the positions."""
    n = flat.size
    pos = np.unique(np.linspace(0, n - 1, len(values)).astype(np.int64)) if n >= len(values) else np.arange(n)
    flat[pos] = values[:pos.size]
    return pos


def leaf64(a):
    return torch.from_numpy(np.asarray(a, np.float64)).requires_grad_()


def c64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


# ------------------------------------------------------------------------------------------------ latent rows
def _latent_case(B, zd):
    rs = np.random.RandomState(1000 * B + zd)
    r = lambda *s: rs.standard_normal(s).astype(np.float32)
    mu, eps, x, dz, dz2 = r(B, zd), r(B, zd), r(B, zd), r(B, zd), r(B, zd)
    gq = (rs.uniform(0.5, 1.5, B) * rs.choice([-1.0, 1.0], B)).astype(np.float32)          # nonzero: no accidental zero gradient
    pre = rs.uniform(-8.0, 4.0, (B, zd)).astype(np.float32)                              # part of it outside Hardtanh(-6, 2)
    scatter(pre.reshape(-1), PRE_EDGES)
    lv = np.clip(pre, f32(LO), f32(HI))                                                  # so logvar holds both ends of [-6, 2]
    return dict(mu=mu, eps=eps, x=x, dz=dz, dz2=dz2, gq=gq, pre=pre, lv=lv)


def _ref_log_normal(x, mu, lv):
    return (-0.5 * (lv + LOG2PI + (x - mu) ** 2 / torch.exp(lv))).sum(1)


@pytest.mark.parametrize("B,zd", LATENT_SHAPES)
def test_latent_row_kernels_at_ragged_shapes_and_hardtanh_edges(ops, lib, B, zd):
    c = _latent_case(B, zd)
    d = {k: dev(v) for k, v in c.items()}
    if B * zd >= 6:
        assert (c["pre"] == f32(LO)).any() and (c["pre"] == f32(HI)).any() and (c["lv"] == f32(LO)).any() and (c["lv"] == f32(HI)).any()

    # --- ReparamLogQ: sample, log q and their gradients
    mu_t, lv_t = d["mu"].clone().requires_grad_(), d["lv"].clone().requires_grad_()
    z, logq = ops.ReparamLogQ.apply(mu_t, lv_t, d["eps"])
    ((z * d["dz"]).sum() + (logq * d["gq"]).sum()).backward()
    mu_, lv_ = leaf64(c["mu"]), leaf64(c["lv"])
    z_ = mu_ + c64(c["eps"]) * torch.exp(0.5 * lv_)
    logq_ = _ref_log_normal(z_, mu_, lv_)
    ((z_ * c64(c["dz"])).sum() + (logq_ * c64(c["gq"])).sum()).backward()
    assert rel(z, z_) < 1e-6
    assert rel(logq, logq_) < 1e-5
    assert rel(mu_t.grad, mu_.grad) < 1e-4
    assert rel(lv_t.grad, lv_.grad) < 1e-4

    # --- its backward with the Hardtanh folded in (two upstream gradients of z), alone and as the step's tail launch
    mu_, pre_ = leaf64(c["mu"]), leaf64(c["pre"])
    lvh_ = F.hardtanh(pre_, LO, HI)
    z_ = mu_ + c64(c["eps"]) * torch.exp(0.5 * lvh_)
    ((z_ * (c64(c["dz"]) + c64(c["dz2"]))).sum() + (_ref_log_normal(z_, mu_, lvh_) * c64(c["gq"])).sum()).backward()
    zd_ = z.detach()
    dmu = torch.empty_like(d["mu"]); dpre = torch.empty_like(d["mu"])
    ok(lib.evae_reparam_logq_bwd_hardtanh(vp(d["mu"]), vp(d["lv"]), vp(d["eps"]), vp(zd_), vp(d["dz"]), vp(d["dz2"]), vp(d["gq"]),
                                          vp(d["pre"]), LO, HI, B, zd, vp(dmu), vp(dpre), st()), "reparam_logq_bwd_hardtanh")
    assert rel(dmu, mu_.grad) < 1e-4
    assert rel(dpre, pre_.grad) < 1e-4
    assert same_zeros(dpre, pre_.grad)
    dmu2 = torch.full_like(d["mu"], float("nan")); dpre2 = torch.full_like(d["mu"], float("nan"))
    ok(lib.evae_reparam_logq_bwd_hardtanh_tail(vp(d["mu"]), vp(d["lv"]), vp(d["eps"]), vp(zd_), vp(d["dz"]), vp(d["dz2"]), vp(d["gq"]),
                                               vp(d["pre"]), LO, HI, B, zd, vp(dmu2), vp(dpre2), None, None, None, None, 0.0, None, None,
                                               None, None, 0, None, st()), "reparam_logq_bwd_hardtanh_tail")
    assert torch.equal(dmu2, dmu) and torch.equal(dpre2, dpre)

    # --- LogNormalDiag and its gradients
    leaves = [d[k].clone().requires_grad_() for k in ("x", "mu", "lv")]
    out = ops.LogNormalDiag.apply(*leaves)
    (out * d["gq"]).sum().backward()
    ref = [leaf64(c[k]) for k in ("x", "mu", "lv")]
    out_ = _ref_log_normal(*ref)
    (out_ * c64(c["gq"])).sum().backward()
    assert rel(out, out_) < 1e-5
    for a, b in zip(leaves, ref):
        assert rel(a.grad, b.grad) < 1e-5

    # --- its backward with the Hardtanh folded in
    x_, mu_, pre_ = leaf64(c["x"]), leaf64(c["mu"]), leaf64(c["pre"])
    (_ref_log_normal(x_, mu_, F.hardtanh(pre_, LO, HI)) * c64(c["gq"])).sum().backward()
    dx = torch.empty_like(d["mu"]); dmu = torch.empty_like(d["mu"]); dpre = torch.empty_like(d["mu"])
    ok(lib.evae_log_normal_diag_bwd_hardtanh(vp(d["x"]), vp(d["mu"]), vp(d["lv"]), vp(d["pre"]), LO, HI, vp(d["gq"]), B, zd, vp(dx),
                                             vp(dmu), vp(dpre), st()), "log_normal_diag_bwd_hardtanh")
    assert rel(dx, x_.grad) < 1e-5 and rel(dmu, mu_.grad) < 1e-5 and rel(dpre, pre_.grad) < 1e-5
    assert same_zeros(dpre, pre_.grad)

    # --- the standard normal's density and its gradient
    xt = d["x"].clone().requires_grad_()
    out = ops.LogNormalStandard.apply(xt)
    (out * d["gq"]).sum().backward()
    x_ = leaf64(c["x"])
    out_ = (-0.5 * (LOG2PI + x_ ** 2)).sum(1)
    (out_ * c64(c["gq"])).sum().backward()
    assert rel(out, out_) < 1e-5
    assert rel(xt.grad, x_.grad) < 1e-5


# ------------------------------------------------------------------------------------------------ pixel rows
def _pixel_case(B, D):
    rs = np.random.RandomState(2000 * B + D)
    mean = (1.0 / (1.0 + np.exp(-rs.standard_normal((B, D)) * 8.0))).astype(np.float32)    # saturates: the clamp region is hit
    x = (rs.random_sample((B, D)) < 0.3).astype(np.float32)
    # every edge value once under x = 0 and once under x = 1
    pos = scatter(mean.reshape(-1), np.concatenate([MEAN_EDGES, MEAN_EDGES]))
    x.reshape(-1)[pos] = (np.arange(pos.size) >= 8).astype(np.float32) if pos.size == 16 else (np.arange(pos.size) % 2).astype(np.float32)
    gq = (rs.uniform(0.5, 1.5, B) * rs.choice([-1.0, 1.0], B)).astype(np.float32)
    return x, mean, gq


def _ref_bernoulli(x, mean_leaf):
    p = torch.clamp(mean_leaf, float(MIN_EPS), float(MAX_EPS))
    return (c64(x) * torch.log(p) + (1.0 - c64(x)) * torch.log(1.0 - p)).sum(1)


@pytest.mark.parametrize("B,D", PIXEL_SHAPES)
def test_bernoulli_row_kernels_at_ragged_shapes_and_clamp_edges(ops, lib, B, D):
    x, mean, gq = _pixel_case(B, D)
    if B * D >= 16:
        for e in MEAN_EDGES:
            assert ((mean == e) & (x == 0)).any() and ((mean == e) & (x == 1)).any()
    xd, md, gd = dev(x), dev(mean), dev(gq)
    m_ = leaf64(mean)
    re_ = _ref_bernoulli(x, m_)
    (re_ * c64(gq)).sum().backward()
    mt = md.clone().requires_grad_()
    re = ops.BernoulliLL.apply(xd, mt)
    (re * gd).sum().backward()
    assert rel(re, re_) < 1e-5
    assert rel(mt.grad, m_.grad) < 1e-5
    assert same_zeros(mt.grad, m_.grad)
    # through the sigmoid that made `mean`: d/dpre = d/dmean * mean (1 - mean), the mean itself being the kernel's input
    dpre_ = m_.grad * c64(mean) * (1.0 - c64(mean))
    dpre = torch.empty_like(md)
    ok(lib.evae_bernoulli_sigmoid_bwd(vp(xd), vp(md), vp(gd), B, D, vp(dpre), st()), "bernoulli_sigmoid_bwd")
    assert rel(dpre, dpre_) < 1e-5
    assert same_zeros(dpre, dpre_)

    # --- the step's one launch: RE, the unit upstream's coefficients and the head's gradient
    beta = 0.37
    m_ = leaf64(mean)
    re_ = _ref_bernoulli(x, m_)
    (re_ * (-1.0 / B)).sum().backward()                                   # loss = mean(beta KL - RE): d loss / d RE_b = -1 / B
    dpre_ = m_.grad * c64(mean) * (1.0 - c64(mean))
    one = torch.ones(1, device="cuda")
    parts = [torch.empty(B, device="cuda") for _ in range(4)] + [torch.empty_like(md)]
    ok(lib.evae_bernoulli_ll_fwd(vp(xd), vp(md), B, D, vp(parts[0]), st()), "bernoulli_ll_fwd")
    ok(lib.evae_elbo_bwd(vp(one), 1, None, 0, None, 0, None, beta, B, vp(parts[1]), vp(parts[2]), vp(parts[3]), st()), "elbo_bwd")
    ok(lib.evae_bernoulli_sigmoid_bwd(vp(xd), vp(md), vp(parts[1]), B, D, vp(parts[4]), st()), "bernoulli_sigmoid_bwd")
    for beta_dev in (None, torch.tensor([beta], device="cuda")):
        fused = [torch.full((B,), float("nan"), device="cuda") for _ in range(4)] + [torch.full_like(md, float("nan"))]
        ok(lib.evae_bernoulli_unit_step(vp(xd), vp(md), B, D, vp(beta_dev), 0.0 if beta_dev is not None else beta, *[vp(t) for t in fused],
                                        st()), "bernoulli_unit_step")
        for name, a, b in zip(("RE", "cRE", "cKL", "neg_cKL", "dpre"), fused, parts):
            assert torch.equal(a, b), (name, beta_dev is not None)
        assert rel(fused[0], re_) < 1e-5
        assert rel(fused[1], np.full(B, -1.0 / B)) < 1e-6
        assert rel(fused[2], np.full(B, f32(beta).astype(np.float64) / B)) < 1e-6
        assert rel(fused[3], np.full(B, -f32(beta).astype(np.float64) / B)) < 1e-6
        assert rel(fused[4], dpre_) < 1e-5
        assert same_zeros(fused[4], dpre_)


# ------------------------------------------------------------------------------------------------ ELBO rows
def _elbo_inputs(B, seed):
    """Magnitudes of a training step (RE ~ -90, log q ~ -40, log p ~ -45) and upstream gradients of one sign and distinct sizes:
    rel() of a batch mean, or of the one row of B = 1, measures the kernel only while that number is not a cancellation of
    its terms (KL = 5 +- 1.4 per layer, loss ~ 92, d/dRE = gr - gl with gr >= 2 gl)."""
    rs = np.random.RandomState(seed)
    ins = [rs.normal(m, s, B).astype(np.float32) for m, s in ((-90.0, 5.0), (-40.0, 1.0), (-45.0, 1.0), (-20.0, 1.0), (-25.0, 1.0))]
    return rs, ins


@pytest.mark.parametrize("B", [1, 63, 64, 65, 255, 256, 257, 1000])
@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("average", [False, True])
def test_elbo_at_batch_sizes_around_the_block_stride(ops, B, two, average):
    rs, ins = _elbo_inputs(B, 3000 + B)
    shape = () if average else (B,)
    ups = [rs.uniform(lo, lo + 0.5, shape).astype(np.float32) for lo in (0.5, 2.0, 0.5)]
    for beta in (0.37, torch.tensor([0.37], device="cuda")):
        leaves = [dev(a).requires_grad_() for a in ins]
        RE, q1, p1, q2, p2 = leaves
        loss, RE_o, KL = ops.elbo(RE, q1, p1, beta, average, q2 if two else None, p2 if two else None)
        sum((o * dev(u)).sum() for o, u in zip((loss, RE_o, KL), ups)).backward()
        ref = [leaf64(a) for a in ins]
        RE_, q1_, p1_, q2_, p2_ = ref
        KL_ = (q1_ - p1_) + (q2_ - p2_) if two else q1_ - p1_
        loss_ = -RE_ + float(f32(0.37)) * KL_
        outs_ = (loss_.mean(), RE_.mean(), KL_.mean()) if average else (loss_, RE_, KL_)
        sum((o * c64(u)).sum() for o, u in zip(outs_, ups)).backward()
        for a, b in zip((loss, RE_o, KL), outs_):
            assert rel(a, b) < 1e-6
        for i, (a, b) in enumerate(zip(leaves, ref)):
            if i >= 3 and not two:
                assert a.grad is None
            else:
                assert rel(a.grad, b.grad) < 1e-6, i


@pytest.mark.parametrize("B,sum_n", [(127, 1), (128, 63), (129, 65), (300, 200)])
def test_assembly_block_of_the_latent_backward_launch(lib, B, sum_n):
    """evae_reparam_logq_bwd_hardtanh_tail's last block: the ELBO rows over 128 threads (B around that stride) and the sum of a
    short row in the block's last wave, beside the element-wise blocks."""
    zd = 40
    c = _latent_case(B, zd)
    d = {k: dev(v) for k, v in c.items()}
    rs, (RE, lq, lp, _, _) = _elbo_inputs(B, 4000 + B)
    src = rs.standard_normal(sum_n).astype(np.float32)
    z = d["mu"] + d["eps"] * torch.exp(0.5 * d["lv"])
    want_dmu = torch.empty_like(z); want_dpre = torch.empty_like(z)
    ok(lib.evae_reparam_logq_bwd_hardtanh(vp(d["mu"]), vp(d["lv"]), vp(d["eps"]), vp(z), vp(d["dz"]), vp(d["dz2"]), vp(d["gq"]),
                                          vp(d["pre"]), LO, HI, B, zd, vp(want_dmu), vp(want_dpre), st()), "reparam_logq_bwd_hardtanh")
    srcd, lpd, REd, lqd = dev(src), dev(lp), dev(RE), dev(lq)
    want_sum = torch.empty(1, device="cuda")
    ok(lib.evae_sum_small(vp(srcd), sum_n, vp(want_sum), st()), "sum_small")
    beta32 = float(f32(0.37))
    KL_ = c64(lq) - c64(lp)
    loss_ = beta32 * KL_ - c64(RE)
    means_ = torch.stack([loss_.mean(), c64(RE).mean(), KL_.mean()])
    for beta_dev in (None, torch.tensor([0.37], device="cuda")):
        for want_means in (True, False):
            nan = lambda *s: torch.full(s, float("nan"), device="cuda")
            dmu, dpre, loss, KL, means, total = nan(B, zd), nan(B, zd), nan(B + 3), nan(B + 3), nan(3), nan(2)
            ok(lib.evae_reparam_logq_bwd_hardtanh_tail(vp(d["mu"]), vp(d["lv"]), vp(d["eps"]), vp(z), vp(d["dz"]), vp(d["dz2"]), vp(d["gq"]),
                                                       vp(d["pre"]), LO, HI, B, zd, vp(dmu), vp(dpre), vp(lpd), vp(REd), vp(lqd),
                                                       vp(beta_dev), 0.0 if beta_dev is not None else 0.37, vp(loss), vp(KL),
                                                       vp(means) if want_means else None, vp(srcd), sum_n, vp(total), st()), "tail")
            assert torch.equal(dmu, want_dmu) and torch.equal(dpre, want_dpre)
            assert rel(loss[:B], loss_) < 1e-6 and rel(KL[:B], KL_) < 1e-6
            assert bool(torch.isnan(loss[B:]).all()) and bool(torch.isnan(KL[B:]).all()) and bool(torch.isnan(total[1:]).all())
            if want_means:
                assert rel(means, means_) < 1e-6
            else:
                assert bool(torch.isnan(means).all())
            assert torch.equal(total[:1], want_sum)                       # evae_sum_small's order, so its very sum
            assert _sum_within_bound(float(total[0]), src)


# ------------------------------------------------------------------------------------------------ small element-wise kernels
def _sum_within_bound(got, src):
    """one wave's sum: lane i adds elements i, i + 64, ... serially, then six butterfly steps -- at most ceil(n / 64) - 1 + 6
    float32 additions on any element's path, each off by at most 2^-24 of a partial sum that never exceeds sum |x|"""
    n = src.size
    steps = (n + 63) // 64 - 1 + 6
    s64 = src.astype(np.float64)
    return abs(got - s64.sum()) <= steps * 2.0 ** -24 * np.abs(s64).sum() * (1.0 + 1e-6)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_sum_small_and_broadcast_scalar(lib, n):
    rs = np.random.RandomState(5000 + n)
    src = rs.standard_normal(n).astype(np.float32)
    srcd = dev(src)
    out = torch.full((2,), float("nan"), device="cuda")
    ok(lib.evae_sum_small(vp(srcd), n, vp(out), st()), "sum_small")
    assert _sum_within_bound(float(out[0]), src) and bool(torch.isnan(out[1]))
    dst = torch.full((n + 5,), float("nan"), device="cuda")
    val = dev(np.array([-3.25, 9.0], np.float32))
    ok(lib.evae_broadcast_scalar(vp(val), vp(dst), n, st()), "broadcast_scalar")
    assert bool((dst[:n] == -3.25).all()) and bool(torch.isnan(dst[n:]).all())


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1025])
def test_elu_forward_float4_body_and_scalar_tail(lib, n):
    """ELU(x) = x for x > 0, expm1(x) elsewhere.  The positive branch is a copy (exact); the other is one expm1f, which HIP's
    math API lists at 1 ulp -- with the float32 rounding of the float64 reference the bar is 2 ulp = 2^-22 relative."""
    rs = np.random.RandomState(6000 + n)
    x = (rs.standard_normal(n) * 3.0).astype(np.float32)
    special = np.array([0.0, -0.0, 1e-8, -1e-8, -100.0], np.float32)
    # at the head (the float4 body, where there is one) and at the very end (the scalar tail, where there is one)
    k = min(n, special.size)
    x[:k] = special[:k]
    if n >= 2 * special.size:
        x[-special.size:] = special[::-1]
    xd = dev(x)
    buf = torch.full((n + 7,), float("nan"), device="cuda")
    ok(lib.evae_elu_fwd(vp(xd), n, vp(buf), st()), "elu_fwd")
    got = buf[:n].cpu().numpy().astype(np.float64)
    ref = F.elu(c64(x)).numpy()
    assert bool(torch.isnan(buf[n:]).all())
    assert np.array_equal(got[x > 0], ref[x > 0])
    assert np.all(np.abs(got - ref) <= 2.0 ** -22 * np.abs(ref))
    assert np.all(got[x == 0] == 0.0)


def test_step_statistics_over_three_calls(ops):
    """step3 = (loss, -re, kl) of the call, totals3 += step3 in float32, with totals3 and without"""
    rs = np.random.RandomState(7)
    vals = rs.normal(0.0, 50.0, (3, 3)).astype(np.float32)
    step3 = torch.full((4,), float("nan"), device="cuda")
    totals = torch.zeros(4, device="cuda"); totals[3] = float("nan")
    want = np.zeros(3, np.float32)
    for loss, re, kl in vals:
        ops.step_stats_add(dev(np.array([loss])), dev(np.array([re])), dev(np.array([kl])), step3, totals)
        now = np.array([loss, -re, kl], np.float32)
        want = want + now
        assert np.array_equal(step3[:3].cpu().numpy(), now) and bool(torch.isnan(step3[3]))
        assert np.array_equal(totals[:3].cpu().numpy(), want) and bool(torch.isnan(totals[3]))
    before = totals.clone()
    for loss, re, kl in vals:
        ops.step_stats_add(dev(np.array([loss])), dev(np.array([re])), dev(np.array([kl])), step3)
        assert np.array_equal(step3[:3].cpu().numpy(), np.array([loss, -re, kl], np.float32))
    assert torch.equal(totals[:3], before[:3])
