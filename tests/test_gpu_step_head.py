"""The random draws at the head of a training step (csrc/evae_loss.hip: batch_prologue_kernel and batch_prologue_u8_body) against
an independent host generator (tests/philox_ref.py, itself held to Random123's known answers by tests/test_philox_ref_host.py).

The binarised batch and the staging bytes are compared bit for bit: u = (r >> 8) * 2^-24 and p are exact float32 values, so
`u < p` has one answer.  eps goes through logf / sqrtf / sincosf and is compared with a float64 evaluation of the same
float32-rounded radicand and angle under EPS_BAR below.

Run on a real MI355X:  python -m pytest tests -m gpu"""
import numpy as np
import pytest
import torch

import philox_ref as pr

pytestmark = pytest.mark.gpu

# (B, D, zdim): one element; quads that straddle rows with a partly used last quad (21 and 15 elements); odd sizes over
# several rows; more than one block of quads (4 * 1024 / 4 = 1024 image quads = 4 blocks, the eps quads start in a fifth)
SHAPES = [(1, 1, 1), (3, 7, 5), (37, 53, 9), (4, 1024, 64)]
# (seed, step): the low words alone, then the high word of the seed, of the step counter, and of both
SEED_STEPS = [(5, 0), (5, 7), (2 ** 32 + 5, 7), (5, 2 ** 32 + 7), (2 ** 62 + 3, 2 ** 40 + 1)]
TWINS = [((2 ** 32 + 5, 7), (5, 7)), ((5, 2 ** 32 + 7), (5, 7))]       # a high-word case and its low-word twin

# Largest |device eps - float64 reference| measured on an MI355X over every shape and (seed, step) above,
# both prologues (the two agree bit for bit): 3.115e-07.  The bar is four times that, 1.246e-06, the margin for another
# release's logf / sincosf; a wrong draw is off by O(1).
EPS_MEASURED = 3.115e-07
EPS_BAR = 4 * EPS_MEASURED


@pytest.fixture(scope="module")
def ops():
    from evae import ops as o
    o._lib.load()
    return o


def _seed_ctr(seed, step):
    return torch.tensor([seed, step], dtype=torch.int64, device="cuda")


def _indices(rs, N, B):
    """with repeats, and with the store's last row"""
    idx = rs.randint(0, N, B).astype(np.int64)
    idx[0] = N - 1
    if B >= 2:
        idx[B - 1] = N - 1
    if B >= 4:
        idx[2] = idx[1]
    return idx


def _float_store(rs, N, D):
    """[N x D] probabilities; with D >= 4 a column of exactly 0, one of exactly 1 and one of 2^-24 (the smallest nonzero u is
    2^-24: that column is 1 only where u == 0)"""
    data = rs.random_sample((N, D)).astype(np.float32)
    if D >= 4:
        data[:, 0] = 0.0
        data[:, 1] = 1.0
        data[:, 2] = np.float32(2.0 ** -24)
    return data


def _strided(a, pad, fill):
    """a [R x C] as a view of a device buffer with row stride C + pad, the padding columns = fill"""
    R, Cn = a.shape
    buf = torch.full((R, Cn + pad), fill, dtype=torch.from_numpy(a).dtype, device="cuda")
    buf[:, :Cn].copy_(torch.from_numpy(a))
    return buf, buf[:, :Cn]


def _run_float(ops, data_np, idx_np, seed, step, zd, binarize=True):
    """-> x [B x D], eps [B x zd] (numpy); the output's padding columns and the words behind eps are checked here"""
    B, D = idx_np.size, data_np.shape[1]
    _, data = _strided(data_np, 3, 0.5)
    xbuf = torch.full((B, D + 5), float("nan"), device="cuda")
    x = xbuf[:, :D]
    ebuf = torch.full((B * zd + 8,), float("nan"), device="cuda")
    eps = ebuf[:B * zd].view(B, zd)
    assert data.stride(0) > D and x.stride(0) > D
    ops.batch_prologue(data, torch.from_numpy(idx_np).cuda(), binarize, _seed_ctr(seed, step), x, eps)
    torch.cuda.synchronize()
    assert bool(torch.isnan(xbuf[:, D:]).all()), "padding columns of x_out were written"
    assert bool(torch.isnan(ebuf[B * zd:]).all()), "words behind eps_out were written (the unused values of the last quad)"
    return x.cpu().numpy(), eps.cpu().numpy()


def _run_u8(ops, data_np, idx_np, seed, step, zd, binarize):
    """-> x [B x D], stage [B x D] uint8, eps [B x zd] (numpy)"""
    B, D = idx_np.size, data_np.shape[1]
    _, data = _strided(data_np, 3, 77)
    xbuf = torch.full((B, D + 5), float("nan"), device="cuda")
    x = xbuf[:, :D]
    sbuf = torch.full((B, D + 7), 99, dtype=torch.uint8, device="cuda")
    stage = sbuf[:, :D]
    ebuf = torch.full((B * zd + 8,), float("nan"), device="cuda")
    eps = ebuf[:B * zd].view(B, zd)
    assert data.stride(0) > D and x.stride(0) > D and stage.stride(0) > D
    ops.batch_prologue_u8(data, torch.from_numpy(idx_np).cuda(), binarize, _seed_ctr(seed, step), 255.0, x, stage, eps)
    torch.cuda.synchronize()
    assert bool(torch.isnan(xbuf[:, D:]).all()), "padding columns of x_out were written"
    assert bool((sbuf[:, D:] == 99).all()), "padding columns of the staging rows were written"
    assert bool(torch.isnan(ebuf[B * zd:]).all()), "words behind eps_out were written"
    return x.cpu().numpy(), stage.cpu().numpy(), eps.cpu().numpy()


def _check_eps(got, B, zd, seed, step, what):
    ref = pr.eps_draws(B, zd, seed, step)
    assert got.shape == ref.shape and np.isfinite(got).all()
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print("eps %s B=%d zd=%d seed=%d step=%d: max |device - float64 reference| = %.3e" % (what, B, zd, seed, step, err))
    assert err < EPS_BAR, (what, B, zd, seed, step, err)


@pytest.mark.parametrize("B,D,zd", SHAPES)
def test_float_prologue_draws_equal_the_host_generator(ops, B, D, zd):
    rs = np.random.RandomState(100 + B)
    N = B + 3
    data = _float_store(rs, N, D)
    idx = _indices(rs, N, B)
    p = data[idx]
    x0, _ = _run_float(ops, data, idx, 5, 7, zd, binarize=False)
    assert np.array_equal(x0, p)                                          # the gather alone
    out = {}
    for seed, step in SEED_STEPS:
        x, eps = _run_float(ops, data, idx, seed, step, zd)
        out[(seed, step)] = (x, eps)
        assert np.array_equal(x, pr.binarise(p, seed, step)), (seed, step)
        _check_eps(eps, B, zd, seed, step, "float")
        if D >= 4:
            u = pr.image_uniforms(B, D, seed, step)
            assert not x[:, 0].any() and x[:, 1].all() and np.array_equal(x[:, 2] == 1.0, u[:, 2] == 0.0)
    for hi, lo in TWINS:
        # a dropped high word of the seed or of the counter: the draws of (2^32 + a) would be those of a.  eps is continuous
        # (equal by chance: never); a batch of >= 1000 fair-ish bits likewise
        assert not np.array_equal(out[hi][1], out[lo][1]), (hi, lo)
        if B * D >= 1000:
            assert not np.array_equal(out[hi][0], out[lo][0]), (hi, lo)


@pytest.mark.parametrize("binarize", [False, True])
@pytest.mark.parametrize("B,D,zd", SHAPES)
def test_byte_prologue_draws_equal_the_host_generator_and_the_float_prologue(ops, B, D, zd, binarize):
    rs = np.random.RandomState(200 + B)
    N = B + 3
    q = rs.randint(0, 256, (N, D)).astype(np.uint8)
    if D >= 4:
        q[:, 0] = 0
        q[:, 1] = 255
        q[0::2, 3] = 0
        q[1::2, 3] = 255
    idx = _indices(rs, N, B)
    if D >= 4:
        assert (q[idx] == 0).any() and (q[idx] == 255).any()
    as_float = q.astype(np.float32) / np.float32(255.0)                   # IEEE division: what the fp32 dataset holds
    p = as_float[idx]
    for seed, step in SEED_STEPS:
        x, stage, eps = _run_u8(ops, q, idx, seed, step, zd, binarize)
        xf, epsf = _run_float(ops, as_float, idx, seed, step, zd, binarize)
        if binarize:
            assert np.array_equal(x, pr.binarise(p, seed, step)), (seed, step)
            assert np.array_equal(stage, (255 * x).astype(np.uint8)), (seed, step)
            if D >= 4:
                assert not x[:, 0].any() and x[:, 1].all()                # byte 0 never fires, byte 255 (p = 1) always
        else:
            assert np.array_equal(x, p)
            assert np.array_equal(stage, q[idx])
        assert np.array_equal(x, xf), (seed, step)                        # the two prologues: the same batch ...
        assert np.array_equal(eps, epsf), (seed, step)                    # ... and the same eps, bit for bit
        _check_eps(eps, B, zd, seed, step, "byte")
