"""The cached ancestral sampler of the `pixelcnn` decoder (csrc/evae_pixel_decode.hip behind evae.ops.pixel_decode, and
args.pixelcnn_sampler = 'cached' in models/PixelCNN.py) against the float64 restatement tests/pixelsnail_ref.py.

Tolerance, wherever values are compared: that of tests/test_gpu_pixelsnail.py::close -- |got - ref64| <= 4 |ref32 - ref64| + one
float32 ulp of the largest magnitude, both as maxima over the tensor, printed before they are asserted.  "Bit-equal" is torch.equal.
The model case is that file's: torch.manual_seed(271), the pixelcnn model with 6 components, eval mode."""
import numpy as np
import pytest
import torch

import golden_inputs as gi
import pixelsnail_ref as psr
import smoke_case
from test_gpu_pixelsnail import assert_all, close, dev, host

pytestmark = pytest.mark.gpu

D = 784
SPLITS = (1, 27, 28, 29, 56, 783)


@pytest.fixture(scope="module")
def ops():
    from evae import ops as o
    return o


@pytest.fixture(scope="module")
def case(ops):
    """the model, its packed weights, and B_MAX = 2 G + 1 teacher-forced images with their latents (RandomState 281 / 282)"""
    from utils.utils import importing_model
    args = smoke_case.vae_args(model_name="pixelcnn", number_components=6, training_set_size=6)
    torch.manual_seed(271)
    model = importing_model(args)(args)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model.cuda().eval()
    G = ops.pixel_decode_images_per_block()
    b_max = 2 * G + 1
    rs = np.random.RandomState(281)
    z1, z2 = rs.randn(b_max, 40).astype(np.float32), rs.randn(b_max, 40).astype(np.float32)
    x = gi.binary_images(282, b_max)
    with torch.no_grad():
        packed = ops.pixel_decode_pack(model.pixelcnn, model.p_x_mean)
        latent = model._decoder_images(dev(z1), dev(z2))
    return dict(model=model, sd=sd, G=G, b_max=b_max, z1=z1, z2=z2, x=x, packed=packed, latent=latent)


def _mean_ref(sd, dtype, x, z1, z2):
    s = {k: v.to(dtype).clone() for k, v in sd.items()}
    with torch.no_grad():
        return psr.pixelcnn_decoder_mean(s, torch.from_numpy(x).to(dtype).view(-1, 1, 28, 28), torch.from_numpy(z1).to(dtype),
                                         torch.from_numpy(z2).to(dtype)).numpy()


@pytest.fixture(scope="module")
def forced_ref(case):
    """the restatement on the B_MAX teacher-forced images, float64 and float32 (computed once; images are independent, so its first
    B rows are the reference of a launch of B images)"""
    c = case
    return tuple(_mean_ref(c["sd"], dt, c["x"], c["z1"], c["z2"]) for dt in (torch.float64, torch.float32))


@pytest.fixture(scope="module")
def sampling_case(case):
    """B = 2, z from RandomState(283), the uniforms of RandomState(284): the latents and the table on the device"""
    rs = np.random.RandomState(283)
    z1, z2 = rs.randn(2, 40).astype(np.float32), rs.randn(2, 40).astype(np.float32)
    u = np.random.RandomState(284).rand(2, D).astype(np.float32)
    with torch.no_grad():
        latent = case["model"]._decoder_images(dev(z1), dev(z2))
    return dict(z1=z1, z2=z2, u=u, latent=latent)


def _batches(G):
    return sorted({b for b in (1, 2, G - 1, G, G + 1, 2 * G + 1) if b > 0})


def test_batch_sizes_cover_the_block_edges(ops):
    G = ops.pixel_decode_images_per_block()
    assert G >= 1 and 2 * G + 1 in _batches(G) and G in _batches(G)


@pytest.mark.parametrize("k", range(6))
def test_teacher_forced_means_match_ref_at_every_pixel(ops, case, forced_ref, k):
    """test 1: u = None, one launch over [0, 784); B in {1, 2, G - 1, G, G + 1, 2 G + 1}"""
    c = case
    sizes = _batches(c["G"])
    if k >= len(sizes):
        return                                                            # (duplicates dropped: fewer than six sizes)
    B = sizes[k]
    mean64, mean32 = (m[:B] for m in forced_ref)
    x = dev(c["x"][:B])
    mean, x_out, _ = ops.pixel_decode(c["packed"], c["latent"][:B], x)
    got = host(mean)
    assert got.shape == (B, D) and bool(((got > 0) & (got < 1)).all())
    img = lambda a: a.reshape(B, 28, 28)
    for tag, sel in (("pixel 0", lambda a: img(a)[:, 0, 0]), ("row 0", lambda a: img(a)[:, 0, :]), ("column 0", lambda a: img(a)[:, :, 0]),
                     ("column 27", lambda a: img(a)[:, :, 27]), ("last pixel", lambda a: img(a)[:, 27, 27])):
        close("teacher-forced B = %d, %s" % (B, tag), sel(got), sel(mean64), sel(mean32))           # printed: a failure names its edge
    assert_all([close("teacher-forced B = %d, all 784 pixels" % B, got, mean64, mean32)])
    # test 2: x is untouched
    assert torch.equal(x_out, dev(c["x"][:B])) and x_out.data_ptr() == x.data_ptr()


def _sample(ops, case, s, ranges=((0, D),)):
    x = torch.zeros(2, D, device="cuda")
    cache, mean = None, None
    for t0, t1 in ranges:
        mean, x, cache = ops.pixel_decode(case["packed"], s["latent"], x, u=dev(s["u"]), t0=t0, t1=t1, cache=cache)
    return mean, x


@pytest.fixture(scope="module")
def sampled(ops, case, sampling_case):
    mean, x = _sample(ops, case, sampling_case)
    return mean.clone(), x.clone()


@pytest.mark.parametrize("t", SPLITS)
def test_split_launches_are_bit_equal_to_one(ops, case, sampling_case, sampled, t):
    """test 3: [0, t) then [t, 784) over one cache, sampling and teacher-forced; t0 == t1 is a no-op"""
    c = case
    mean, x = _sample(ops, c, sampling_case, ((0, t), (t, t), (t, D)))
    assert torch.equal(mean, sampled[0]) and torch.equal(x, sampled[1])
    B = 2
    xf = dev(c["x"][:B])
    one, _, _ = ops.pixel_decode(c["packed"], c["latent"][:B], xf)
    first, _, cache = ops.pixel_decode(c["packed"], c["latent"][:B], xf, t0=0, t1=t)
    assert torch.equal(first[:, :t], one[:, :t]) and not first[:, t:].any()
    before = first.clone()
    same, _, _ = ops.pixel_decode(c["packed"], c["latent"][:B], xf, t0=t, t1=t, cache=cache)
    assert torch.equal(same, before)
    two, _, _ = ops.pixel_decode(c["packed"], c["latent"][:B], xf, t0=t, t1=D, cache=cache)
    assert torch.equal(two, one)


def test_sampling_is_consistent_with_its_draws(case, sampling_case, sampled):
    """test 4: the means returned are the restatement's, teacher-forced on the x the kernel drew, and x = (u < mean64) exactly"""
    s = sampling_case
    mean, x = host(sampled[0]), host(sampled[1])
    assert set(np.unique(x)) <= {0.0, 1.0} and 0 < x.mean() < 1
    mean64, mean32 = (_mean_ref(case["sd"], dt, x, s["z1"], s["z2"]) for dt in (torch.float64, torch.float32))
    res = close("sampling: means returned", mean, mean64, mean32)
    assert_all([res])
    _, err, yard, ulp = res[1]
    bar, gap = 4.0 * yard + ulp, np.abs(s["u"].astype(np.float64) - mean64).min()
    print("sampling: smallest |u - mean64| %.3e = %.1f x the bar %.3e" % (gap, gap / bar, bar))
    assert gap > 8.0 * bar                                                # (input condition: no threshold within reach of the error)
    assert np.array_equal(x, (s["u"].astype(np.float64) < mean64).astype(np.float32))


def test_runs_are_bit_identical(ops, case, sampling_case, sampled):
    """test 5"""
    mean, x = _sample(ops, case, sampling_case)
    assert torch.equal(mean, sampled[0]) and torch.equal(x, sampled[1])
    B = case["b_max"]
    one, _, _ = ops.pixel_decode(case["packed"], case["latent"], dev(case["x"]))
    two, _, _ = ops.pixel_decode(case["packed"], case["latent"], dev(case["x"]))
    assert one.shape == (B, D) and torch.equal(one, two)


def test_teacher_forced_decoder_is_causal(ops, case):
    """test 6: flipping x at flat pixels >= 400 leaves the means of pixels <= 400 bit-equal and changes the later ones"""
    c, B = case, 2
    x = dev(c["x"][:B])
    x2 = x.clone()
    x2[:, 400:] = 1.0 - x2[:, 400:]
    m1, _, _ = ops.pixel_decode(c["packed"], c["latent"][:B], x)
    m2, _, _ = ops.pixel_decode(c["packed"], c["latent"][:B], x2)
    assert torch.equal(m1[:, :401], m2[:, :401]) and not torch.equal(m1[:, 401:], m2[:, 401:])


def test_refusals(ops, case):
    """test 7"""
    from evae import _lib
    c, B = case, 2
    x, latent = dev(c["x"][:B]), c["latent"][:B]
    bad = ops.PixelDecodeWeights(c["packed"].buffer, c["packed"].table, c["packed"].entries)
    bad.table[1] = 32                                                     # channel count of the packed table
    with pytest.raises(_lib.EvaeError, match="channel"):
        ops.pixel_decode(bad, latent, x)
    with pytest.raises(_lib.EvaeError, match="785"):
        ops.pixel_decode(c["packed"], latent, x, t1=785)
    with pytest.raises(_lib.EvaeError, match="range"):
        ops.pixel_decode(c["packed"], latent, x, t0=5, t1=4)
    with pytest.raises(_lib.EvaeError):
        ops.pixel_decode(c["packed"], latent, x.cpu())
    with pytest.raises(_lib.EvaeError):
        ops.pixel_decode(c["packed"], latent.cpu(), x)
    with pytest.raises(_lib.EvaeError, match="grad"):
        ops.pixel_decode(c["packed"], latent.clone().requires_grad_(True), x)
    with torch.no_grad():                                                 # (grad disabled: nothing to refuse)
        ops.pixel_decode(c["packed"], latent.clone().requires_grad_(True), x, t0=0, t1=1)
    mean, x0, cache = ops.pixel_decode(c["packed"], latent[:0], x[:0], u=torch.zeros(0, D, device="cuda"))
    assert mean.shape == (0, D) and x0.shape == (0, D) and cache.planes.shape[0] == 0


def test_cached_sampler_through_the_model(ops, case, sampling_case, sampled, monkeypatch):
    """test 8: args.pixelcnn_sampler = 'cached' in eval mode is one torch.rand and no torch.bernoulli, and returns the kernel's means;
    reconstruct_x and generate_x_from_z reach it; in training mode the same flag runs the 784 passes"""
    model, s = case["model"], sampling_case
    calls = dict(rand=0, bernoulli=0)
    real_bernoulli = torch.bernoulli

    def rand(*size, **kw):
        calls["rand"] += 1
        assert tuple(size) in ((2, D), ((2, D),)) and torch.device(kw.get("device", "cpu")).type == "cuda"
        return dev(s["u"])

    def bernoulli(p, *a, **k):
        calls["bernoulli"] += 1
        return real_bernoulli(p, *a, **k)

    model.args.pixelcnn_sampler = "cached"
    try:
        monkeypatch.setattr(torch, "rand", rand)
        monkeypatch.setattr(torch, "bernoulli", bernoulli)
        out = model.pixelcnn_generate(dev(s["z1"]), dev(s["z2"]))
        assert calls == dict(rand=1, bernoulli=0)
        assert torch.equal(out, sampled[0])
        monkeypatch.undo()

        seen = []
        model.pixelcnn_generate = lambda z1, z2: seen.append((z1, z2)) or "generated"
        try:
            with torch.no_grad():
                assert model.reconstruct_x(dev(case["x"][:2])) == "generated"
                assert model.generate_x_from_z(dev(s["z2"])) == "generated"
        finally:
            del model.pixelcnn_generate
        assert len(seen) == 2 and all(z1.shape == (2, 40) and z2.shape == (2, 40) for z1, z2 in seen)

        # training mode: the flag is ignored, the passes run (one truncated-height decoder pass and one bernoulli call per pixel)
        n = [0]

        def count(p, *a, **k):
            n[0] += 1
            return torch.zeros_like(p)

        monkeypatch.setattr(torch, "bernoulli", count)
        model.train()
        out = model.pixelcnn_generate(dev(s["z1"][:1]), dev(s["z2"][:1]))
        assert n[0] == D and out.shape == (1, D)
    finally:
        monkeypatch.undo()
        model.eval()
        del model.args.pixelcnn_sampler
