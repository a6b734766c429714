"""The cached sampler's three kernel instances (1, 2 and 4 images per workgroup, `images_per_block`) and its per-image start
pixels (`start`: image completion) -- csrc/evae_pixel_decode.hip behind evae.ops.pixel_decode -- against the float64 restatement
tests/pixelsnail_ref.py.

Tolerance, wherever values are compared: that of tests/test_gpu_pixelsnail.py::close -- |got - ref64| <= 4 |ref32 - ref64| + one
float32 ulp of the largest magnitude, both as maxima over the tensor, printed before they are asserted.  "Bit-equal" is torch.equal.
The model case is that of tests/test_gpu_pixel_decode.py: torch.manual_seed(271), the pixelcnn model with 6 components, eval mode.

The sampling inputs (SAMPLING_SEEDS and the images in tests/golden/pixel_decode_scale_draws.npz) were chosen on the CPU, not by
the kernel: `python tests/test_gpu_pixel_decode_scale.py` (the package and tests/ on PYTHONPATH) runs the float64 restatement's own ancestral loop on the 9 images for the
seed pairs (383, 384), (385, 386), ... and keeps the first whose smallest |u - mean64| exceeds SEED_ROOM x the bar; it writes the
images that loop drew.  The test recomputes the restatement teacher-forced on those images, asserts the condition (8 x the bar)
and that they are (u < mean64), and only then compares what the kernel drew."""
import os

import numpy as np
import pytest
import torch

import golden_inputs as gi
import pixelsnail_ref as psr
import smoke_case
from test_gpu_pixelsnail import assert_all, close, dev, host

pytestmark = pytest.mark.gpu

D = 784
GS = (1, 2, 4)
B_MAX = 9                                                                  # 2 G + 1 at G = 4
STARTS = (0, 1, 27, 28, 29, 400, 783, 784, -3, 900)
SAMPLING_SEEDS = (383, 384)                                                # (z, u): see the module docstring
SEED_ROOM = 16.0
DRAWS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pixel_decode_scale_draws.npz")


def _batches(G):
    out = []
    for b in (1, G - 1, G, G + 1, 2 * G + 1):
        if b > 0 and b not in out:
            out.append(b)
    return out


FORCED = [(G, B) for G in GS for B in _batches(G)]


def _starts(G):
    """2 G + 1 values of STARTS, neighbours in the list three apart: every workgroup holds a mix, the three G cover all ten"""
    return [STARTS[(3 * k + G) % len(STARTS)] for k in range(2 * G + 1)]


def test_cases_cover_the_block_edges_and_every_start_value():
    assert all(B <= B_MAX for _, B in FORCED) and {B for G, B in FORCED if G == 4} == {1, 3, 4, 5, 9}
    assert {s for G in GS for s in _starts(G)} == set(STARTS)
    assert all(len(set(_starts(G)[:G])) == min(G, len(_starts(G))) for G in GS)


@pytest.fixture(scope="module")
def ops():
    from evae import ops as o
    return o


def _model():
    from utils.utils import importing_model
    args = smoke_case.vae_args(model_name="pixelcnn", number_components=6, training_set_size=6)
    torch.manual_seed(271)
    model = importing_model(args)(args)
    return model, {k: v.clone() for k, v in model.state_dict().items()}


@pytest.fixture(scope="module")
def case(ops):
    """the model, its packed weights, and B_MAX teacher-forced images with their latents (RandomState 381 / 382)"""
    model, sd = _model()
    model.cuda().eval()
    rs = np.random.RandomState(381)
    z1, z2 = rs.randn(B_MAX, 40).astype(np.float32), rs.randn(B_MAX, 40).astype(np.float32)
    x = gi.binary_images(382, B_MAX)
    with torch.no_grad():
        packed = ops.pixel_decode_pack(model.pixelcnn, model.p_x_mean)
        latent = model._decoder_images(dev(z1), dev(z2))
    return dict(model=model, sd=sd, z1=z1, z2=z2, x=x, packed=packed, latent=latent)


def _mean_ref(sd, dtype, x, z1, z2):
    s = {k: v.to(dtype).clone() for k, v in sd.items()}
    with torch.no_grad():
        return psr.pixelcnn_decoder_mean(s, torch.from_numpy(x).to(dtype).view(-1, 1, 28, 28), torch.from_numpy(z1).to(dtype),
                                         torch.from_numpy(z2).to(dtype)).numpy()


@pytest.fixture(scope="module")
def forced_ref(case):
    """the restatement on the B_MAX teacher-forced images, float64 and float32, computed once (images are independent: its first
    B rows are the reference of a launch of B images)"""
    c = case
    return tuple(_mean_ref(c["sd"], dt, c["x"], c["z1"], c["z2"]) for dt in (torch.float64, torch.float32))


def _sampling_inputs(seeds):
    rs = np.random.RandomState(seeds[0])
    z1, z2 = rs.randn(B_MAX, 40).astype(np.float32), rs.randn(B_MAX, 40).astype(np.float32)
    return z1, z2, np.random.RandomState(seeds[1]).rand(B_MAX, D).astype(np.float32)


@pytest.fixture(scope="module")
def sampling_case(case):
    """B_MAX images: the latents and uniforms of SAMPLING_SEEDS, the images the float64 ancestral loop drew from them (golden),
    and the restatement teacher-forced on those images, float64 and float32, computed once"""
    z1, z2, u = _sampling_inputs(SAMPLING_SEEDS)
    with np.load(DRAWS) as f:
        assert tuple(f["seeds"]) == SAMPLING_SEEDS
        x = np.unpackbits(f["x_bits"])[:B_MAX * D].reshape(B_MAX, D).astype(np.float32)
    mean64, mean32 = (_mean_ref(case["sd"], dt, x, z1, z2) for dt in (torch.float64, torch.float32))
    with torch.no_grad():
        latent = case["model"]._decoder_images(dev(z1), dev(z2))
    return dict(z1=z1, z2=z2, u=u, x=x, mean64=mean64, mean32=mean32, latent=latent)


# ---- teacher-forced means ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,B", FORCED)
def test_teacher_forced_means_match_ref_at_every_pixel(ops, case, forced_ref, G, B):
    c = case
    mean64, mean32 = (m[:B] for m in forced_ref)
    x = dev(c["x"][:B])
    mean, x_out, _ = ops.pixel_decode(c["packed"], c["latent"][:B], x, images_per_block=G)
    got = host(mean)
    assert got.shape == (B, D) and bool(((got > 0) & (got < 1)).all())
    img = lambda a: a.reshape(B, 28, 28)
    for tag, sel in (("pixel 0", lambda a: img(a)[:, 0, 0]), ("row 0", lambda a: img(a)[:, 0, :]), ("column 0", lambda a: img(a)[:, :, 0]),
                     ("column 27", lambda a: img(a)[:, :, 27]), ("last pixel", lambda a: img(a)[:, 27, 27])):
        close("teacher-forced G = %d B = %d, %s" % (G, B, tag), sel(got), sel(mean64), sel(mean32))     # printed: a failure names its edge
    assert_all([close("teacher-forced G = %d B = %d, all 784 pixels" % (G, B), got, mean64, mean32)])
    assert torch.equal(x_out, dev(c["x"][:B])) and x_out.data_ptr() == x.data_ptr()
    if G == 1:                                                              # the old entry point: the same bits
        old, _, _ = ops.pixel_decode(c["packed"], c["latent"][:B], x)
        assert ops.pixel_decode_images_per_block() == 1 and torch.equal(old, mean)


# ---- sampling -------------------------------------------------------------------------------------------------------------------
def test_sampling_inputs_keep_every_threshold_out_of_reach(sampling_case):
    """the input condition of the sampling tests, on the CPU restatement alone: min |u - mean64| > 8 x the bar, and the golden
    images are the float64 ancestral draws (u < mean64)"""
    s = sampling_case
    res = close("restatement on the golden draws, float32 against float64", s["mean32"], s["mean64"], s["mean32"])
    _, _, yard, ulp = res[1]
    bar, gap = 4.0 * yard + ulp, np.abs(s["u"].astype(np.float64) - s["mean64"]).min()
    print("sampling: smallest |u - mean64| %.3e = %.1f x the bar %.3e" % (gap, gap / bar, bar))
    assert gap > 8.0 * bar
    assert np.array_equal(s["x"], (s["u"].astype(np.float64) < s["mean64"]).astype(np.float32))
    assert set(np.unique(s["x"])) <= {0.0, 1.0} and 0 < s["x"].mean() < 1


@pytest.mark.parametrize("G", GS)
def test_sampling_is_consistent_with_its_draws(ops, case, sampling_case, G):
    s = sampling_case
    x = torch.zeros(B_MAX, D, device="cuda")
    mean, x, _ = ops.pixel_decode(case["packed"], s["latent"], x, u=dev(s["u"]), images_per_block=G)
    assert_all([close("sampling G = %d: means returned" % G, host(mean), s["mean64"], s["mean32"])])
    assert np.array_equal(host(x), s["x"])                                 # = (u < mean64) exactly, asserted above
    again, x2, _ = ops.pixel_decode(case["packed"], s["latent"], torch.zeros(B_MAX, D, device="cuda"), u=dev(s["u"]), images_per_block=G)
    assert torch.equal(again, mean) and torch.equal(x2, x)                  # runs at one G are bit-identical


# ---- start pixels ---------------------------------------------------------------------------------------------------------------
def _completion(ops, case, s, G, B, start, ranges=((0, D),)):
    x = dev(case["x"][:B]).clone()
    cache, mean = None, None
    for t0, t1 in ranges:
        mean, x, cache = ops.pixel_decode(case["packed"], s["latent"][:B], x, u=dev(s["u"][:B]), t0=t0, t1=t1, cache=cache, start=start,
                                          images_per_block=G)
    return mean.clone(), x.clone()


@pytest.mark.parametrize("G", GS)
def test_start_pixels_in_one_launch(ops, case, sampling_case, G):
    """x_given = the teacher-forced images of `case`, latents and uniforms of `sampling_case`, 2 G + 1 images"""
    c, s, B = case, sampling_case, 2 * G + 1
    starts = _starts(G)
    given = dev(c["x"][:B])
    dtype = torch.int64 if G == 2 else torch.int32
    mean, x = _completion(ops, c, s, G, B, torch.tensor(starts, dtype=dtype, device="cuda"))
    assert set(np.unique(host(x))) <= {0.0, 1.0}
    for b, st in enumerate(starts):
        k = min(max(st, 0), D)
        assert torch.equal(x[b, :k], given[b, :k]), (b, st)
        # the two-launch form on this image alone, same G: teacher-forced over [0, k), sampling over [k, 784) on the same cache
        xb = given[b:b + 1].clone()
        _, _, cache = ops.pixel_decode(c["packed"], s["latent"][b:b + 1], xb, t0=0, t1=k, images_per_block=G)
        assert torch.equal(xb, given[b:b + 1])
        mb, xb, _ = ops.pixel_decode(c["packed"], s["latent"][b:b + 1], xb, u=dev(s["u"][b:b + 1]), t0=k, t1=D, cache=cache, images_per_block=G)
        assert torch.equal(mb[0], mean[b]) and torch.equal(xb[0], x[b]), (b, st)
        if k <= 400:
            assert not torch.equal(x[b, k:], given[b, k:]), (b, st)         # (it did draw: 784 - k fair coins do not all match)
    # start = 784 for all: the teacher-forced launch, no x written
    forced, _, _ = ops.pixel_decode(c["packed"], s["latent"][:B], given.clone(), images_per_block=G)
    for full in (D, torch.full((B,), D, dtype=torch.int64, device="cuda")):
        m784, x784 = _completion(ops, c, s, G, B, full)
        assert torch.equal(m784, forced) and torch.equal(x784, given)
    # start null: the launch without the argument, and all zeros
    plain, xp, _ = ops.pixel_decode(c["packed"], s["latent"][:B], given.clone(), u=dev(s["u"][:B]), images_per_block=G)
    for none in (None, 0, torch.zeros(B, dtype=torch.int32, device="cuda")):
        m0, x0 = _completion(ops, c, s, G, B, none)
        assert torch.equal(m0, plain) and torch.equal(x0, xp)
    if G == 1:
        old, xo, _ = ops.pixel_decode(c["packed"], s["latent"][:B], given.clone(), u=dev(s["u"][:B]))
        assert torch.equal(old, plain) and torch.equal(xo, xp)


# ---- across G -------------------------------------------------------------------------------------------------------------------
def test_cache_begun_at_one_g_continues_at_another(ops, case, forced_ref):
    c = case
    x = dev(c["x"])
    _, _, cache = ops.pixel_decode(c["packed"], c["latent"], x, t0=0, t1=300, images_per_block=1)
    mean, _, _ = ops.pixel_decode(c["packed"], c["latent"], x, t0=300, t1=D, cache=cache, images_per_block=4)
    assert_all([close("G = 1 over [0, 300), G = 4 over [300, 784)", host(mean), forced_ref[0], forced_ref[1])])
    one, _, _ = ops.pixel_decode(c["packed"], c["latent"], x, images_per_block=1)
    assert torch.equal(mean[:, :300], one[:, :300])


@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("t", (1, 28, 400))
def test_split_launches_with_start_are_bit_equal_to_one(ops, case, sampling_case, G, t):
    B = 2 * G + 1
    start = torch.tensor(_starts(G), dtype=torch.int32, device="cuda")
    one = _completion(ops, case, sampling_case, G, B, start)
    two = _completion(ops, case, sampling_case, G, B, start, ((0, t), (t, t), (t, D)))
    assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1])
    again = _completion(ops, case, sampling_case, G, B, start)
    assert torch.equal(one[0], again[0]) and torch.equal(one[1], again[1])


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(ops, case, sampling_case):
    from evae import _lib
    c, s, B = case, sampling_case, 3
    latent, u = s["latent"][:B], dev(s["u"][:B])
    for bad in (3, 0, 8):
        x = dev(c["x"][:B])
        cache = ops.PixelDecodeCache(B, x.device)
        cache.mean.fill_(-7.0)
        with pytest.raises(_lib.EvaeError, match=r"\b%d images" % bad):
            ops.pixel_decode(c["packed"], latent, x, u=u, cache=cache, images_per_block=bad)
        torch.cuda.synchronize()
        assert torch.equal(x, dev(c["x"][:B])) and bool((cache.mean == -7.0).all()) and not cache.planes.any()      # nothing ran
    with pytest.raises(_lib.EvaeError, match="images_per_block"):
        ops.pixel_decode(c["packed"], latent, dev(c["x"][:B]), images_per_block="most")
    x = dev(c["x"][:B])
    for start in (torch.zeros(B + 1, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32), torch.zeros(B, 1, dtype=torch.int32, device="cuda"),
                  torch.zeros(B, device="cuda")):
        with pytest.raises(_lib.EvaeError, match="start"):
            ops.pixel_decode(c["packed"], latent, x, u=u, start=start)
    assert torch.equal(x, dev(c["x"][:B]))
    assert ops.pixel_decode_choose_images(B) == 1 and ops.pixel_decode_cache_bytes(B) == B * 4 * (cache.planes.shape[1] + D)
    auto, _, _ = ops.pixel_decode(c["packed"], latent, x, images_per_block="auto")
    one, _, _ = ops.pixel_decode(c["packed"], latent, x, images_per_block=1)
    assert torch.equal(auto, one)


# ---- the choice of SAMPLING_SEEDS (CPU; not a test) ----------------------------------------------------------------------------
def _ancestral64(sd, z1, z2, u):
    """the float64 restatement's ancestral loop: pass (i, j) on the rows <= i (the network is causal), x[i, j] = u < mean"""
    s = {k: v.to(torch.float64).clone() for k, v in sd.items()}
    B = z1.shape[0]
    with torch.no_grad():
        lat = torch.cat((psr._gated_dense(s, "p_x_layers_z1.0", torch.from_numpy(z1).double()).view(B, 1, 28, 28),
                         psr._gated_dense(s, "p_x_layers_z2.0", torch.from_numpy(z2).double()).view(B, 1, 28, 28)), 1)
        x = torch.zeros(B, 1, 28, 28, dtype=torch.float64)
        uu = torch.from_numpy(u).double().view(B, 28, 28)
        for i in range(28):
            for j in range(28):
                top = psr.pixelsnail(s, torch.cat((x[:, :, :i + 1], lat[:, :, :i + 1]), 1), 3, 1, 4, prefix="pixelcnn")
                mean = torch.sigmoid(torch.nn.functional.conv2d(top, s["p_x_mean.conv.weight"], s["p_x_mean.conv.bias"]))
                x[:, 0, i, j] = (uu[:, i, j] < mean[:, 0, i, j]).double()
    return x.view(B, D).numpy().astype(np.float32)


def _choose_seeds():
    _, sd = _model()
    seeds = (383, 384)
    while True:
        z1, z2, u = _sampling_inputs(seeds)
        x = _ancestral64(sd, z1, z2, u)
        mean64, mean32 = (_mean_ref(sd, dt, x, z1, z2) for dt in (torch.float64, torch.float32))
        assert np.array_equal(x, (u.astype(np.float64) < mean64).astype(np.float32))
        _, (_, _, yard, ulp) = close("seeds %s" % (seeds,), mean32, mean64, mean32)
        bar, gap = 4.0 * yard + ulp, np.abs(u.astype(np.float64) - mean64).min()
        print("seeds %s: smallest |u - mean64| %.3e = %.1f x the bar %.3e" % (seeds, gap, gap / bar, bar), flush=True)
        if gap > SEED_ROOM * bar:
            np.savez(DRAWS, seeds=np.asarray(seeds), x_bits=np.packbits(x.astype(np.uint8)))
            print("kept %s -> %s" % (seeds, DRAWS))
            return
        seeds = (seeds[0] + 2, seeds[1] + 2)


if __name__ == "__main__":
    _choose_seeds()
