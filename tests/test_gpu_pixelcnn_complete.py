"""Image completion and large batches through the model (models/PixelCNN.py: pixelcnn_generate(x_given, given), pixelcnn_complete,
PIXEL_DECODE_CHUNK_IMAGES) against the float64 restatement tests/pixelsnail_ref.py.  Tolerance and model case: those of
tests/test_gpu_pixel_decode.py (tests/test_gpu_pixelsnail.py::close; torch.manual_seed(271), 6 components, eval mode)."""
import numpy as np
import pytest
import torch

import golden_inputs as gi
import pixelsnail_ref as psr
import smoke_case
from test_gpu_pixelsnail import assert_all, close, dev, host

pytestmark = pytest.mark.gpu

D = 784
KEEP_ROWS = (0, 1, 14, 27, 28)


@pytest.fixture(scope="module")
def case():
    from utils.utils import importing_model
    args = smoke_case.vae_args(model_name="pixelcnn", number_components=6, training_set_size=6)
    torch.manual_seed(271)
    model = importing_model(args)(args)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model.cuda().eval()
    return dict(model=model, sd=sd, x=gi.binary_images(482, 7))


@pytest.fixture
def sampler(case):
    """sets args.pixelcnn_sampler for one test"""
    model = case["model"]

    def use(name):
        model.args.pixelcnn_sampler = name
    yield use
    if hasattr(model.args, "pixelcnn_sampler"):
        del model.args.pixelcnn_sampler
    model.eval()


def _record_latents(model, monkeypatch):
    """the (z1, z2) every model.forward call drew, as pixelcnn_complete reads them"""
    seen, real = [], model.forward

    def forward(x):
        out = real(x)
        seen.append((out[2][0].reshape(-1, model.args.z1_size), out[2][3].reshape(-1, model.args.z2_size)))
        return out
    monkeypatch.setattr(model, "forward", forward)
    return seen


def _mean_ref(sd, dtype, x, z1, z2):
    s = {k: v.to(dtype).clone() for k, v in sd.items()}
    with torch.no_grad():
        return psr.pixelcnn_decoder_mean(s, torch.from_numpy(x).to(dtype).view(-1, 1, 28, 28), torch.from_numpy(z1).to(dtype),
                                         torch.from_numpy(z2).to(dtype)).numpy()


def _assert_completion(tag, case, x_in, keep_rows, N, mean, samples, z):
    """kept rows are the input's, the rest is binary, and the means are the restatement's on the returned images"""
    B = x_in.shape[0]
    assert mean.shape == samples.shape == (B * N, D)
    got = host(samples)
    assert set(np.unique(got)) <= {0.0, 1.0}
    for b in range(B):
        for n in range(N):
            k = 28 * keep_rows[b]
            assert np.array_equal(got[b * N + n, :k], x_in[b, :k]), (tag, b, n)
    z1, z2 = (host(t).repeat(N, axis=0) for t in z)
    mean64, mean32 = (_mean_ref(case["sd"], dt, got, z1, z2) for dt in (torch.float64, torch.float32))
    assert_all([close("%s: means on the returned images" % tag, host(mean), mean64, mean32)])


def test_complete_keeps_the_given_rows_cached(case, sampler, monkeypatch):
    model, x_in, N = case["model"], case["x"][:5], 2
    sampler("cached")
    seen = _record_latents(model, monkeypatch)
    torch.manual_seed(11)
    mean, samples = model.pixelcnn_complete(dev(x_in), KEEP_ROWS, N=N, return_samples=True)
    assert len(seen) == 1
    _assert_completion("complete, cached", case, x_in, KEEP_ROWS, N, mean, samples, seen[0])
    got = host(samples)
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[4], got[5])          # N completions of one image differ
    assert np.array_equal(got[8], x_in[4]) and np.array_equal(got[9], x_in[4])               # keep_rows = 28: the image itself
    # an int for the whole batch, a 4-d input, means only
    torch.manual_seed(12)
    only = model.pixelcnn_complete(dev(x_in).view(5, 1, 28, 28), 14)
    assert only.shape == (5, D)


def test_complete_keeps_the_given_rows_passes(case, sampler, monkeypatch):
    model, x_in, N = case["model"], case["x"][:5], 2
    sampler("passes")
    seen = _record_latents(model, monkeypatch)
    torch.manual_seed(13)
    mean, samples = model.pixelcnn_complete(dev(x_in), KEEP_ROWS, N=N, return_samples=True)
    _assert_completion("complete, passes", case, x_in, KEEP_ROWS, N, mean, samples, seen[0])


def test_one_short_passes_completion(case, sampler, monkeypatch):
    """B = 2, given = 756: the loop starts at the smallest `given`, 28 passes"""
    model, x_in = case["model"], case["x"][:2]
    sampler("passes")
    seen = _record_latents(model, monkeypatch)
    n, real = [0], torch.bernoulli

    def bernoulli(p, *a, **k):
        n[0] += 1
        return real(p, *a, **k)
    monkeypatch.setattr(torch, "bernoulli", bernoulli)
    torch.manual_seed(14)
    mean, samples = model.pixelcnn_complete(dev(x_in), 27, return_samples=True)
    assert n[0] == 28
    _assert_completion("complete, 28 passes", case, x_in, (27, 27), 1, mean, samples, seen[0])
    # through pixelcnn_generate, one `given` per image: 784 - min(given) passes
    n[0] = 0
    z1, z2 = seen[0]
    out = model.pixelcnn_generate(z1, z2, x_given=dev(x_in), given=[770, 784])
    assert n[0] == 14 and out.shape == (2, D)


def test_chunked_generation_is_bit_equal_to_one_launch(case, sampler, monkeypatch):
    from evae import ops
    from models import PixelCNN
    model, x_in = case["model"], case["x"]
    keep = (0, 3, 28, 14, 27, 1, 9)
    sampler("cached")
    assert PixelCNN.PIXEL_DECODE_CHUNK_IMAGES == 2048 and ops.pixel_decode_choose_images(7) == ops.pixel_decode_choose_images(3) == 1
    torch.manual_seed(15)
    one = model.pixelcnn_complete(dev(x_in), keep, return_samples=True)
    torch.manual_seed(16)
    z = torch.randn(7, 40, device="cuda"), torch.randn(7, 40, device="cuda")
    torch.manual_seed(17)
    gen = model.pixelcnn_generate(*z)
    launches = []
    real = ops.pixel_decode
    monkeypatch.setattr(ops, "pixel_decode", lambda *a, **k: launches.append(a[2].shape[0]) or real(*a, **k))
    monkeypatch.setattr(PixelCNN, "PIXEL_DECODE_CHUNK_IMAGES", 3)
    torch.manual_seed(15)
    chunked = model.pixelcnn_complete(dev(x_in), keep, return_samples=True)
    assert launches == [3, 3, 1]
    assert torch.equal(one[0], chunked[0]) and torch.equal(one[1], chunked[1])
    torch.manual_seed(17)
    assert torch.equal(gen, model.pixelcnn_generate(*z)) and launches == [3, 3, 1] * 2


def test_generate_without_the_new_arguments_is_todays_launch(case, sampler):
    from evae import ops
    model = case["model"]
    sampler("cached")
    rs = np.random.RandomState(483)
    z1, z2 = dev(rs.randn(3, 40).astype(np.float32)), dev(rs.randn(3, 40).astype(np.float32))
    torch.manual_seed(18)
    out = model.pixelcnn_generate(z1, z2)
    with torch.no_grad():
        latent = model._decoder_images(z1, z2)
        torch.manual_seed(18)
        u = torch.rand(3, D, device="cuda")
        packed = ops.pixel_decode_pack(model.pixelcnn, model.p_x_mean)
        mean, _, _ = ops.pixel_decode(packed, latent, torch.zeros(3, D, device="cuda"), u=u)
    assert torch.equal(out, mean)
