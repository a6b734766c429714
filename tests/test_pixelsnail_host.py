"""CPU-only checks of the `pixelcnn` model (PixelSNAIL decoder): the registry builds it with the reference's state dict, the new
layers keep the reference's constructor signatures, the float64 restatement the GPU tests compare against (tests/pixelsnail_ref.py)
reproduces the real reference (goldens G27 (a)-(c), tools/gen_goldens.py::g27), the documented dropout-mask layout keeps the share
it should, and the C ABI refuses what the attention kernel does not support before anything is launched."""
import inspect
import json
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import pixelsnail_ref as psr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def pixelcnn_args(**kw):
    a = dict(prior="exemplar_prior", input_type="binary", input_size=[1, 28, 28], hidden_size=300, z1_size=40, z2_size=40,
             model_name="pixelcnn", device="cpu", number_components=1000, training_set_size=50000, approximate_prior=False,
             approximate_k=10, no_mask=False, no_attention=False, same_variational_var=False, use_logit=False, lambd=1e-4,
             bottleneck=6, dataset_name="dynamic_mnist", continuous=False)
    a.update(kw)
    return Namespace(**a)


@pytest.fixture(scope="module")
def state_fixture():
    with open(os.path.join(GOLDEN, "g27_pixelcnn_state.json")) as f:
        return json.load(f)


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def test_registry_builds_pixelcnn_with_the_reference_state_dict(state_fixture):
    from utils.utils import importing_model
    args = pixelcnn_args()
    cls = importing_model(args)
    model = cls(args)
    got = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    assert len(state_fixture["entries"]) == 143
    assert got == state_fixture["entries"]
    assert sum(p.numel() for p in model.parameters()) == state_fixture["parameters"] == 1638510


def test_out_of_scope_configurations_raise():
    from utils.utils import importing_model
    from utils.nn import PixelSNAIL
    for kind in ("gray", "continuous"):
        with pytest.raises(NotImplementedError):
            importing_model(pixelcnn_args(input_type=kind))(pixelcnn_args(input_type=kind))
    with pytest.raises(NotImplementedError):
        PixelSNAIL([6, 5], 8, 8, 3, 1, 0, 8, n_cond_res_block=1, cond_res_channel=4)
    net = PixelSNAIL([6, 5], 8, 8, 3, 1, 0, 8)
    with pytest.raises(NotImplementedError):
        net(torch.zeros(1, 3, 6, 5), condition=torch.zeros(1, 3, 3, dtype=torch.long))


def test_layer_signatures_match_the_reference(state_fixture):
    import utils.nn as nn_
    for name, want in state_fixture["signatures"].items():
        obj = getattr(nn_, name)
        params = inspect.signature(getattr(obj, "__wrapped__", obj)).parameters
        got = [[n, (None if p.default is inspect.Parameter.empty else repr(p.default))] for n, p in params.items()]
        assert got == want, name
    m, s = nn_.causal_mask(4)
    assert m.shape == (1, 4, 4) and s.shape == (4, 1) and m.dtype == torch.uint8
    assert m[0].tolist() == [[0, 0, 0, 0], [1, 0, 0, 0], [1, 1, 0, 0], [1, 1, 1, 0]] and s.reshape(-1).tolist() == [0, 1, 1, 1]


def _sd64(g):
    return {k[2:]: torch.from_numpy(g[k]).double() for k in g.files if k.startswith("p.")}


def _check(g, fn, inputs):
    """fn(sd, *inputs) -> out; outputs, input gradients and every parameter gradient against the golden, 1e-10 relative"""
    sd = {k: v.clone().requires_grad_(v.dtype.is_floating_point and not k.endswith("background")) for k, v in _sd64(g).items()}
    xs = [torch.from_numpy(g["x." + n]).double().requires_grad_(True) for n in inputs]
    out = fn(sd, *xs)
    assert rel(out.detach().numpy(), g["out"]) < 1e-10
    (out * torch.from_numpy(g["gout"]).double()).sum().backward()
    for n, x in zip(inputs, xs):
        assert rel(x.grad.numpy(), g["dx." + n]) < 1e-10, n
    names = [k[2:] for k in g.files if k.startswith("g.")]
    assert names
    # relative to the module's largest parameter gradient: the key bias of the attention adds one constant to every score of a
    # row, which the softmax ignores -- its gradient is zero in exact arithmetic and 1e-16 of rounding in the golden
    scale = max(np.abs(g["g." + n]).max() for n in names)
    for n in names:
        assert sd[n].grad is not None, n
        assert np.abs(sd[n].grad.numpy() - g["g." + n]).max() < 1e-10 * scale, n


def test_ref_reproduces_attention_golden(golden):
    g = golden("g27_attention")
    assert g["x.query"].shape == (2, 66, 6, 5) and g["x.key"].shape == (2, 130, 6, 5) and g["out"].shape == (2, 32, 6, 5)
    assert g["out"].dtype == np.float64 and g["x.query"].dtype == np.float32
    assert np.abs(g["out"][:, :, 0, 0]).max() == 0.0                     # the start mask: pixel 0 attends to nothing
    _check(g, lambda sd, q, k: psr.causal_attention({"m." + n: v for n, v in sd.items()}, "m", q, k), ["query", "key"])


def test_ref_reproduces_gated_resblock_golden(golden):
    g = golden("g27_gated_resblock")
    assert g["x.input"].shape == (2, 16, 6, 5)
    v = g["p.conv1.conv.conv.weight_v"]
    assert np.abs(v[:, :, -1, 1:]).max() == 0.0 and np.abs(v[:, :, -1, 0]).min() > 0.0     # stored masked, as a checkpoint is
    _check(g, lambda sd, x: psr.gated_resblock({"m." + n: t for n, t in sd.items()}, "m", x, 3, conv="causal"), ["input"])


def test_ref_reproduces_pixelsnail_golden(golden):
    g = golden("g27_pixelsnail")
    assert g["x.input"].shape == (2, 3, 6, 5) and g["out"].shape == (2, 64, 6, 5)
    assert sum(g[k].size for k in g.files if k.startswith("g.")) > 60000
    _check(g, lambda sd, x: psr.pixelsnail(sd, x, 3, 1, 0), ["input"])


def test_restated_decoder_is_causal():
    """the mean of pixel p does not move when x changes at pixels >= p (float64: exactly)"""
    torch.manual_seed(5)
    from utils.nn import PixelSNAIL
    net = PixelSNAIL([6, 5], 16, 16, 3, 1, 1, 16)
    sd = {k: v.double() for k, v in net.state_dict().items()}
    x = torch.randn(1, 3, 6, 5, dtype=torch.float64)
    y0 = psr.pixelsnail(sd, x, 3, 1, 1).reshape(1, 16, 30)
    x2 = x.clone().reshape(1, 3, 30)
    x2[:, :, 17:] += 1.0
    y1 = psr.pixelsnail(sd, x2.reshape(1, 3, 6, 5), 3, 1, 1).reshape(1, 16, 30)
    assert torch.equal(y0[:, :, :18], y1[:, :, :18]) and not torch.equal(y0[:, :, 18:], y1[:, :, 18:])


def test_dropout_mask_keeps_its_share():
    """10^6 draws of the documented layout: the kept share is within 4 sigma of 1 - p; another offset or seed is another mask"""
    n = 1000000
    for p in (0.1, 0.5):
        keep = psr.flat_keep_mask(n, p, seed=1234, offset=7)
        sigma = np.sqrt(p * (1 - p) / n)
        assert abs(keep.mean() - (1 - p)) < 4 * sigma, (p, keep.mean())
    a = psr.flat_keep_mask(4096, 0.1, 1234, 7)
    assert not np.array_equal(a, psr.flat_keep_mask(4096, 0.1, 1234, 8))
    assert not np.array_equal(a, psr.flat_keep_mask(4096, 0.1, 1235, 7))
    assert np.array_equal(a[:1001], psr.flat_keep_mask(1001, 0.1, 1234, 7))          # a prefix, whatever the length
    assert psr.attn_keep_mask(3, 5, 0.1, 9, 2).shape == (3, 5, 5)
    assert psr.flat_keep_mask(64, 0.0, 1, 1).all()


def test_per_head_masks_are_slices_of_the_whole_mask():
    """an even L (every head starts on a quad) and an odd one (heads start inside a quad); a wrap no index reaches changes nothing,
    one inside the tensor restarts the stream there"""
    for BH, L in ((5, 6), (4, 5)):
        whole = psr.attn_keep_mask(BH, L, 0.3, 1234, 7)
        assert 0 < whole.mean() < 1
        for bh in range(BH):
            assert np.array_equal(psr.attn_keep_mask_head(bh, L, 0.3, 1234, 7), whole[bh]), (L, bh)
            assert np.array_equal(psr.attn_keep_mask_head(bh, L, 0.3, 1234, 7, wrap_bits=8), whole[bh]), (L, bh)
    flat = psr.flat_keep_mask(5 * 36, 0.3, 1234, 7)
    wrapped = np.concatenate([psr.attn_keep_mask_head(bh, 6, 0.3, 1234, 7, wrap_bits=6).reshape(-1) for bh in range(5)])
    assert np.array_equal(wrapped, np.concatenate([flat[:64], flat[:64], flat[:52]])) and not np.array_equal(wrapped, flat)
    assert np.array_equal(psr.flat_keep_mask(21, 0.3, 1234, 7, first=40), flat[40:61])
    with pytest.raises(AssertionError):
        psr.flat_keep_mask(8, 0.3, 1234, 7, first=2)


def test_mask_offset_reaches_the_second_counter_word():
    """first = 2^34 - 8: quads 2^32 - 2, 2^32 - 1, 2^32 -- counter words (0xFFFFFFFE, 0), (0xFFFFFFFF, 0) and (0, 1)"""
    import philox_ref as pr
    seed, offset, p = 0x1234567887654321, 0x100000003, 0.3
    got = psr.flat_keep_mask(12, p, seed, offset, first=(1 << 34) - 8)
    off = (offset & 0xFFFFFFFF, offset >> 32)
    want = []
    for lo, hi in ((0xFFFFFFFE, 0), (0xFFFFFFFF, 0), (0, 1)):
        words = pr.philox4x32_10((np.uint64(lo), np.uint64(hi), np.uint64(off[0]), np.uint64(off[1])), pr.seed_key(seed))
        want += [bool(pr.u01(w) >= np.float32(p)) for w in words]
    assert got.tolist() == want and 0 < sum(want) < 12
    # ... and is not what the low counter word alone gives: quad 2^32 is not quad 0
    assert np.array_equal(psr.flat_keep_mask(12, p, seed, offset), psr.flat_keep_mask(12, p, seed, offset, first=0))
    assert not np.array_equal(psr.flat_keep_mask(256, p, seed, offset, first=1 << 34), psr.flat_keep_mask(256, p, seed, offset))


def test_attention_abi_refuses_unsupported_shapes_without_launching():
    from evae import _lib
    lib = _lib.load()
    lmax = lib.evae_causal_attn_max_len()
    assert lmax >= 784
    for L in (1, 2, 783, 784, lmax):
        assert lib.evae_causal_attn_lds_bytes(L, 0) == 32 * L and lib.evae_causal_attn_lds_bytes(L, 1) == 40 * L <= 65536
    assert lib.evae_causal_attn_lds_bytes(lmax + 1, 0) == 0 and lib.evae_causal_attn_lds_bytes(0, 1) == 0
    assert lib.evae_causal_attn_lds_bytes(8, 2) == 0
    # (null pointers: a call that got past the checks would fail on them, not launch)
    assert lib.evae_causal_attn_fwd(None, None, None, 2, 8, 16, 8, 0.0, 0, 0, None, None, None) == -1
    assert b"head width" in lib.evae_last_error()
    assert lib.evae_causal_attn_fwd(None, None, None, 2, 8, lmax + 1, 4, 0.0, 0, 0, None, None, None) == -1
    assert b"LDS" in lib.evae_last_error()
    assert lib.evae_causal_attn_bwd(None, None, None, None, None, None, 2, 8, 16, 4, 1.0, 0, 0, None, None, None, None, None) == -1
    assert b"p_drop" in lib.evae_last_error()
    assert lib.evae_causal_attn_fwd(None, None, None, 2, 8, 16, 4, 0.0, 0, 0, None, None, None) == -1
    assert b"null" in lib.evae_last_error()
    assert lib.evae_elu_dropout_fwd(None, 4, -0.5, 0, 0, None, None) == -1
    assert lib.evae_glu_res_fwd(None, None, 4, 0, None, None) == -1


def test_ops_refuse_cpu_tensors():
    from evae import ops, _lib
    q = torch.zeros(6, 8)
    with pytest.raises(_lib.EvaeError):
        ops.causal_attn(q, q, q, 2, 3, 2)
    with pytest.raises(_lib.EvaeError):
        ops.elu_dropout(torch.zeros(5))
    with pytest.raises(_lib.EvaeError):
        ops.glu_res(torch.zeros(3, 8), torch.zeros(3, 4))
