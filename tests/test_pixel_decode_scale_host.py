"""CPU-only checks of what the cached pixelcnn sampler gained for large batches and image completion: the three new entry points
agree between include/evae_hip.h, evae/_lib.py and the library; the LDS of the three kernel instances; the images-per-workgroup
table; the cache budget behind models.PixelCNN.PIXEL_DECODE_CHUNK_IMAGES; and the refusals made before anything is launched."""
import ctypes as C
import inspect
import json
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("evae_pixel_decode_ex", "evae_pixel_decode_lds_bytes_for", "evae_pixel_decode_choose_images")
CACHE_FLOATS = 8 * 784 * 64 + 2 * 8 * 784 * 4                              # 8 planes, K and V: 451 584


@pytest.fixture(scope="module")
def lib():
    from evae import _lib
    return _lib.load()


def test_new_symbols_agree_between_header_binding_and_library(lib):
    from evae import _lib
    with open(os.path.join(ROOT, "include", "evae_hip.h")) as f:
        header = f.read()
    raw = C.CDLL(lib._name)
    for name in NEW:
        decl = re.search(r"^\w[\w \*]*?\b%s\(([^;]*)\);" % name, header, re.M | re.S)
        assert decl, name
        n_args = 0 if decl.group(1).strip() == "void" else decl.group(1).count(",") + 1
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args, name
        assert hasattr(raw, name), name
    # _ex is the old entry point plus `start` (a pointer, after u) and `images_per_block` (an int, before the stream)
    old, new = _lib.SIGNATURES["evae_pixel_decode"][1], _lib.SIGNATURES["evae_pixel_decode_ex"][1]
    assert new == old[:6] + [C.c_void_p] + old[6:11] + [C.c_int] + old[11:]


def test_lds_of_the_three_instances(lib):
    per_image = 8 * 448 + 1192                                              # the 7 taps of 8 planes, the vectors (V_END)
    for g in (1, 2, 4):
        want = 4 * (g * per_image + 4 * 1024 * g + 64 + 2048)               # + four partial-sum regions, slot offsets, biases
        assert lib.evae_pixel_decode_lds_bytes_for(g) == want <= 160 * 1024, g
    assert lib.evae_pixel_decode_lds_bytes_for(1) == 43936
    for g in (-1, 0, 3, 5, 8, 16):
        assert lib.evae_pixel_decode_lds_bytes_for(g) == 0, g
    default = lib.evae_pixel_decode_images_per_block()
    assert default == 1
    assert lib.evae_pixel_decode_lds_bytes_for(default) == lib.evae_pixel_decode_lds_bytes()


def test_choose_images_table(lib):
    from evae import ops
    seen, last = set(), 1
    for B in list(range(0, 4200)) + [5000, 10000, 50000, 1 << 20, (1 << 31) - 1]:
        g = lib.evae_pixel_decode_choose_images(B)
        assert g in (1, 2, 4) and g >= last, (B, g, last)
        if B <= 256:
            assert g == 1, B
        seen.add(g)
        last = g
    assert lib.evae_pixel_decode_choose_images(-5) == 1
    # the table as measured: one round of at most 256 workgroups at 2 up to 512 images, 4 above
    assert seen == {1, 2, 4}
    assert [lib.evae_pixel_decode_choose_images(B) for B in (256, 257, 512, 513, 550, 2048, 2049)] == [1, 2, 2, 4, 4, 4, 4]
    assert ops.pixel_decode_choose_images(100) == 1 and ops.pixel_decode_choose_images(550) == lib.evae_pixel_decode_choose_images(550)


def test_cache_budget_arithmetic(lib):
    from evae import ops
    from models import PixelCNN
    assert lib.evae_pixel_decode_cache_floats() == CACHE_FLOATS == 451584
    for B in (0, 1, 7, 2048):
        assert ops.pixel_decode_cache_bytes(B) == B * 4 * (CACHE_FLOATS + 784)
    chunk = PixelCNN.PIXEL_DECODE_CHUNK_IMAGES
    assert chunk == 2048
    assert 3.6e9 < ops.pixel_decode_cache_bytes(chunk) < 3.8e9               # "about 3.7 GB", whatever the batch
    assert ops.pixel_decode_cache_bytes(50000) > 90e9                        # what one launch of an augmentation-sized batch would ask for


def _table():
    from evae import ops
    with open(os.path.join(ROOT, "tests", "golden", "g27_pixelcnn_state.json")) as f:
        shapes = {k: tuple(s) for k, s in json.load(f)["entries"]}
    return ops.pixel_decode_layout(shapes)


def test_abi_refuses_other_images_per_block_before_anything_else(lib):
    good = _table()["table"]
    arr = (C.c_int * len(good))(*good)

    def call(g, B=2, t0=0, t1=784):
        # (null pointers: a call that got past the checks would fail on them, not launch)
        return lib.evae_pixel_decode_ex(None, arr, len(good), None, None, None, None, None, None, B, t0, t1, g, None)

    for g in (3, 0, 8, -1, 5):
        assert call(g) == -1 and (b"%d images" % g) in lib.evae_last_error(), g
        assert call(g, B=0) == -1 and (b"%d images" % g) in lib.evae_last_error(), g      # refused even with nothing to do
    for g in (1, 2, 4):
        assert call(g) == -1 and b"null" in lib.evae_last_error(), g        # past the new check, on to the old ones
        assert call(g, B=0) == 0 and call(g, t0=9, t1=9) == 0
        assert call(g, t1=785) == -1 and b"785" in lib.evae_last_error()


def test_operator_signature_and_cpu_refusal():
    from evae import ops, _lib
    sig = inspect.signature(ops.pixel_decode)
    assert list(sig.parameters)[:7] == ["packed", "latent", "x", "u", "t0", "t1", "cache"]
    assert sig.parameters["start"].default is None and sig.parameters["images_per_block"].default is None
    lay = _table()
    packed = ops.PixelDecodeWeights(torch.zeros(lay["total"]), lay["table"], lay["entries"])
    with pytest.raises(_lib.EvaeError, match="no CPU fallback"):
        ops.pixel_decode(packed, torch.zeros(2, 2, 28, 28), torch.zeros(2, 784), start=3, images_per_block=2)


def test_model_refuses_half_a_completion_and_wrong_lengths():
    from utils.utils import importing_model
    from test_pixelsnail_host import pixelcnn_args
    args = pixelcnn_args()
    model = importing_model(args)(args)
    z = torch.zeros(2, 40)
    with pytest.raises(ValueError, match="go together"):
        model.pixelcnn_generate(z, z, x_given=torch.zeros(2, 784))
    with pytest.raises(ValueError, match="go together"):
        model.pixelcnn_generate(z, z, given=28)
    with pytest.raises(ValueError, match="x_given"):
        model.pixelcnn_generate(z, z, x_given=torch.zeros(3, 784), given=28)
    with pytest.raises(ValueError, match="one int per image"):
        model.pixelcnn_generate(z, z, x_given=torch.zeros(2, 784), given=[1, 2, 3])
