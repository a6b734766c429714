"""CPU-only checks of the cached pixelcnn sampler's host side: the packer's table (evae.ops.pixel_decode_layout) against the pixelcnn
state-dict fixture tests/test_pixelsnail_host.py loads, its agreement with the slot sizes compiled into csrc/evae_pixel_decode.hip,
and the refusals the C ABI and the operator make before anything is launched."""
import ctypes as C
import json
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def shapes():
    with open(os.path.join(GOLDEN, "g27_pixelcnn_state.json")) as f:
        return {k: tuple(s) for k, s in json.load(f)["entries"]}


def _numel(shape):
    n = 1
    for d in shape:
        n *= d
    return n


def test_packer_table_covers_the_decoder_state_dict_exactly_once(shapes):
    from evae import ops
    lay = ops.pixel_decode_layout(shapes)
    want = {k for k in shapes if k.startswith("pixelcnn.") or k.startswith("p_x_mean.conv.")}
    assert len(want) == 66
    seen = [(name, n) for e in lay["entries"] for name, n in e["sources"].items()]
    names = [name for name, _ in seen]
    assert sorted(names) == sorted(want)                                  # every one exactly once, nothing else
    for name, n in seen:
        assert n == _numel(shapes[name]), name                            # the element counts match
    assert not [n for n in names if not (n.startswith("pixelcnn.") or n.startswith("p_x_mean.conv."))]


def test_layout_matches_the_kernel_slots(shapes):
    from evae import ops, _lib
    lib = _lib.load()
    lay = ops.pixel_decode_layout(shapes)
    assert len(lay["table"]) == lib.evae_pixel_decode_table_len() == 9 + len(lay["entries"])
    assert lay["table"][:9] == [ops.PIXEL_DECODE_MAGIC, 64, 64, 28, 28, 4, 8, 4, lay["total"]]
    for s, e in enumerate(lay["entries"]):
        assert e["floats"] == lib.evae_pixel_decode_slot_floats(s), e["slot"]
        assert e["offset"] % 4 == 0 and lay["table"][9 + s] == e["offset"], e["slot"]
    end = 0
    for e in sorted(lay["entries"], key=lambda e: e["offset"]):          # no two slots overlap
        assert e["offset"] >= end, e["slot"]
        end = e["offset"] + e["floats"]
    assert end <= lay["total"]
    biases = [e for e in lay["entries"] if e["kind"] == "b"]             # one block, which the kernel keeps in LDS
    assert max(e["offset"] + e["floats"] for e in biases) - min(e["offset"] for e in biases) == sum(e["floats"] for e in biases) <= 2048
    assert lib.evae_pixel_decode_slot_floats(len(lay["entries"])) == -1 and lib.evae_pixel_decode_slot_floats(-1) == -1
    # the live taps: 7 of 9 for every causal 3 x 3 filter, everything else whole (the mean head's one output padded to 4)
    live = sum(e["floats"] for e in lay["entries"])
    whole = sum(_numel(s) for k, s in shapes.items() if (k.startswith("pixelcnn.") or k.startswith("p_x_mean.conv."))
                and not k.endswith("weight_g"))
    assert whole - live == 4 * (64 * 64 + 128 * 64) * 2 - (3 * 64 + 3)
    G = ops.pixel_decode_images_per_block()
    assert 1 <= G <= 16 and lib.evae_pixel_decode_lds_bytes() <= 160 * 1024
    assert lib.evae_pixel_decode_cache_floats() == 8 * 784 * 64 + 2 * 784 * 32


def test_abi_refuses_what_the_kernel_is_not_built_for_without_launching(shapes):
    from evae import ops, _lib
    lib = _lib.load()
    lay = ops.pixel_decode_layout(shapes)

    def call(table, B=2, t0=0, t1=784):
        arr = (C.c_int * len(table))(*table)
        # (null pointers: a call that got past the checks would fail on them, not launch)
        return lib.evae_pixel_decode(None, arr, len(table), None, None, None, None, None, B, t0, t1, None)

    good = lay["table"]
    assert call(good) == -1 and b"null" in lib.evae_last_error()
    assert call(good, B=0) == 0 and call(good, t0=5, t1=5) == 0          # nothing to do: no launch, no pointer read
    for pos, what in ((1, b"channel"), (2, b"channel"), (3, b"images"), (4, b"images"), (5, b"residual"), (6, b"heads"), (7, b"heads")):
        bad = list(good)
        bad[pos] += 1
        assert call(bad) == -1 and what in lib.evae_last_error(), pos
    bad = list(good)
    bad[0] = 0
    assert call(bad) == -1 and b"table" in lib.evae_last_error()
    assert call(good[:-1]) == -1 and b"entries" in lib.evae_last_error()
    bad = list(good)
    bad[-1] = good[8] - 4                                                 # the last slot (background) past the end of the buffer
    assert call(bad) == -1 and b"does not fit" in lib.evae_last_error()
    bad = list(good)
    bad[9 + 1] = 0                                                        # a bias slot far from the others
    assert call(bad) == -1 and b"one block" in lib.evae_last_error()
    bad = list(good)
    bad[10] += 1                                                          # an offset that is no multiple of 4
    assert call(bad) == -1 and b"does not fit" in lib.evae_last_error()
    assert call(good, t1=785) == -1 and b"785" in lib.evae_last_error()
    assert call(good, t0=5, t1=4) == -1 and b"range" in lib.evae_last_error()
    assert call(good, t0=-1, t1=4) == -1
    assert call(good, B=-1) == -1


def test_operator_refuses_cpu_tensors(shapes):
    from evae import ops, _lib
    lay = ops.pixel_decode_layout(shapes)
    packed = ops.PixelDecodeWeights(torch.zeros(lay["total"]), lay["table"], lay["entries"])
    with pytest.raises(_lib.EvaeError, match="no CPU fallback"):
        ops.pixel_decode(packed, torch.zeros(2, 2, 28, 28), torch.zeros(2, 784))


def test_sampler_flag_values():
    """the flag takes 'passes' and 'cached'; anything else is refused before any work"""
    from utils.utils import importing_model
    from test_pixelsnail_host import pixelcnn_args
    args = pixelcnn_args(pixelcnn_sampler="fast")
    model = importing_model(args)(args)
    with pytest.raises(ValueError, match="pixelcnn_sampler"):
        model.pixelcnn_generate(torch.zeros(1, 40), torch.zeros(1, 40))
