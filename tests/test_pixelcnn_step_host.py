"""Host side of the captured pixelcnn step (no GPU): which configurations utils/training.py::pixelcnn_step_eligible takes, where
evae.ops._rng_args takes a dropout mask's Philox words from (the process counter, or the step's source on the hand-off), and the
one offset formula of the device-sourced launches, evae_dropout_step_offset, against its restatement."""
import ctypes
import itertools

import pytest

import smoke_case


def step_offset(counter, ordinal):
    """include/evae_hip.h: 2^63 | (counter mod 2^47) << 16 | ordinal"""
    return (1 << 63) | ((counter % (1 << 47)) << 16) | ordinal


def test_eligibility_over_the_argument_grid():
    from utils.training import pixelcnn_step_eligible
    grid = itertools.product(("pixelcnn", "vae", "hvae_2level", "convhvae_2level"), ("exemplar_prior", "vampprior", "standard"),
                             (False, True), (False, True, None))
    seen = 0
    for model_name, prior, approximate, shard_exemplars in grid:
        a = smoke_case.vae_args(model_name=model_name, prior=prior, approximate_prior=approximate)
        if shard_exemplars is not None:                              # (None: the attribute is absent, as in a plain run)
            a.shard_exemplars = shard_exemplars
        want = model_name == "pixelcnn" and prior == "exemplar_prior" and approximate is False and not shard_exemplars
        assert pixelcnn_step_eligible(a) is want, (model_name, prior, approximate, shard_exemplars)
        seen += want
    assert seen == 2                                                 # shard_exemplars False and absent


def test_eligibility_has_no_capture_flag():
    """the captured step is ahead of the eager one at a measured size (profiles/pixelsnail_step.json), so it is on by default: an
    explicit pixelcnn_capture attribute, either way, changes nothing"""
    from utils.training import pixelcnn_step_eligible
    for flag in (True, False):
        a = smoke_case.vae_args(model_name="pixelcnn")
        a.pixelcnn_capture = flag
        assert pixelcnn_step_eligible(a) is True


def test_rng_args_without_a_handoff_advance_the_process_counter():
    from evae import handoff, ops
    assert handoff.current() is None
    n0 = ops._DROPOUT_CALLS[0]
    p, seed, off, src = ops._rng_args(0.1, None)
    assert (p, off, src) == (0.1, n0, None) and ops._DROPOUT_CALLS[0] == n0 + 1
    assert ops._rng_args(0.1, None)[2] == n0 + 1 and ops._DROPOUT_CALLS[0] == n0 + 2
    assert ops._rng_args(0.0, None) == (0.0, 0, 0, None) and ops._DROPOUT_CALLS[0] == n0 + 2       # p = 0 draws nothing
    assert ops._rng_args(0.25, (7, 9)) == (0.25, 7, 9, None) and ops._DROPOUT_CALLS[0] == n0 + 2   # an explicit pair: as given
    # a hand-off without a dropout source (every model but pixelcnn) changes nothing
    with handoff.active(handoff.StepHandoff()):
        assert ops._rng_args(0.1, None)[2:] == (n0 + 2, None)
    assert ops._DROPOUT_CALLS[0] == n0 + 3


def test_rng_args_take_ordinals_from_the_step_source():
    from evae import handoff, ops
    block = object()                                                 # stands for the control block's seed_ctr tensor
    n0 = ops._DROPOUT_CALLS[0]
    h = handoff.StepHandoff()
    h.dropout = handoff.DropoutSource(block)
    with handoff.active(h):
        got = [ops._rng_args(0.1, None) for _ in range(3)]
        assert ops._rng_args(0.0, None) == (0.0, 0, 0, None)         # p = 0 takes no ordinal ...
        got.append(ops._rng_args(0.5, None))                         # ... so the next mask is number 3
        assert ops._rng_args(0.1, (7, 9)) == (0.1, 7, 9, None)       # an explicit pair goes the host way, and takes none either
        got.append(ops._rng_args(0.1, None))
    assert [g[2] for g in got] == [0, 1, 2, 3, 4] and all(g[3] is block and g[1] == 0 for g in got)
    assert got[3][0] == 0.5 and h.dropout.ordinal == 5
    assert ops._DROPOUT_CALLS[0] == n0                               # the process counter never moved
    assert handoff.current() is None
    # every step starts at 0 again
    h2 = handoff.StepHandoff()
    h2.dropout = handoff.DropoutSource(block)
    with handoff.active(h2):
        assert ops._rng_args(0.1, None)[2] == 0
    # an explicit StepRng names its own ordinal and moves nothing
    assert ops._rng_args(0.1, ops.StepRng(block, 41)) == (0.1, 0, 41, block) and ops._DROPOUT_CALLS[0] == n0


@pytest.mark.parametrize("counter", [0, 1, (1 << 47) - 1, 1 << 47])
@pytest.mark.parametrize("ordinal", [0, 65535])
def test_step_offset_matches_its_restatement(counter, ordinal):
    from evae import _lib, ops
    got = _lib.load().evae_dropout_step_offset(counter, ordinal)
    assert got == step_offset(counter, ordinal) == ops.dropout_step_offset(counter, ordinal)
    assert got >> 63 == 1 and got & 0xFFFF == ordinal                # bit 63: apart from every host-counter offset 0, 1, 2, ...
    if counter == 1 << 47:
        assert got == step_offset(0, ordinal)                        # the counter wraps at 2^47


def test_ordinal_65536_is_refused():
    """by the launch wrappers (EVAE_EINVAL before anything is launched: no GPU is touched) and by the operators' helper"""
    from evae import _lib, ops
    lib = _lib.load()
    buf = (ctypes.c_float * 8)()
    ctr = (ctypes.c_int64 * 2)(5, 7)
    x, c = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(ctr, ctypes.c_void_p)
    EINVAL = lib.evae_elu_dropout_fwd(x, 4, 1.5, 0, 0, x, None)      # (p_drop outside [0, 1): the library's invalid-argument code)
    assert EINVAL != 0
    for p in (0.1, 0.0):
        assert lib.evae_elu_dropout_fwd_dev(x, 4, p, c, 65536, x, None) == EINVAL
        assert b"ordinal" in lib.evae_last_error()
        assert lib.evae_elu_dropout_bwd_dev(x, x, 4, p, c, 65536, x, None) == EINVAL
        assert lib.evae_causal_attn_fwd_dev(x, x, x, 1, 1, 1, 4, p, c, 65536, x, x, None) == EINVAL
        assert lib.evae_causal_attn_bwd_dev(x, x, x, x, x, x, 1, 1, 1, 4, p, c, 65536, x, x, x, x, None) == EINVAL
    assert lib.evae_dropout_step_offset(3, 65536) == 0               # outside the function's domain: no step offset is 0
    with pytest.raises(_lib.EvaeError, match="ordinal"):
        ops.dropout_step_offset(3, 65536)
    # with dropout on, a null counter block is refused too (p = 0 never reads it, so null is fine there: the GPU tests run that)
    assert lib.evae_elu_dropout_fwd_dev(x, 4, 0.1, None, 0, x, None) == EINVAL
