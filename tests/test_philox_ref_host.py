"""The host reference of the step's generator (tests/philox_ref.py) against published known answers -- no GPU needed.
tests/test_gpu_step_head.py then holds the device to this reference."""
import numpy as np

import philox_ref as pr

# Random123's known-answer vectors for philox4x32, 10 rounds (its kat_vectors file): counter, key, expected output
KAT = [
    ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def _run(ctr, key, **kw):
    return tuple(int(w) for w in pr.philox4x32(ctr, key, **kw))


def test_known_answer_vectors():
    for ctr, key, want in KAT:
        assert tuple(int(w) for w in pr.philox4x32_10(ctr, key)) == want


def test_known_answer_vectors_as_one_vectorised_call():
    ctr = [np.array([k[0][i] for k in KAT], dtype=np.uint64) for i in range(4)]
    out = pr.philox4x32_10(ctr, (np.array([k[1][0] for k in KAT], dtype=np.uint64), np.array([k[1][1] for k in KAT], dtype=np.uint64)))
    for j, (_, _, want) in enumerate(KAT):
        assert tuple(int(w[j]) for w in out) == want
    assert all(int(w.max()) <= 0xFFFFFFFF for w in out)


def test_wrong_generators_miss_the_known_answers():
    for ctr, key, want in KAT:
        assert _run(ctr, key, rounds=9) != want
        assert _run(ctr, key, rounds=11) != want
        assert _run(ctr, key, multipliers=(pr.M1, pr.M0)) != want


def test_the_two_streams_never_share_a_counter():
    quads = np.array([0, 1, 2, 3, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 5], dtype=np.uint64)
    steps = [0, 1, 7, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 7, 2 ** 40 + 1, 2 ** 62 + 3]
    seen = {}
    for stream in (pr.STREAM_IMAGE, pr.STREAM_EPS):
        for step in steps:
            c = np.broadcast_arrays(*pr.stream_counter(quads, step, stream))
            assert np.all((c[3] & np.uint64(1)) == stream)               # the stream bit, for every quad and step
            for j in range(quads.size):
                k = tuple(int(w[j]) for w in c)
                assert k not in seen, (k, seen[k], (stream, step, int(quads[j])))
                seen[k] = (stream, step, int(quads[j]))
    assert len(seen) == 2 * len(steps) * quads.size
    # ... and the high words of the step and of the seed reach the generator
    assert pr.stream_counter(quads, 7, 0)[3] != pr.stream_counter(quads, 2 ** 32 + 7, 0)[3]
    assert pr.seed_key(5) != pr.seed_key(2 ** 32 + 5)


def test_uniforms_are_exact_float32_in_their_intervals():
    r = np.array([0, 255, 256, 0xFFFFFFFF, 0xFFFFFF00], dtype=np.uint64)
    assert pr.u01(r).dtype == np.float32 and pr.u01_open(r).dtype == np.float32
    assert pr.u01(r).tolist() == [0.0, 0.0, 2.0 ** -24, 1.0 - 2.0 ** -24, 1.0 - 2.0 ** -24]
    assert pr.u01_open(r).tolist() == [2.0 ** -24, 2.0 ** -24, 2.0 ** -23, 1.0, 1.0]


def test_streams_do_not_depend_on_the_batch_shape():
    """element e = word e % 4 of quad e // 4 of the FLATTENED array: the same draws however they are cut into rows"""
    a = pr.image_uniforms(3, 7, 5, 7).reshape(-1)
    b = pr.image_uniforms(7, 3, 5, 7).reshape(-1)
    c = pr.image_uniforms(1, 24, 5, 7).reshape(-1)
    assert np.array_equal(a, b) and np.array_equal(a, c[:21])
    e = pr.eps_draws(3, 5, 5, 7).reshape(-1)
    assert np.array_equal(e, pr.eps_draws(1, 16, 5, 7).reshape(-1)[:15])
    assert not np.array_equal(pr.image_uniforms(3, 7, 5, 8), pr.image_uniforms(3, 7, 5, 7))
    assert not np.array_equal(pr.image_uniforms(3, 7, 6, 7), pr.image_uniforms(3, 7, 5, 7))


def test_binarise_at_the_edges_of_the_comparison():
    p = np.zeros((50, 40), np.float32)
    p[:, 1] = 1.0
    p[:, 2] = np.float32(2.0 ** -24)
    x = pr.binarise(p, 5, 7)
    u = pr.image_uniforms(50, 40, 5, 7)
    assert not x[:, 0].any() and x[:, 1].all() and np.array_equal(x[:, 2] == 1.0, u[:, 2] == 0.0)


def test_eps_moments():
    e = pr.eps_draws(2500, 100, 5, 7)
    assert e.shape == (2500, 100) and e.dtype == np.float64 and np.isfinite(e).all()
    assert abs(e.mean()) < 0.01 and abs(e.var() - 1.0) < 0.01
