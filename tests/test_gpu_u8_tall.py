"""GPU tests of the 448-row instance of the byte layer's copy-pipeline forward (u8p_gemm_kernel<7, 2>, csrc/evae_dense_u8.hip),
at sizes where the host rule (u8_fwd_block_rows, csrc/evae_tile_map.h) picks 448 rows by itself: 4 200 gathered rows (nine full
blocks and one of 168 rows: a partial wave row) x 1 000 outputs (16 column tiles, the last one partial) make 17 x 16 = 272 blocks of
256 rows, more than the CUs of an MI355X, and 10 x 16 = 160 blocks of 448; K = 80 (three slabs, the last one partial) and K = 96.
Checked: out and s against float64 at the uint8 forward tests' bar (tests/test_gpu_kernels.py), and bit for bit against the same
entry points on slices of the rows short enough to run the 128-row kernel -- a row's result does not depend on the row count.
Run on a real MI355X:  python -m pytest tests -m gpu"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

R, M, N = 5000, 4200, 1000
SLICES = ((0, 1000), (1600, 2600), (3200, 4200))
COVER = ((0, 1000), (1000, 2000), (2000, 3000), (3000, 4000), (4000, 4200))      # all rows, each launch short, starts multiples of 8


def rel(a, b):
    return float((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.fixture(scope="module", params=[80, 96])
def case(request):
    """One layer per K: operands, the prepared weight image and the float64 restatement -- shared by the tests, never written."""
    from evae import ops as o, _lib
    lib = _lib.load()
    K = request.param
    rs = np.random.RandomState(448 + K)
    q = (rs.randint(0, 256, (R, K)) * (rs.random_sample((R, K)) < 0.4)).astype(np.uint8)
    rows_h = rs.randint(0, R, size=M).astype(np.int64)
    rows_h[100:140] = rows_h[7]                      # repeats: within a wave row, and across blocks
    rows_h[3000:4200:97] = rows_h[5]
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    wh, wg = (cuda((rs.standard_normal((N, K)) * 0.1).astype(np.float32)) for _ in range(2))
    bh, bg = (cuda((rs.standard_normal(N) * 0.1).astype(np.float32)) for _ in range(2))
    store = torch.zeros(R * K + 64, dtype=torch.uint8, device="cuda")          # slack behind the last row
    xs = store[:R * K].view(R, K); xs.copy_(torch.from_numpy(q))
    rows = cuda(rows_h)
    prep = o.u8_prepare(wh, wg)
    x64 = xs[rows].double() / 255.0
    g64 = torch.sigmoid(x64 @ wg.double().t() + bg.double())
    y64 = (x64 @ wh.double().t() + bh.double()) * g64

    class E:
        pass
    e = E()
    e.ops, e.lib, e.chk, e.count_calls = o, lib, _lib.check, _lib.count_calls
    e.K, e.xs, e.rows, e.prep, e.bh, e.bg, e.y64, e.g64 = K, xs, rows, prep, bh, bg, y64, g64

    def fwd(m0, m1, out, s, img=None, nks=0):
        """the entry point on rows m0 .. m1 - 1, results into the same rows of out / s (and image columns m0 ..)"""
        p = o._p
        at = lambda t, off: C.c_void_p(t.data_ptr() + off)
        if img is None:
            e.chk(lib.evae_gated_dense_fwd_u8(p(xs), at(rows, 8 * m0), m1 - m0, K, K, 1.0 / 255.0, p(prep), p(bh), p(bg), N, at(out, 4 * m0 * N),
                                              at(s, 4 * m0 * N), o._stream()), "fwd_u8")
        else:
            e.chk(lib.evae_gated_dense_fwd_u8_timg(p(xs), at(rows, 8 * m0), m1 - m0, K, K, 1.0 / 255.0, p(prep), p(bh), p(bg), N,
                                                   at(out, 4 * m0 * N), at(s, 4 * m0 * N), p(img), nks, 0, m0, o._stream()), "fwd_u8_timg")
    e.fwd = fwd
    return e


def test_the_host_rule_picks_448_rows_at_these_sizes(case):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles_n = (N + 63) // 64
    assert -(-M // 256) * tiles_n > cus >= -(-M // 448) * tiles_n, cus      # two rounds of 256-row blocks, one of 448-row blocks
    assert case.lib.evae_dense_u8_block_rows(M, N, cus) == 448
    assert case.lib.evae_dense_u8_block_rows(M, N, 0) == 448                # ... with the device's own CU count
    for m0, m1 in SLICES + COVER:
        assert case.lib.evae_dense_u8_block_rows(m1 - m0, N, cus) == 128    # the slices stay on the 128-row kernel


def test_448_row_forward_against_float64_and_the_short_launches(case):
    out = torch.full((M, N), float("nan"), device="cuda"); s = torch.full_like(out, float("nan"))
    with case.count_calls("evae_gated_dense_fwd_u8") as n:
        case.fwd(0, M, out, s)
    assert n == {"evae_gated_dense_fwd_u8": 1}
    e_out, e_s = rel(out, case.y64), rel(s, case.g64)
    print("K=%d  out %.3g  s %.3g  (bar 2e-6)" % (case.K, e_out, e_s))
    assert e_out < 2e-6
    assert e_s < 2e-6
    out_p = torch.empty_like(out); s_p = torch.empty_like(out)
    for m0, m1 in SLICES:
        case.fwd(m0, m1, out_p, s_p)
        assert torch.equal(out[m0:m1], out_p[m0:m1]) and torch.equal(s[m0:m1], s_p[m0:m1]), (m0, m1)


def test_448_row_forward_leaves_the_same_transposed_image(case):
    lib, o = case.lib, case.ops
    nks = lib.evae_p6_nks_rows(M)
    image = lambda: torch.zeros(lib.evae_p6_image_bytes(N, nks), dtype=torch.uint8, device="cuda")
    out0 = torch.empty((M, N), device="cuda"); s0 = torch.empty_like(out0)
    case.fwd(0, M, out0, s0)
    img = image(); out = torch.empty_like(out0); s = torch.empty_like(out0)
    with case.count_calls("evae_gated_dense_fwd_u8") as n:
        case.fwd(0, M, out, s, img, nks)
    assert n == {"evae_gated_dense_fwd_u8_timg": 1}
    assert torch.equal(out, out0) and torch.equal(s, s0)
    # the image of the short launches (the 128-row kernel), which together cover every row
    img_p = image(); out_p = torch.empty_like(out0); s_p = torch.empty_like(out0)
    for m0, m1 in COVER:
        case.fwd(m0, m1, out_p, s_p, img_p, nks)
    assert torch.equal(out, out_p) and torch.equal(s, s_p)
    assert torch.equal(img, img_p)
    # ... and evae_p6_pack_cols of the fp32 output, as tests/test_gpu_p6.py holds the other _timg entry points
    want = image()
    case.chk(lib.evae_p6_pack_cols(o._p(out), None, M, N, out.stride(0), -1, nks, o._p(want), want.numel(), o._stream()), "pack_cols")
    assert torch.equal(img, want)
