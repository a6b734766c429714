"""The tables of tests/conv_edge_cases.py, checked without a GPU: every row's float64 reference is built here and the edge the row
exists for must really occur in it -- so that tests/test_gpu_conv_edges.py, which imports the same tables, cannot drift into testing
nothing.  The declared kernel family of every row is held to the library's selection rule restated in Python."""
import numpy as np
import pytest
import torch

import conv_edge_cases as ce

IDS = [r.id for r in ce.ALL_ROWS]


def test_tables_are_complete():
    assert len(set(IDS)) == len(IDS)
    assert len(ce.ACT_ROWS) == 10 and len(ce.SUBSET_ROWS) == 3 * (10 + 12)
    fams = {r.fam for r in ce.ALL_ROWS}
    # every branch of Conv2dFn.backward: all channels-last, the mixed case, all NCHW, patch forward with either weight gradient
    assert {("cl", "cl", "cl"), ("cl", "nchw", "cl"), ("nchw", "nchw", "nchw"), ("patch", "patch", "nchw"),
            ("cl", "cl", "none"), ("nchw", "nchw", "none"), ("patch", "patch", "none")} <= fams, fams
    for rows, both in ((ce.SUBSET_ROWS, True), (ce.GEOM_ROWS, True), (ce.ACT_ROWS, False)):
        assert {r.gated for r in rows} == ({True, False} if both else {False})
    assert {r.act for r in ce.ACT_ROWS} == {"sigmoid", "hardtanh"}
    assert {r.gout for r in ce.SUBSET_ROWS} == {"nchw", "cl", "slice", "expand"}
    assert {r.x_layout for r in ce.SUBSET_ROWS} == {"nchw", "cl", "slice"}
    assert sum(r.raises for r in ce.ALL_ROWS) == 2 and sum(r.per_pass is not None for r in ce.ALL_ROWS) == 4
    assert all(r.poison for r in ce.ALL_ROWS if r.small_filter) and sum(r.small_filter for r in ce.ALL_ROWS) == 16


@pytest.mark.parametrize("rid", IDS)
def test_row_has_outputs_and_its_declared_family_is_the_rule(rid):
    row = ce.BY_ID[rid]
    N, C, H, W, Co, KH, KW, s, p = row.geom
    OH, OW = ce.out_dims(row.geom)
    assert OH > 0 and OW > 0
    assert row.fam == ce.family_rule(row.geom, row.gated, "x" in row.grads), (row.fam, ce.family_rule(row.geom, row.gated, "x" in row.grads))
    ref = ce.reference(rid)
    assert tuple(ref["y"].shape) == (N, Co, OH, OW)
    assert (ref["dx"] is not None) == ("x" in row.grads)
    assert (ref["dwh"] is not None) == ("w" in row.grads) and (ref["dwg"] is not None) == ("w" in row.grads and row.gated)
    assert (ref["dbh"] is not None) == ("b" in row.grads and row.bh) and (ref["dbg"] is not None) == ("b" in row.grads and row.bg)
    for k, v in ref.items():
        assert v is None or bool(torch.isfinite(v).all()), k
    if row.raises:      # the NCHW data gradient takes strides up to 3 (csrc/evae_conv.hip)
        assert row.fam[2] == "nchw" and s > 3


@pytest.mark.parametrize("rid", IDS)
def test_structural_zeros_are_exact_in_the_reference(rid):
    """where structural_zeros() says zero the float64 gradient IS zero, and the rest of the tensor is alive"""
    row = ce.BY_ID[rid]
    ref = ce.reference(rid)
    for name, mask in ce.structural_zeros(row).items():
        if ref[name] is None:
            continue
        assert mask.shape == ref[name].shape
        assert bool((ref[name][mask] == 0).all()), name
        assert bool((ref[name][~mask] != 0).any()), name


@pytest.mark.parametrize("rid", [r.id for r in ce.ALL_ROWS if r.small_filter])
def test_small_filter_rows_leave_input_pixels_without_a_tap(rid):
    row = ce.BY_ID[rid]
    N, C, H, W, Co, KH, KW, s, p = row.geom
    assert min(KH, KW) < s
    mask = ce.structural_zeros(row)["dx"]
    dx = ce.reference(rid)["dx"]
    assert bool(mask.any()) and bool((~mask).any())
    assert bool((dx[mask] == 0).all())
    assert bool((dx[~mask] != 0).all())          # every reached pixel of every channel carries a gradient


@pytest.mark.parametrize("rid", [r.id for r in ce.ALL_ROWS if r.act == "hardtanh"])
def test_hardtanh_rows_sit_on_both_bounds_and_just_inside(rid):
    row = ce.BY_ID[rid]
    ref = ce.reference(rid)
    pre = ref["pre"]
    assert bool((pre[:, 0] == ce.LO).all()) and bool((pre[:, 1] == ce.HI).all())
    assert bool((pre[:, 2] == float(ce.LO_IN)).all()) and ce.LO < float(ce.LO_IN) < ce.LO + 1e-6
    # torch's Hardtanh passes no gradient AT a bound (csrc/evae_dense.hip: v > lo && v < hi): channels 0 and 1 are dead, 2 is alive
    if ref["dbh"] is not None:
        assert ref["dbh"][0] == 0 and ref["dbh"][1] == 0 and ref["dbh"][2] != 0
        t = ce.inputs(row)
        assert abs(float(ref["dbh"][2]) - float(t["gout"][:, 2].double().sum())) <= 1e-12 * float(t["gout"][:, 2].double().abs().sum())
    # the random channels clamp on both sides and pass in between, and none of their pre-activations is within float32 rounding of
    # a bound: the only entries ON a bound are the planted ones
    rest = pre[:, 3:]
    assert bool((rest > ce.HI).any()) and bool(((rest > ce.LO) & (rest < ce.HI)).any())
    assert float(torch.minimum((rest - ce.LO).abs(), (rest - ce.HI).abs()).min()) > 1e-4


def test_gradient_buffer_strides_round_up_to_64():
    assert ce.dy_stride(33) == 64 and ce.dy_stride(34) == 64 and ce.dy_stride(4) == 4 and ce.dy_stride(1) == 32 and ce.dy_stride(6) == 32
    by = {r.id: r for r in ce.GEOM_ROWS}
    assert by["geo-ldy-33-plain"].geom[4] == 33 and by["geo-ldy-34-gated"].geom[4] * 2 == 34
    # the thresholds sit where the rule changes: 64 patch columns against 100, 64 taps against 81
    for rid, cols, taps in (("geo-patch-64-c4-plain", 64, 16), ("geo-patch-64-c1-plain", 64, 64), ("geo-no-patch-100-plain", 100, 25),
                            ("geo-taps-64-plain", 1024, 64), ("geo-taps-81-plain", 1296, 81)):
        N, C, H, W, Co, KH, KW, s, p = by[rid].geom
        assert (C * KH * KW, KH * KW) == (cols, taps)


def test_expected_calls_name_one_entry_point_per_pass():
    for row in ce.ALL_ROWS:
        want = ce.expected_calls(row)
        assert set(want) <= set(ce.LAUNCHES) and all(v == 1 for v in want.values())
        assert len(want) == 2 + (row.fam[2] != "none") + bool(row.act) + row.gated
        assert any(n.endswith("bwd_data") for n in want) == ("x" in row.grads)
    assert np.all([("_cl_" in n) == (f != "nchw") for (k, f), n in ce._ENTRY.items()])
