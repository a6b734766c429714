"""The two fused training steps (evae/fused_vae.py, evae/fused_std.py) ISSUE what they issued at the commit named in
tests/golden/g28_fused_step_traces.json: every C ABI call with its non-pointer arguments, which pointers were null and which
stream it went to; every stream wait and event record; every allocation with the stream current at it -- record for record, in
order (tests/step_trace.py).  A captured step replays without Python, so an equal recording of its capture is the same graph.

The one difference allowed: in the standard-prior cases evae_dense_bwd_data may have become evae_dense_bwd_data_wt with a null
wT -- the same launch (both are dense_bwd_data_core, csrc/evae_dense.hip).  Each case also asserts the entry points that mark
its branch, so that none passes by quietly taking another one.  Nothing here rewrites the golden.

The same holds the autograd Functions of evae/ops.py (the modular paths: hvae_2level steps, convolution layers, the gated
convolution stack, a residual run) to tests/golden/g29_modular_step_traces.json -- see MODULAR_MARKERS below."""
import json
import os

import pytest

import step_trace

pytestmark = pytest.mark.gpu

# case -> (entry points that must appear, entry points that must not)
MARKERS = {
    "eager_u8": (["evae_prior_elbo_fwd", "evae_elbo_bwd", "evae_gated_dense_fwd_u8"], []),
    "eager_fp32": (["evae_gated_dense_fwd"], ["evae_gated_dense_fwd_u8"]),
    "graphed_rows_c1000": (["evae_prior_train_step_rows", "evae_batch_prologue_u8_step"], []),
    "graphed_every_draw": (["evae_prior_train_step"], ["evae_prior_train_step_rows"]),
    "graphed_p6": (["evae_gated_dense_fwd_p6t", "evae_dense_bwd_data_p6t", "evae_dense_bwd_weight_p6"], []),
    "graphed_merge_0": ([], ["evae_reparam_logq_bwd_hardtanh_tail"]),
    "graphed_merge_15": (["evae_reparam_logq_bwd_hardtanh_tail"], []),
    "eager_approx_k10": (["evae_pairdist_topk", "evae_select_exemplars"], []),
    "std_graphed": (["evae_heads_reparam_std_fwd", "evae_heads_std_bwd", "evae_bernoulli_unit_step"], []),
    "std_eager": (["evae_elbo_bwd", "evae_bernoulli_sigmoid_bwd"], []),
    "std_eager_refused": (["evae_heads_reparam_fwd", "evae_log_normal_std_bwd"], []),
}
WT_ARG = 13       # evae_dense_bwd_data_wt's wT, behind evae_dense_bwd_data's ldo


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g28_fused_step_traces.json")) as f:
        return json.load(f)


def _same_launch(rec):
    """evae_dense_bwd_data_wt with a null wT, written as the evae_dense_bwd_data call it is"""
    if rec[0] == "call" and rec[1] == "evae_dense_bwd_data_wt" and rec[2][WT_ARG] == "null":
        return ["call", "evae_dense_bwd_data", rec[2][:WT_ARG] + rec[2][WT_ARG + 1:]]
    return rec


def test_the_cases_are_the_recorded_ones(recorded):
    assert set(recorded["cases"]) == set(step_trace.CASES) == set(MARKERS)
    assert len(recorded["commit"]) == 40


@pytest.mark.parametrize("case", sorted(MARKERS))
def test_step_issues_what_the_recorded_commit_issued(recorded, case):
    want = recorded["cases"][case]
    got = json.loads(json.dumps(step_trace.record(case)))
    names = {r[1] for r in got if r[0] == "call"}
    present, absent = MARKERS[case]
    assert all(m in names for m in present) and not any(m in names for m in absent), sorted(names)
    if case == "eager_fp32":            # the fp32 store's first layer gathers its rows through a row list
        assert any(r[2][1] == "ptr" for r in step_trace.calls(got, "evae_gated_dense_fwd"))
    if case.endswith("graphed") or case.startswith("graphed"):
        # the two replays issue no launch, no wait and no allocation: only the runner's upload of the next control block
        tail = got[[i for i, r in enumerate(got) if r == ["mark", "call 3"]][0]:]
        assert not [r for r in tail if r[0] in ("alloc", "wait_stream", "wait_event")
                    or (r[0] == "call" and str(r[2][-1]).startswith("s"))], tail
    if step_trace.CASES[case][1]:
        want, got = [_same_launch(r) for r in want], [_same_launch(r) for r in got]
    first = next((i for i, (a, b) in enumerate(zip(want, got)) if a != b), None)
    assert first is None, "record %d: recorded %s, issued %s" % (first, want[first], got[first])
    assert len(got) == len(want), (len(want), len(got))


# ---- the autograd Functions of evae/ops.py (tests/golden/g29_modular_step_traces.json, step_trace.MODULAR_CASES): the same
# comparison, evae_dense_bwd_data against evae_dense_bwd_data_wt with a null wT allowed in every case
_HVAE2 = ["evae_heads_reparam_fwd", "evae_heads_density_fwd", "evae_dense_bwd_weight_group"]
MODULAR_MARKERS = {
    "hvae2_u8": (_HVAE2 + ["evae_gated_dense_fwd_u8"], []),
    "hvae2_fp32": (_HVAE2, ["evae_gated_dense_fwd_u8"]),
    "hvae2_leaf": (_HVAE2 + ["evae_gated_dense_fwd_u8"], []),
    "conv_layers": (["evae_conv2d_fwd", "evae_conv2d_cl_fwd", "evae_conv2d_bwd_weight", "evae_conv2d_cl_bwd_weight", "evae_conv2d_bwd_data",
                     "evae_conv2d_cl_bwd_data", "evae_act_bwd"], []),
    "conv_stack": (["evae_cw_gate_bwd_image"], []),
    "res_run": (["evae_cw_res_run_fwd", "evae_cw_res_run_bwd"], []),
}


@pytest.fixture(scope="module")
def recorded_modular():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g29_modular_step_traces.json")) as f:
        return json.load(f)


def test_the_modular_cases_are_the_recorded_ones(recorded_modular):
    assert set(recorded_modular["cases"]) == set(step_trace.MODULAR_CASES) == set(MODULAR_MARKERS)
    assert len(recorded_modular["commit"]) == 40


def _launch_streams(records):
    return {r[2][-1] for r in records if r[0] == "call" and str(r[2][-1]).startswith("s")}


@pytest.mark.parametrize("case", sorted(MODULAR_MARKERS))
def test_modular_operators_issue_what_the_recorded_commit_issued(recorded_modular, case):
    want = recorded_modular["cases"][case]
    got = json.loads(json.dumps(step_trace.record(case)))
    names = {r[1] for r in got if r[0] == "call"}
    present, absent = MODULAR_MARKERS[case]
    assert all(m in names for m in present) and not any(m in names for m in absent), sorted(names)
    if case.startswith("hvae2"):
        groups = step_trace.calls(got, "evae_dense_bwd_weight_group")
        # the batch rows' second use of a weight the exemplar rows' GEMM made: added in place (ops._try_defer)
        assert any(job[5] == 1 for r in groups for job in r[3]), groups
        # ... and the scope's own grouped launches, behind the backward pass (ops.deferred_wgrads.__exit__)
        assert step_trace.calls(got[got.index(["mark", "deferred"]):], "evae_dense_bwd_weight_group")
        assert len(_launch_streams(got)) >= (3 if case == "hvae2_leaf" else 2), _launch_streams(got)
    want, got = [_same_launch(r) for r in want], [_same_launch(r) for r in got]
    first = next((i for i, (a, b) in enumerate(zip(want, got)) if a != b), None)
    assert first is None, "record %d: recorded %s, issued %s" % (first, want[first], got[first])
    assert len(got) == len(want), (len(want), len(got))
