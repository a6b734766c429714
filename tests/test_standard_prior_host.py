"""CPU-only checks around the captured standard-normal-prior training step: golden G26 (tools/gen_goldens.py::g26, two epochs of the
reference's train_one_epoch for `vae` and `hvae_2level` with --prior standard) is what the GPU test expects it to be, and the
eligibility predicates of utils/training.py are functions of the arguments."""
import itertools
from argparse import Namespace

import numpy as np
import pytest

MODELS = ("vae", "hvae_2level")


def test_g26_has_the_documented_keys(golden):
    g = golden("g26_standard_epochs")
    N, B, D, z, hidden, warmup = (int(v) for v in g["meta"])
    assert (N, B, D, z, hidden, warmup) == (80, 16, 64, 8, 32, 4)                 # G25's sizes, five full batches per epoch
    steps = 2 * (N // B)
    assert g["eps"].shape == (steps, 2, B, z) and g["eps"].dtype == np.float32
    assert float(g["lr"]) == 5e-4
    for tag in MODELS:
        assert g[tag + "_epoch1"].shape == (3,) and g[tag + "_epoch2"].shape == (3,)
        sd = {k[len(tag) + 4:] for k in g.files if k.startswith(tag + "_sd_")}
        final = {k[len(tag) + 6:] for k in g.files if k.startswith(tag + "_norm_")}
        assert final == {k[len(tag) + 5:] for k in g.files if k.startswith(tag + "_sum_")}
        assert "q_z_mean.weight" in sd and g[tag + "_sd_q_z_mean.weight"].shape == (z, hidden)
        assert not any(k.startswith("means.") or k == "prior_log_variance" for k in sd)     # no parameter of another prior
        assert final and final <= sd                                              # every trained parameter has its initial value
        moved = 0
        for n in final:
            a = g[tag + "_sd_" + n].astype(np.float64)
            norm, total = float(g[tag + "_norm_" + n]), float(g[tag + "_sum_" + n])
            assert np.isfinite(norm) and np.isfinite(total) and abs(total) <= norm * np.sqrt(a.size) * (1 + 1e-9)
            moved += abs(np.sqrt((a * a).sum()) - norm) > 1e-6 * max(norm, 1e-3)
        assert moved > len(final) // 2                                            # two epochs of training moved the parameters


def test_g26_epochs_are_finite_and_tied_by_beta(golden):
    g = golden("g26_standard_epochs")
    for tag in MODELS:
        e1, e2 = g[tag + "_epoch1"], g[tag + "_epoch2"]
        assert np.isfinite(e1).all() and np.isfinite(e2).all()
        # train_one_epoch returns (loss, -RE, KL) averaged over the batches, loss = -RE + beta KL per batch: with ONE beta per
        # epoch the three are tied by it -- 1/4 in the first epoch, 2/4 in the second (warmup = 4)
        for e, beta in ((e1, 0.25), (e2, 0.5)):
            assert abs(e[0] - (e[1] + beta * e[2])) <= 1e-5 * abs(e[0])


def test_the_vae_nodes_parameter_order_is_the_goldens_state_dict(golden):
    from evae import fused_std
    g = golden("g26_standard_epochs")
    sd = {k[len("vae_sd_"):] for k in g.files if k.startswith("vae_sd_")}
    assert set(fused_std.PARAM_ORDER) == sd and len(fused_std.PARAM_ORDER) == len(sd)
    assert "prior_log_variance" not in fused_std.PARAM_ORDER


GRID = list(itertools.product(("vae", "hvae_2level", "convhvae_2level", "single_conv"), ("standard", "vampprior", "exemplar_prior"),
                              (False, True)))


@pytest.mark.parametrize("model_name,prior,sharded", GRID)
def test_standard_eligibility_is_a_function_of_the_arguments(model_name, prior, sharded):
    from utils.training import standard_step_eligible
    want = prior == "standard" and model_name in ("vae", "hvae_2level") and not sharded
    a = Namespace(model_name=model_name, prior=prior, shard_exemplars=sharded, number_components=500)
    assert standard_step_eligible(a) is want
    if not sharded:
        del a.shard_exemplars                      # a configuration that never heard of sharding is an unsharded one
        assert standard_step_eligible(a) is want


@pytest.mark.parametrize("model_name,prior,sharded", GRID)
def test_vampprior_eligibility_is_unchanged(model_name, prior, sharded):
    from utils.training import vampprior_step_eligible
    a = Namespace(model_name=model_name, prior=prior, shard_exemplars=sharded, number_components=500)
    assert vampprior_step_eligible(a) is (prior == "vampprior" and model_name in ("vae", "hvae_2level") and not sharded)
