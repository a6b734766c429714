"""Host side of the per-rank dropout noise of data-parallel batches (args.shard_batch): evae.ops.dropout_rng() mixes a
process-level salt into its seed.  Salt 0 -- the default, and what replicated sharding keeps -- is the seed of torch.manual_seed
unchanged; the rank is folded in with the constant the captured runner folds into its own seed (evae/graph.py)."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "exemplar-vae_amd"))
GOLDEN_RATIO_64 = 0x9E3779B97F4A7C15
M64 = 0xFFFFFFFFFFFFFFFF


@pytest.fixture
def ops():
    from evae import ops as o
    salt, calls = o.dropout_salt(), o._DROPOUT_CALLS[0]
    yield o
    o.dropout_salt(salt)
    o._DROPOUT_CALLS[0] = calls


def test_salt_zero_is_the_seed_of_torch_manual_seed(ops):
    torch.manual_seed(1234567)
    assert ops.dropout_salt() == 0                           # the default: nobody has stepped with shard_batch in this process
    seed, off = ops.dropout_rng()
    assert seed == int(torch.initial_seed()) & M64 == 1234567
    assert ops.dropout_rng() == (seed, off + 1)              # the counter still advances by one per mask


def test_two_salts_give_two_seeds_and_leave_the_counter_alone(ops):
    torch.manual_seed(99)
    seeds = []
    for rank in (0, 1, 7):
        ops.dropout_salt(ops.rank_salt(rank))
        seeds.append(ops.dropout_rng())
    assert len({s for s, _ in seeds}) == 3
    assert [o for _, o in seeds] == [seeds[0][1] + i for i in range(3)]
    ops.dropout_salt(0)
    assert ops.dropout_rng()[0] == 99


def test_the_rank_is_folded_with_the_runners_constant(ops):
    assert ops.RANK_SALT == GOLDEN_RATIO_64
    for rank in (0, 1, 7):
        assert ops.rank_salt(rank) == (GOLDEN_RATIO_64 * (rank + 1)) & M64
    torch.manual_seed(5)
    ops.dropout_salt(ops.rank_salt(3))
    assert ops.dropout_rng()[0] == (5 + GOLDEN_RATIO_64 * 4) & M64
    # the captured runner's seed takes the same fold: one statement of the constant for both
    src = open(os.path.join(ROOT, "exemplar-vae_amd", "evae", "graph.py")).read()
    assert "ops.RANK_SALT * (shard.world()[0] + 1)" in src and "0x9E37" not in src


def test_fold_rank_into_noise_sets_the_salt_once(ops, monkeypatch):
    from evae import shard
    monkeypatch.setattr(shard, "_NOISE_FOLDED", [False])
    monkeypatch.setattr(shard.dist, "get_rank", lambda group=None: 1)
    shard.fold_rank_into_noise()
    assert ops.dropout_salt() == ops.rank_salt(1)
    ops.dropout_salt(0)
    shard.fold_rank_into_noise()                             # once per process
    assert ops.dropout_salt() == 0
