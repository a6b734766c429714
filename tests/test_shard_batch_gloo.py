"""Two gloo ranks on the CPU: the host side of the data-parallel sharded prior (args.shard_batch on the modular path,
evae/shard.py: gather_queries, gather_partials, own_columns).  Every rank holds its OWN five latents; the partials of all ten
queries against a rank's exemplar shard come from the oracle (the HIP kernels need a GPU), and the merge of a rank's own columns
must equal log p(z) of its five rows against ALL exemplars."""
import os
import sys
import traceback

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, ZD = 5, 40                     # rows per rank, latent size
SIZES = (33, 3)                   # exemplars: shards of 17 / 16, and of 2 / 1


def _case(C, world):
    """Latents of all ranks [world * B x z], exemplars [C x z], dataset indices of both.  Leave-one-out hits: query 0 (rank 0)
    names the LAST exemplar, which lies in rank 1's shard -- and exemplar 1 carries the same index (an index drawn twice; for
    C = 3 the two copies sit in different shards) --, queries B and B + 2 (rank 1) name exemplar 0, in rank 0's shard."""
    import golden_inputs as gi
    z, c = gi.clustered_latents(70 + C, world * B, C, ZD)
    ci = (100 + 3 * np.random.RandomState(C).permutation(C)).astype(np.int64)
    ci[1] = ci[C - 1]
    zi = (5000 + np.arange(world * B)).astype(np.int64)
    zi[0] = ci[C - 1]
    zi[B] = zi[B + 2] = ci[0]
    return z, c, zi, ci


def _worker(rank, world, port, q):
    try:
        for p in (os.path.join(ROOT, "exemplar-vae_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
            sys.path.insert(0, p)
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        try:
            import evae_oracle as orc
            from evae import shard
            T = torch.from_numpy
            out = []
            for C in SIZES:
                z, c, zi, ci = _case(C, world)
                lv = np.linspace(-0.9, -0.3, ZD).astype(np.float32)
                lo, hi = shard.bounds(C)
                mine = slice(rank * B, (rank + 1) * B)
                # the arrangement the case promises: a hit in the OTHER rank's shard for one of this rank's queries, a repeated index
                other = np.concatenate((ci[:lo], ci[hi:]))
                crossing = bool(np.isin(zi[mine], other).any())
                repeated = bool(len(np.unique(ci)) < C)
                for masked in (True, False):
                    z_all, zi_all = shard.gather_queries(T(z[mine].copy()), T(zi[mine].copy()) if masked else None)
                    assert z_all.shape == (world * B, ZD) and np.array_equal(z_all.numpy(), z)
                    assert (zi_all is None) if not masked else np.array_equal(zi_all.numpy(), zi)
                    m, s, n = orc.prior_partials(z_all.numpy(), zi_all.numpy() if masked else None, c[lo:hi], lv, ci[lo:hi], masked)
                    parts = shard.gather_partials(T(m), T(s), T(n))
                    assert parts[0].shape == (world, world * B)
                    om, os_, on = shard.own_columns(parts, B)
                    assert om.shape == (world, B) and om.data_ptr() == parts[0][:, rank * B:].data_ptr()      # views, not copies
                    merged = orc.prior_merge(om.numpy(), os_.numpy(), on.numpy(), C)
                    full = orc.log_p_z(z[mine], zi[mine], c, lv[None], ci, test=not masked)
                    out.append((C, masked, hi - lo, crossing, repeated, float(np.abs(merged - full).max() / np.abs(full).max()),
                                float(on.numpy().sum())))
            q.put((rank, out))
        finally:
            dist.destroy_process_group()
    except Exception:
        q.put((rank, traceback.format_exc()))
        raise


def _spawn2(target, port):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = [q.get(timeout=180) for _ in range(2)]
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.terminate()
    for rank, out in res:
        assert not isinstance(out, str), out
    for p in procs:
        assert p.exitcode == 0
    return res


def _worker_fn(rank, world, port, q):
    """ShardedPriorLogPBatch itself, forward and backward, with the oracle standing in for the three device kernels (the seam of
    tests/test_shard_gloo.py: the wrappers of evae.ops are replaced in this worker process)."""
    try:
        for p in (os.path.join(ROOT, "exemplar-vae_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
            sys.path.insert(0, p)
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        try:
            import evae_oracle as orc
            from evae import ops, shard
            T = torch.from_numpy

            def fwd(z, c, lv, zi, ci):
                masked = zi is not None and ci is not None
                m, s, n = orc.prior_partials(z.numpy(), None if zi is None else zi.numpy(), c.numpy(), lv.numpy(),
                                             None if ci is None else ci.numpy(), masked)
                return T(m), T(s), T(n), None

            def merge(m, s, n, c_total):
                assert m.shape == (world, B) and not m.is_contiguous()           # the own columns, where they lie
                m, s, n = m.numpy(), s.numpy(), n.numpy()
                mm = m.max(0)
                ls = np.log((s * np.exp(m - mm)).sum(0))
                return T(orc.prior_merge(m, s, n, c_total).astype(np.float32)), T(np.stack((mm, ls)).astype(np.float32))

            def bwd(z, c, lv, zi, ci, tok, g):
                z64, c64, lv64 = (t.numpy().astype(np.float64) for t in (z, c, lv))
                assert tok.shape == (2, len(z64)) and g.shape == (len(z64),)
                diff = z64[:, None, :] - c64[None, :, :]
                p = -0.5 * (lv64 + np.log(2 * np.pi)).sum() - 0.5 * (diff ** 2 * np.exp(-lv64)).sum(-1)
                if zi is not None and ci is not None:
                    p[zi.numpy().reshape(-1, 1) == ci.numpy().reshape(1, -1)] = -np.inf
                w = np.exp(p - tok.numpy().astype(np.float64).sum(0)[:, None]) * g.numpy().astype(np.float64)[:, None]
                dz = -(w[:, :, None] * diff * np.exp(-lv64)).sum(1)
                dc = (w[:, :, None] * diff * np.exp(-lv64)).sum(0)
                dlv = (w[:, :, None] * (-0.5 + 0.5 * diff ** 2 * np.exp(-lv64))).sum((0, 1))
                return T(dz.astype(np.float32)), T(dc.astype(np.float32)), T(dlv.astype(np.float32))
            ops.prior_lse_fwd, ops.prior_merge, ops.prior_lse_bwd = fwd, merge, bwd
            out = []
            for C in SIZES:
                z, c, zi, ci = _case(C, world)
                lv = np.linspace(-0.9, -0.3, ZD).astype(np.float32)
                gout = np.random.RandomState(9).standard_normal(world * B).astype(np.float32)      # every query its own upstream gradient
                lo, hi = shard.bounds(C)
                mine = slice(rank * B, (rank + 1) * B)
                for masked in (True, False):
                    zt = T(z[mine].copy()).requires_grad_(True); ct = T(c[lo:hi].copy()).requires_grad_(True)
                    lt = T(lv.copy()).requires_grad_(True)
                    lp = shard.ShardedPriorLogPBatch.apply(zt, ct, lt, T(zi[mine].copy()) if masked else None,
                                                           T(ci[lo:hi].copy()) if masked else None, C)
                    (lp * T(gout[mine])).sum().backward()
                    f64 = lambda a: a.astype(np.float64)
                    dz, dc, dlv, _ = orc.prior_grads(f64(z), zi, f64(c), f64(lv), ci, masked, f64(gout))
                    full = orc.log_p_z(z[mine], zi[mine], c, lv[None], ci, test=not masked)
                    dlv_sum = lt.grad.clone()
                    dist.all_reduce(dlv_sum)                # the Function leaves dlogvar un-reduced: the shards' parts add up to the whole
                    r = lambda a, b: float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
                    out.append((C, masked, r(lp.detach().numpy(), full), r(zt.grad.numpy(), dz[mine]),
                                r(ct.grad.numpy(), dc[lo:hi]),            # complete sums over all queries, NOT scaled by the world size
                                r(dlv_sum.numpy(), dlv)))
            q.put((rank, out))
        finally:
            dist.destroy_process_group()
    except Exception:
        q.put((rank, traceback.format_exc()))
        raise


def test_two_rank_data_parallel_prior_function_gloo():
    """forward = log p(z) of the own rows against all exemplars; backward = the gradients of sum over ALL ranks' queries of
    g_i log p(z_i): dz of the own rows, dcentres of the own shard unscaled, dlogvar in shard parts (bars of
    tests/test_shard_gloo.py's four-rank check of ShardedPriorLogP)"""
    for rank, out in _spawn2(_worker_fn, 35500 + (os.getpid() % 2000)):
        for C, masked, e_lp, e_dz, e_dc, e_dlv in out:
            assert e_lp < 2e-6 and e_dz < 2e-5 and e_dc < 2e-5 and e_dlv < 2e-5, (rank, C, masked, e_lp, e_dz, e_dc, e_dlv)


def test_two_rank_own_batches_merge_to_the_full_prior_gloo():
    res = _spawn2(_worker, 33500 + (os.getpid() % 2000))
    sizes = {}
    for rank, out in res:
        for C, masked, n_local, crossing, repeated, err, hits in out:
            sizes.setdefault(C, {})[rank] = n_local
            assert crossing and repeated, (rank, C)
            assert err < 2e-6, (rank, C, masked, err)           # the bar of tests/test_shard_gloo.py's merge check
            assert (hits > 0) == masked, (rank, C, masked, hits)
    assert sizes == {33: {0: 17, 1: 16}, 3: {0: 2, 1: 1}}
