"""The standard-normal prior on the GPU: the two latent kernels of csrc/evae_latent_std.hip against float64 (tests/standard_ref.py),
the one-node `vae` step of evae/fused_std.py against float64, the captured step of `vae` and `hvae_2level` against eager steps
(tests/test_gpu_vampprior_step.py's harness) and against the reference golden G26, and the promise that the node runs on one stream."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import golden_inputs as gi
import smoke_case
import standard_ref as sr
from test_gpu_vampprior_step import EpsFeed, FeedingLoader, N_ROWS, B_STEP, D_STEP, Z_STEP

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def vp(t):
    return None if t is None else C.c_void_p(t if isinstance(t, int) else t.data_ptr())


def nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------ the two kernels
# (M, K, Z, ldx): the batch of the flagship step, a row count that is no multiple of the 16-row tile, one row tile with Z < 16
# (the tiled GEMMs serve the launches the backward kernel replaces), one row with Z not a multiple of 4, and rows of x inside a
# wider buffer
SHAPES = [(100, 300, 40, 300), (37, 300, 40, 300), (5, 48, 8, 48), (1, 20, 6, 20), (21, 64, 12, 72)]


@functools.lru_cache(maxsize=None)
def latent_case(M, K, Z, ldx):
    """inputs (fp32) and the float64 reference of both kernels for one shape, computed once and shared by the tests.  Weights scaled
    as in tests/test_gpu_kernels.py::test_heads_and_sample_in_one_call (wl x 0.5); the seed is the first one whose pre-activations
    reach both ends of the Hardtanh (a property of the inputs: the one-row shape has six of them)."""
    for seed in range(M + K, M + K + 2000):
        rs = np.random.RandomState(seed)
        x = rs.standard_normal((M, K)).astype(np.float32)
        wm = (rs.standard_normal((Z, K)) * 0.1).astype(np.float32); bm = (rs.standard_normal(Z) * 0.1).astype(np.float32)
        wl = (rs.standard_normal((Z, K)) * 0.5).astype(np.float32); bl = (rs.standard_normal(Z) * 0.5).astype(np.float32)
        eps = rs.standard_normal((M, Z)).astype(np.float32)
        fwd = sr.heads_forward(x, wm, bm, wl, bl, eps)
        if (fwd["pre"] < -6.01).any() and (fwd["pre"] > 2.01).any() and ((fwd["pre"] > -5.9) & (fwd["pre"] < 1.9)).any():
            break
    else:
        raise AssertionError("no seed reaches both ends of the Hardtanh")
    # the backward's inputs: what a forward pass saved (fp32), a decoder gradient whose rows span scales, per-row coefficients
    # with a zero row, the saved output and gate of the layer below
    sav = {k: fwd[k].astype(np.float32) for k in ("mean", "pre", "lv", "z")}
    dz = (rs.standard_normal((M, Z)) * np.exp(rs.uniform(-6, 2, (M, 1)))).astype(np.float32)
    cKL = rs.uniform(0.05, 1.5, M).astype(np.float32)
    if M > 1:
        cKL[M // 2] = 0.0
    a_prev = rs.standard_normal((M, K)).astype(np.float32); s_prev = rs.random_sample((M, K)).astype(np.float32)
    bwd = sr.heads_backward(sav["lv"], sav["pre"], eps, sav["z"], dz, cKL, wm, wl, a_prev, s_prev)
    return dict(x=x, wm=wm, bm=bm, wl=wl, bl=bl, eps=eps, fwd=fwd, sav=sav, dz=dz, cKL=cKL, a_prev=a_prev, s_prev=s_prev, bwd=bwd)


@pytest.mark.parametrize("M,K,Z,ldx", SHAPES)
def test_heads_sample_and_both_densities_in_one_launch(M, K, Z, ldx):
    """evae_heads_reparam_std_fwd against float64 at the bars of test_heads_and_sample_in_one_call (logp: a row sum of logq's kind,
    logq's bar), outputs NaN-filled before the launch; bit-equal to evae_heads_reparam_fwd_bcast where that applies too."""
    from evae import _lib
    lib = _lib.load()
    c = latent_case(M, K, Z, ldx)
    f = c["fwd"]
    assert (f["pre"] < -6.0).any() and (f["pre"] > 2.0).any()                    # both ends of the Hardtanh are hit
    assert lib.evae_heads_std_applies(M, K, Z, ldx) == 1
    xw = torch.zeros((M, ldx), device="cuda")
    xw[:, :K] = dev(c["x"])
    t = {k: dev(c[k]) for k in ("wm", "bm", "wl", "bl", "eps")}

    def launch(bcast):
        o = {k: nan(M, Z) for k in ("mean", "pre", "lv", "z")}
        o["logq"] = nan(M)
        head = (vp(xw), M, K, ldx, vp(t["wm"]), vp(t["bm"]), vp(t["wl"]), vp(t["bl"]), Z, -6.0, 2.0, vp(t["eps"]), vp(o["mean"]),
                vp(o["pre"]), vp(o["lv"]), vp(o["z"]), vp(o["logq"]))
        if bcast:
            src, dst = torch.full((1,), 0.5, device="cuda"), nan(Z)
            _lib.check(lib.evae_heads_reparam_fwd_bcast(*head, vp(src), vp(dst), Z, st()), "heads_reparam_fwd_bcast")
        else:
            o["logp"] = nan(M)
            _lib.check(lib.evae_heads_reparam_std_fwd(*head, vp(o["logp"]), st()), "heads_reparam_std_fwd")
        return o
    o = launch(False)
    figs = {k: rel(host(o[k]), f[k]) for k in ("mean", "pre", "z", "logq", "logp")}
    figs["lv"] = np.abs(host(o["lv"]) - f["lv"]).max() / np.abs(f["pre"]).max()
    print("std heads forward", (M, K, Z, ldx), {k: "%.2e" % v for k, v in figs.items()})
    assert all(bool(torch.isfinite(v).all()) for v in o.values())
    assert figs["mean"] < 2e-6 and figs["pre"] < 2e-6
    assert figs["lv"] < 2e-6 and figs["z"] < 5e-6
    assert figs["logq"] < 5e-6 and figs["logp"] < 5e-6
    if lib.evae_heads_reparam_fwd_bcast_applies(M, K, Z, ldx):
        b = launch(True)
        for k in ("mean", "pre", "lv", "z", "logq"):
            assert torch.equal(o[k], b[k]), k
    else:
        assert (M, K, Z, ldx) not in SHAPES[:2]


@pytest.mark.parametrize("M,K,Z,ldx", SHAPES)
def test_latent_backward_in_one_launch(M, K, Z, ldx):
    """evae_heads_std_bwd against float64.  dmu / dlv_pre at the 1e-4 of test_reparam_logq_and_densities, exact zeros outside the
    Hardtanh's open interval.  [dh | dg]: the existing test of evae_dense_bwd_data_timg holds this product to the BITS of
    evae_dense_bwd_data on the same (dmu, dlv_pre) -- asserted wherever the thin kernel serves that launch (Z a multiple of 4, >= 16;
    the tiled GEMM sums in another order: 2e-6, the fp32-against-fp32 bar of tests/test_gpu_kernels.py) -- and to float64 at the 1e-5
    test_linear_fwd_bwd holds a data gradient to."""
    from evae import _lib
    lib = _lib.load()
    c = latent_case(M, K, Z, ldx)
    s = c["sav"]
    t = {k: dev(v) for k, v in dict(mean=s["mean"], lv=s["lv"], pre=s["pre"], z=s["z"], eps=c["eps"], dz=c["dz"], cKL=c["cKL"],
                                    neg=-c["cKL"], wm=c["wm"], wl=c["wl"], a=c["a_prev"], s=c["s_prev"]).items()}
    dhd, dq = nan(M, 2 * Z), nan(M, 2 * K)
    _lib.check(lib.evae_heads_std_bwd(vp(t["mean"]), vp(t["lv"]), vp(t["pre"]), vp(t["eps"]), vp(t["z"]), vp(t["dz"]), vp(t["cKL"]),
                                      vp(t["neg"]), -6.0, 2.0, M, Z, vp(t["wm"]), vp(t["wl"]), K, vp(t["a"]), vp(t["s"]), vp(dhd),
                                      vp(dhd.data_ptr() + 4 * Z), 2 * Z, vp(dq), vp(dq.data_ptr() + 4 * K), 2 * K, st()), "heads_std_bwd")
    assert bool(torch.isfinite(dhd).all()) and bool(torch.isfinite(dq).all())
    rdmu, rdlp, rdh, rdg = c["bwd"]
    dmu, dlp = host(dhd[:, :Z]), host(dhd[:, Z:])
    figs = dict(dmu=rel(dmu, rdmu), dlv_pre=rel(dlp, rdlp), dh=rel(host(dq[:, :K]), rdh), dg=rel(host(dq[:, K:]), rdg))
    print("std latent backward", (M, K, Z), {k: "%.2e" % v for k, v in figs.items()})
    assert figs["dmu"] < 1e-4 and figs["dlv_pre"] < 1e-4
    outside = (s["pre"] <= -6.0) | (s["pre"] >= 2.0)
    assert outside.any() and (dlp[outside] == 0.0).all() and (dlp[~outside] != 0.0).any()
    assert figs["dh"] < 1e-5 and figs["dg"] < 1e-5
    # the two launches it replaces, on the kernel's own (dmu, dlv_pre)
    two = nan(M, 2 * K)
    nb = lib.evae_dense_bwd_data_workspace_bytes(M, Z, K, 2)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    mu_c, lp_c = dhd[:, :Z].contiguous(), dhd[:, Z:].contiguous()
    _lib.check(lib.evae_dense_bwd_data(vp(mu_c), vp(t["wm"]), vp(lp_c), vp(t["wl"]), M, Z, Z, K, vp(t["a"]), vp(t["s"]), vp(two),
                                       vp(two.data_ptr() + 4 * K), 2 * K, vp(ws), nb, st()), "dense_bwd_data")
    if Z % 4 == 0 and Z >= 16:
        assert torch.equal(dq, two)
    else:
        assert rel(host(dq), host(two)) < 2e-6


# ------------------------------------------------------------------------------------------------ the node
def _model(model_name, seed=2610, **kw):
    from utils.utils import importing_model
    cfg = dict(prior="standard", model_name=model_name, input_size=[1, 8, 8], hidden_size=32, z1_size=Z_STEP, z2_size=Z_STEP,
               number_components=1, training_set_size=N_ROWS, batch_size=B_STEP, warmup=4, dynamic_binarization=False)
    cfg.update(kw)
    args = smoke_case.vae_args(**cfg)
    torch.manual_seed(seed)
    model = importing_model(args)(args).cuda()
    model.train()
    return args, model


def _dataset(seed, n=N_ROWS):
    x = torch.from_numpy(gi.binary_images(seed, n, D_STEP))
    return torch.utils.data.TensorDataset(x, torch.arange(n).reshape(-1, 1), torch.zeros(n))


def _node_against_ref(model, sd, x, eps, beta, average, loss_bar):
    model.zero_grad(set_to_none=True)
    model._draw_eps = lambda like: dev(eps)
    B = x.shape[0]
    loss, RE, KL = model.calculate_loss((dev(x), torch.arange(B).reshape(-1, 1).cuda()), beta, average=average)
    assert "VaeStandardLoss" in type(loss.grad_fn).__name__
    (loss if average else loss.mean()).backward()
    (rl, rr, rk), rg = sr.step(sd, x, eps, beta, average=average)
    figs = dict(loss=rel(host(loss), rl), RE=rel(host(RE), rr), KL=rel(host(KL), rk))
    gfig = {}
    for n, p in model.named_parameters():
        ref = float(np.sqrt((rg[n] ** 2).sum()))
        gfig[n] = abs(p.grad.double().norm().item() - ref) / max(ref, 1e-6)
    print("std node B=%d beta=%s average=%s:" % (B, beta, average), {k: "%.2e" % v for k, v in figs.items()},
          "worst gradient norm %s" % (max(gfig.items(), key=lambda kv: kv[1]),))
    assert max(figs.values()) < loss_bar, figs
    assert max(gfig.values()) <= 1e-3, gfig
    return loss


@pytest.mark.parametrize("average", [True, False])
@pytest.mark.parametrize("beta", [0.25, 1.0])
def test_node_matches_float64_at_g26_sizes(golden, beta, average):
    """one step of the `vae` node on G26's initial weights, first batch and first injected eps against tests/standard_ref.py, at
    the bars tests/test_gpu_vampprior.py::test_models_match_reference_golden holds the VampPrior models to (1e-4; 1e-3 by norm)"""
    g = golden("g26_standard_epochs")
    args, model = _model("vae")
    sd = {k[len("vae_sd_"):]: g[k] for k in g.files if k.startswith("vae_sd_")}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    x = gi.binary_images(int(g["seed"]), N_ROWS, D_STEP)[:B_STEP]
    _node_against_ref(model, sd, x, g["eps"][0, 0], beta, average, 1e-4)


def test_a_refused_size_takes_the_existing_launches():
    """M = 2000 rows: evae_heads_std_applies says no, the node composes evae_heads_reparam_fwd + the row density kernels (and, past
    128 rows, single weight-gradient launches), nothing raises, and the loss holds the forward kernel's bar against float64"""
    from evae import _lib
    lib = _lib.load()
    B = 2000
    assert lib.evae_heads_std_applies(B, 300, 40, 300) == 0 and lib.evae_heads_std_applies(B, 32, Z_STEP, 32) == 0
    assert lib.evae_heads_std_applies(100, 300, 40, 300) == 1
    args, model = _model("vae", batch_size=B)
    sd = {k: host(v) for k, v in model.state_dict().items()}
    x = gi.binary_images(2611, B, D_STEP)
    eps = np.random.RandomState(2612).standard_normal((B, Z_STEP)).astype(np.float32)
    _node_against_ref(model, sd, x, eps, 0.5, False, 5e-6)


def test_the_node_stays_on_one_stream(monkeypatch):
    """while the `vae` node runs, forward and backward, nobody asks for the model's second stream"""
    from evae import ops
    calls = []
    plain = ops.model_side_stream
    monkeypatch.setattr(ops, "model_side_stream", lambda device: calls.append(device) or plain(device))
    args, model = _model("vae")
    x = dev(gi.binary_images(2613, B_STEP, D_STEP))
    loss, RE, KL = model.calculate_loss((x, torch.arange(B_STEP).reshape(-1, 1).cuda()), 0.5, average=True)
    assert "VaeStandardLoss" in type(loss.grad_fn).__name__
    loss.backward()
    torch.cuda.synchronize()
    assert calls == []
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())


# ------------------------------------------------------------------------------------------------ the captured step
@pytest.mark.parametrize("model_name", ["vae", "hvae_2level"])
def test_captured_step_matches_eager(model_name):
    """tests/test_gpu_vampprior_step.py::test_captured_step_matches_eager with --prior standard: three warm-up calls, four replays,
    against seven eager steps of a twin on the same batches and injected eps; then beta changes between replays without a re-capture"""
    from evae import ops
    from utils.optimizer import AdamNormGrad
    from utils.training import _graphed_step
    per_step = 1 if model_name == "vae" else 2
    ds = _dataset(2614)
    loader = torch.utils.data.DataLoader(ds, batch_size=B_STEP, shuffle=False)
    eps = np.random.RandomState(2615).standard_normal((7, per_step, B_STEP, Z_STEP)).astype(np.float32)
    args, model = _model(model_name)
    _, twin = _model(model_name)
    twin.load_state_dict(copy.deepcopy(model.state_dict()))
    betas = [0.25, 0.25, 0.5, 0.5, 0.5, 0.75, 1.0]
    x_all, i_all = ds.tensors[0], ds.tensors[1]
    batch = lambda it: (x_all[(it % 5) * B_STEP:(it % 5 + 1) * B_STEP], i_all[(it % 5) * B_STEP:(it % 5 + 1) * B_STEP])

    feed = model._draw_eps = EpsFeed(per_step)
    opt = AdamNormGrad(model.parameters(), lr=5e-4)
    runner = _graphed_step(args, model, opt, loader)
    assert runner is not None and runner.no_exemplars and runner.hi == runner.lo == 0
    got = []
    for it in range(7):
        feed.load(eps[it])
        xb, ib = batch(it)
        got.append(runner(xb, ib, betas[it]).tolist())
        if it == 2:
            assert runner.graph is None and runner.replays == 0            # the warm-up calls
    assert runner.graph is not None and not runner.failed and runner.by_index
    assert runner.replays == 4

    feed2 = twin._draw_eps = EpsFeed(per_step)
    opt2 = AdamNormGrad(twin.parameters(), lr=5e-4)
    want = []
    for it in range(7):
        feed2.load(eps[it])
        xb, ib = (t.cuda() for t in batch(it))
        opt2.zero_grad()
        loss, RE, KL = twin.calculate_loss((xb, ib), betas[it], average=True, dataset=ds)
        with ops.deferred_wgrads(loss):
            loss.backward()
        opt2.step()
        want.append([loss.item(), -RE.item(), KL.item()])
    got, want = np.asarray(got), np.asarray(want)
    figs = {k: rel(got[:, i], want[:, i]) for i, k in enumerate(("loss", "-RE", "KL"))}
    pfig = {n: rel(host(p), host(q)) for (n, p), (_, q) in zip(model.named_parameters(), twin.named_parameters())}
    print("captured vs eager %s: %s  worst parameter %s" % (model_name, {k: "%.2e" % v for k, v in figs.items()},
                                                           max(pfig.items(), key=lambda kv: kv[1])))
    # the same launches on the same inputs, replayed or issued one by one: the same bits
    assert np.array_equal(got, want), figs
    for (n, p), (_, q) in zip(model.named_parameters(), twin.named_parameters()):
        assert torch.equal(p, q), (n, pfig[n])

    # beta is a field of the control block: two replays on one batch and one noise, two betas, one graph
    graph = runner.graph
    xb, ib = batch(0)
    outs = []
    for beta in (0.3, 0.9):
        feed.load(eps[0])
        outs.append((beta, runner(xb, ib, beta).tolist()))
    assert runner.graph is graph and runner.replays == 6
    for beta, (loss, neg_re, kl) in outs:
        assert abs(loss - (neg_re + beta * kl)) <= 1e-5 * abs(loss), (beta, loss, neg_re, kl)
    assert abs(outs[0][1][2]) > 1e-3 and outs[0][1][0] != outs[1][1][0]


@pytest.mark.parametrize("model_name", ["vae", "hvae_2level"])
def test_epochs_match_reference_golden(golden, model_name):
    """G26: two epochs of train_one_epoch (five full batches each, beta 1/4 then 2/4) through the captured step, at G25's bars"""
    from utils.optimizer import AdamNormGrad
    from utils.training import train_one_epoch
    g = golden("g26_standard_epochs")
    N, B, D, z, hidden, warmup = (int(v) for v in g["meta"])
    assert (N, B, D, z) == (N_ROWS, B_STEP, D_STEP, Z_STEP)
    args, model = _model(model_name, hidden_size=hidden, warmup=warmup)
    sd = {k[len(model_name) + 4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(model_name + "_sd_")}
    assert set(sd) == set(model.state_dict().keys())
    model.load_state_dict(sd)
    per_step = 1 if model_name == "vae" else 2
    feed = model._draw_eps = EpsFeed(per_step)
    ds = _dataset(int(g["seed"]))
    loader = torch.utils.data.DataLoader(ds, batch_size=B, shuffle=False)
    opt = AdamNormGrad(model.parameters(), lr=float(g["lr"]))
    steps = N // B
    r1 = train_one_epoch(1, args, FeedingLoader(loader, feed, g["eps"], 0), model, opt)
    r2 = train_one_epoch(2, args, FeedingLoader(loader, feed, g["eps"], steps), model, opt)
    runners = list(model._graphed_steps.values())
    assert len(runners) == 1 and runners[0].graph is not None and not runners[0].failed and runners[0].by_index
    assert runners[0].no_exemplars
    assert runners[0].replays == 2 * steps - runners[0].warmup_steps        # every step after the warm-up calls was a replay
    figs = (rel(np.asarray(r1), g[model_name + "_epoch1"]), rel(np.asarray(r2), g[model_name + "_epoch2"]))
    print("G26 %s: epochs %s" % (model_name, figs), r1, r2)
    assert figs[0] < 1e-4 and figs[1] < 1e-4
    for n, p in model.named_parameters():
        norm, total = float(g[model_name + "_norm_" + n]), float(g[model_name + "_sum_" + n])
        assert abs(p.detach().double().norm().item() - norm) <= 1e-4 * max(norm, 1e-3), n
        assert abs(p.detach().double().sum().item() - total) <= 2e-4 * max(norm, 1e-3), n
