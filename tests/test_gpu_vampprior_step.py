"""The VampPrior training step on the GPU: the captured step of `vae` and `hvae_2level` (evae/graph.py without exemplar rows,
utils/training.py::vampprior_step_eligible) against eager steps, and two epochs of train_one_epoch against the reference golden
G25.  The captured step issues the launches of the eager one (the prior through ops.MixtureLogP's forward / merge / backward
kernels in both), so the two trajectories are compared for bit equality; G25 is held to G13's bars."""
import copy

import numpy as np
import pytest
import torch

import golden_inputs as gi
import smoke_case

pytestmark = pytest.mark.gpu

PROLOGUE_BAR = 1e-5        # tests/test_gpu_model.py::test_graphed_step_matches_eager's, for the same comparison on the exemplar prior


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def host(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------ the captured step
N_ROWS, B_STEP, C_STEP, D_STEP, Z_STEP = 80, 16, 77, 64, 8


def _model(model_name, seed=2510, **kw):
    from utils.utils import importing_model
    cfg = dict(prior="vampprior", model_name=model_name, input_size=[1, 8, 8], hidden_size=32, z1_size=Z_STEP, z2_size=Z_STEP,
               number_components=C_STEP, training_set_size=N_ROWS, batch_size=B_STEP, pseudoinputs_mean=0.05, pseudoinputs_std=0.01,
               use_training_data_init=False, warmup=4, dynamic_binarization=False)
    cfg.update(kw)
    args = smoke_case.vae_args(**cfg)
    torch.manual_seed(seed)
    model = importing_model(args)(args).cuda()
    model.train()
    return args, model


class EpsFeed:
    """the model's noise hook over static buffers (a captured launch reads them at every replay): draw k of a step is buffer k"""

    def __init__(self, per_step):
        self.bufs = [torch.zeros((B_STEP, Z_STEP), device="cuda") for _ in range(per_step)]
        self.k = 0

    def __call__(self, like):
        buf = self.bufs[self.k % len(self.bufs)]
        self.k += 1
        assert tuple(buf.shape) == tuple(like.shape)
        return buf

    def load(self, eps_step):
        self.k = 0
        for buf, e in zip(self.bufs, eps_step):
            buf.copy_(torch.from_numpy(np.ascontiguousarray(e)))


class FeedingLoader:
    """a DataLoader that refills the noise buffers with step k's draws before it hands out batch k"""

    def __init__(self, loader, feed, eps, first_step):
        self.loader, self.feed, self.eps, self.first = loader, feed, eps, first_step
        self.dataset, self.batch_size = loader.dataset, loader.batch_size

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for k, batch in enumerate(self.loader):
            self.feed.load(self.eps[self.first + k])
            yield batch


def _dataset(seed):
    x = torch.from_numpy(gi.binary_images(seed, N_ROWS, D_STEP))
    return torch.utils.data.TensorDataset(x, torch.arange(N_ROWS).reshape(-1, 1), torch.zeros(N_ROWS))


@pytest.mark.parametrize("model_name", ["vae", "hvae_2level"])
def test_captured_step_matches_eager(model_name):
    """three warm-up calls, then four replays of the captured step, against seven eager steps of a copy of the model on the same
    batches and the same injected eps (betas that fp32 holds exactly: the control block carries beta as fp32); then beta changes between two replays without a re-capture"""
    from evae import ops
    from utils.optimizer import AdamNormGrad
    from utils.training import _graphed_step
    per_step = 1 if model_name == "vae" else 2
    ds = _dataset(2511)
    loader = torch.utils.data.DataLoader(ds, batch_size=B_STEP, shuffle=False)
    eps = np.random.RandomState(2512).standard_normal((7, per_step, B_STEP, Z_STEP)).astype(np.float32)
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
        out = runner(xb, ib, betas[it])
        got.append(out.tolist())
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


def test_vae_step_takes_its_noise_from_the_prologue():
    """a `vae` model without a noise hook: the captured step's eps is the counter-based draw of its prologue launch (seed = torch's
    seed when the runner is built, counter = the call number) -- the same draw handed to eager steps reproduces it"""
    from evae import ops
    from utils.optimizer import AdamNormGrad
    from utils.training import _graphed_step
    ds = _dataset(2513)
    loader = torch.utils.data.DataLoader(ds, batch_size=B_STEP, shuffle=False)
    args, model = _model("vae")
    _, twin = _model("vae")
    twin.load_state_dict(copy.deepcopy(model.state_dict()))
    opt = AdamNormGrad(model.parameters(), lr=5e-4)
    torch.manual_seed(3)
    runner = _graphed_step(args, model, opt, loader)
    assert runner.eps_buf is not None
    x_all, i_all = ds.tensors[0], ds.tensors[1]
    got = [runner(x_all[it * B_STEP:(it + 1) * B_STEP], i_all[it * B_STEP:(it + 1) * B_STEP], 0.5)[0].item() for it in range(5)]
    assert runner.graph is not None and not runner.failed and runner.replays == 2
    opt2 = AdamNormGrad(twin.parameters(), lr=5e-4)
    data = x_all.cuda()
    want = []
    for it in range(5):
        xb, ib = x_all[it * B_STEP:(it + 1) * B_STEP].cuda(), i_all[it * B_STEP:(it + 1) * B_STEP].cuda()
        e = torch.empty((B_STEP, Z_STEP), device="cuda")
        ops.batch_prologue(data, ib.reshape(-1).contiguous(), False, torch.tensor([3, it], dtype=torch.int64, device="cuda"),
                           torch.empty_like(xb), e)
        twin._draw_eps = lambda like, e=e: e
        opt2.zero_grad()
        loss, RE, KL = twin.calculate_loss((xb, ib), 0.5, average=True, dataset=ds)
        with ops.deferred_wgrads(loss):
            loss.backward()
        opt2.step()
        want.append(loss.item())
    print("prologue eps, captured vs eager:", rel(np.asarray(got), np.asarray(want)))
    assert rel(np.asarray(got), np.asarray(want)) < PROLOGUE_BAR


def test_hvae_step_without_a_noise_hook_draws_under_capture():
    """`hvae_2level` without an injected hook: z2 and z1 take torch.randn draws inside the captured step (the device generator is
    registered with the capture, every replay advances its offset) -- the step is captured, stays finite, the two latents do not
    share one draw, and no two replays see the same noise"""
    from utils.optimizer import AdamNormGrad
    from utils.training import _graphed_step
    ds = _dataset(2515)
    loader = torch.utils.data.DataLoader(ds, batch_size=B_STEP, shuffle=False)
    args, model = _model("hvae_2level")
    seen = []
    cls, had = type(model), "_draw_eps" in vars(type(model))
    plain = cls._draw_eps
    cls._draw_eps = lambda self, like: seen.append(plain(self, like)) or seen[-1]      # (class level: not an instance hook)
    try:
        assert "_draw_eps" not in model.__dict__
        runner = _graphed_step(args, model, AdamNormGrad(model.parameters(), lr=0.0), loader)
        assert runner.eps_buf is None
        xb, ib = ds.tensors[0][:B_STEP], ds.tensors[1][:B_STEP]
        outs = [runner(xb, ib, 0.5).tolist() for _ in range(6)]
    finally:
        if had:
            cls._draw_eps = plain
        else:
            del cls._draw_eps
    assert runner.graph is not None and not runner.failed and runner.replays == 3
    assert np.isfinite(np.asarray(outs)).all()
    # the capture's two draws (the last two recorded) are static buffers the replays refill: different from each other ...
    e2, e1 = seen[-2], seen[-1]
    assert e2.data_ptr() != e1.data_ptr() and not torch.equal(e2, e1) and bool(torch.isfinite(e1).all())
    assert 0.5 < float(e1.std()) < 1.5 and 0.5 < float(e2.std()) < 1.5
    # ... and, with the learning rate at zero and one batch, the noise is all that can move the loss between replays
    replayed = [o[0] for o in outs[3:]]
    assert len(set(replayed)) == 3, replayed


@pytest.mark.parametrize("model_name", ["vae", "hvae_2level"])
def test_epochs_match_reference_golden(golden, model_name):
    """G25: two epochs of train_one_epoch (five full batches each, beta 1/4 then 2/4) through the captured step"""
    from utils.optimizer import AdamNormGrad
    from utils.training import train_one_epoch
    g = golden("g25_vampprior_epochs")
    N, B, C, D, z, hidden, warmup = (int(v) for v in g["meta"])
    assert (N, B, C, D, z) == (N_ROWS, B_STEP, C_STEP, D_STEP, Z_STEP)
    args, model = _model(model_name, hidden_size=hidden, warmup=warmup)
    sd = {k[len(model_name) + 4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(model_name + "_sd_")}
    assert set(sd) == set(model.state_dict().keys())
    model.load_state_dict(sd)
    per_step = 1 if model_name == "vae" else 2
    feed = model._draw_eps = EpsFeed(per_step)
    ds = _dataset(251)
    loader = torch.utils.data.DataLoader(ds, batch_size=B, shuffle=False)
    opt = AdamNormGrad(model.parameters(), lr=float(g["lr"]))
    steps = N // B
    r1 = train_one_epoch(1, args, FeedingLoader(loader, feed, g["eps"], 0), model, opt)
    r2 = train_one_epoch(2, args, FeedingLoader(loader, feed, g["eps"], steps), model, opt)
    runners = list(model._graphed_steps.values())
    assert len(runners) == 1 and runners[0].graph is not None and not runners[0].failed and runners[0].by_index
    assert runners[0].replays == 2 * steps - runners[0].warmup_steps        # every step after the warm-up calls was a replay
    figs = (rel(np.asarray(r1), g[model_name + "_epoch1"]), rel(np.asarray(r2), g[model_name + "_epoch2"]))
    print("G25 %s: epochs %s" % (model_name, figs), r1, r2)
    assert figs[0] < 1e-4 and figs[1] < 1e-4
    for n, p in model.named_parameters():
        norm, total = float(g[model_name + "_norm_" + n]), float(g[model_name + "_sum_" + n])
        assert abs(p.detach().double().norm().item() - norm) <= 1e-4 * max(norm, 1e-3), n
        assert abs(p.detach().double().sum().item() - total) <= 2e-4 * max(norm, 1e-3), n


def test_other_configurations_keep_their_runner():
    from evae.graph import GraphedTrainStep
    from utils.optimizer import AdamNormGrad
    from utils.training import _graphed_step
    # an exemplar-prior `vae` next to it: its usual runner, exemplar rows and all
    Cx, Nx = 200, 500
    data = gi.binary_images(2514, Nx)
    ds = torch.utils.data.TensorDataset(torch.from_numpy(data), torch.arange(Nx).reshape(-1, 1), torch.zeros(Nx))
    args = smoke_case.vae_args(number_components=Cx, training_set_size=Nx, batch_size=16)
    from models.VAE import VAE
    model = VAE(args).cuda()
    loader = torch.utils.data.DataLoader(ds, batch_size=16, shuffle=False)
    runner = _graphed_step(args, model, AdamNormGrad(model.parameters(), lr=5e-4), loader)
    assert isinstance(runner, GraphedTrainStep) and not runner.no_exemplars
    assert (runner.lo, runner.hi) == (0, Cx) and runner.rows.numel() == runner._Cd + 16 and runner._Cd > 0
    # a convolutional model with the VampPrior steps eagerly
    cargs, cmodel = _model("convhvae_2level", input_size=[1, 28, 28], number_components=8)
    cds = torch.utils.data.TensorDataset(torch.from_numpy(data[:32]), torch.arange(32).reshape(-1, 1), torch.zeros(32))
    cloader = torch.utils.data.DataLoader(cds, batch_size=16, shuffle=False)
    assert _graphed_step(cargs, cmodel, AdamNormGrad(cmodel.parameters(), lr=5e-4), cloader) is None
    # ... and so does a dense one that was told not to capture
    vargs, vmodel = _model("vae")
    vargs.use_hip_graph = False
    assert _graphed_step(vargs, vmodel, AdamNormGrad(vmodel.parameters(), lr=5e-4), cloader) is None
