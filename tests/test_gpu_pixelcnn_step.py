"""The captured pixelcnn training step on the GPU (utils/training.py::pixelcnn_step_eligible, evae/graph.py): the device-sourced
dropout launches of csrc/evae_attn.hip against the host-argument ones and against the mask restatement of tests/pixelsnail_ref.py,
the replayed step against the same step issued launch by launch, masks that move from replay to replay, one replayed step without
dropout against the float64 restatement of the model, and the routing of utils/training.py::_graphed_step."""
import copy
import ctypes
import types

import numpy as np
import pytest
import torch

import golden_inputs as gi
import pixelsnail_ref as psr
import smoke_case
from test_gpu_pixelsnail import assert_all, close        # the tolerance of test_model_loss_and_gradients_match_ref, not a copy of it

pytestmark = pytest.mark.gpu

SEED = 0x1234567887654321                 # < 2^63 (the control block holds it as int64), both halves in use
COUNTERS = (0x100000003, 7)               # the first reaches past bit 47 of the offset
ORDINALS = (5, 65535)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def seed_ctr(counter, seed=SEED):
    return torch.tensor([seed, counter], dtype=torch.int64, device="cuda")


@pytest.fixture(scope="module")
def ops():
    from evae import ops as o
    return o


# ---- 1. the masks of the device-sourced launches --------------------------------------------------------------------------
def _elu_run(ops, x, go, p, rng):
    xt = dev(x).requires_grad_(True)
    y = ops.elu_dropout(xt, p, rng=rng)
    y.backward(dev(go))
    return y.detach(), xt.grad


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027])
def test_elu_dropout_dev_is_the_host_mask_at_the_step_offset(ops, n, p):
    rs = np.random.RandomState(2800 + n)
    x, go = (rs.randn(n) * 2).astype(np.float32), rs.randn(n).astype(np.float32)
    assert (x != 0).all() and (go != 0).all()
    counter, ordinal = COUNTERS[0], ORDINALS[0]
    offset = ops.dropout_step_offset(counter, ordinal)
    y_dev, dx_dev = _elu_run(ops, x, go, p, ops.StepRng(seed_ctr(counter), ordinal))
    y_host, dx_host = _elu_run(ops, x, go, p, (SEED, offset))
    assert torch.equal(y_dev, y_host) and torch.equal(dx_dev, dx_host)                 # forward and backward: the same bits
    keep = psr.flat_keep_mask(n, p, SEED, offset)
    assert np.array_equal(host(y_dev) != 0, keep) and np.array_equal(host(dx_dev) != 0, keep)      # element for element


def test_elu_dropout_dev_masks_differ_by_counter_and_ordinal(ops):
    n, p = 1027, 0.5
    x = (np.random.RandomState(2810).randn(n) * 2).astype(np.float32)
    xt = dev(x)
    kept = {}
    for c in COUNTERS:
        for o in ORDINALS:
            kept[c, o] = host(ops.elu_dropout(xt, p, rng=ops.StepRng(seed_ctr(c), o))) != 0
            assert np.array_equal(kept[c, o], psr.flat_keep_mask(n, p, SEED, ops.dropout_step_offset(c, o)))
    keys = sorted(kept)
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            assert not np.array_equal(kept[a], kept[b]), (a, b)
    # the same (counter, ordinal) under another seed word is another mask too
    assert not np.array_equal(kept[keys[0]], host(ops.elu_dropout(xt, p, rng=ops.StepRng(seed_ctr(keys[0][0], SEED ^ 1), keys[0][1]))) != 0)


def test_dev_launch_without_dropout_never_reads_the_block(ops):
    """p_drop = 0 through the *_dev entry points with a NULL block: the plain ELU, the plain attention"""
    from evae import _lib
    lib = _lib.load()
    x = dev((np.random.RandomState(2811).randn(1027) * 2).astype(np.float32))
    out = torch.empty_like(x)
    _lib.check(lib.evae_elu_dropout_fwd_dev(ops._p(x), x.numel(), 0.0, None, 0, ops._p(out), ops._stream()), "evae_elu_dropout_fwd_dev")
    assert torch.equal(out, ops.elu_dropout(x))
    B, H, L = 1, 3, 2
    q, k, v = (dev(np.random.RandomState(2812 + i).randn(B * L, H * 4).astype(np.float32)) for i in range(3))
    o, lse = torch.empty_like(q), torch.empty((B, H, L), device="cuda")
    _lib.check(lib.evae_causal_attn_fwd_dev(ops._p(q), ops._p(k), ops._p(v), B, H, L, 4, 0.0, None, 0, ops._p(o), ops._p(lse),
                                            ops._stream()), "evae_causal_attn_fwd_dev")
    assert torch.equal(o, ops.causal_attn(q, k, v, B, L, H))


# (B, H, L): the two smallest shapes of test_gpu_pixelsnail.ATTN_SHAPES whose rows draw anything (L > 1), and H = 8 heads of dh = 4
# at an L that is no multiple of the 256 rows a workgroup takes in one round
ATTN_DEV_SHAPES = [(1, 3, 2), (5, 1, 65), (2, 8, 65)]


def _attn_run(ops, q, k, v, go, B, H, L, p, rng):
    t = [dev(a).requires_grad_(True) for a in (q, k, v)]
    out = ops.causal_attn(*t, B, L, H, p, rng=rng)
    out.backward(dev(go))
    return [out.detach()] + [a.grad for a in t]


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("B,H,L", ATTN_DEV_SHAPES)
def test_causal_attn_dev_is_the_host_mask_at_the_step_offset(ops, B, H, L, p):
    rs = np.random.RandomState(2820 + B * 1000 + H * 100 + L)
    q, k, v, go = (rs.randn(B * L, H * 4).astype(np.float32) for _ in range(4))
    counter, ordinal = COUNTERS[0], ORDINALS[1]
    offset = ops.dropout_step_offset(counter, ordinal)
    got = _attn_run(ops, q, k, v, go, B, H, L, p, ops.StepRng(seed_ctr(counter), ordinal))
    want = _attn_run(ops, q, k, v, go, B, H, L, p, (SEED, offset))
    for name, a, b in zip(("out", "dq", "dk", "dv"), got, want):
        assert torch.equal(a, b), name                                                  # forward and backward: the same bits
    keep = psr.attn_keep_mask(B * H, L, p, SEED, offset)

    def ref(dtype):
        t = [torch.from_numpy(a).to(dtype).requires_grad_(True) for a in (q, k, v)]
        out = psr.causal_attention_rows(*t, B, L, H, keep, p)
        (out * torch.from_numpy(go).to(dtype)).sum().backward()
        return [out.detach().numpy()] + [a.grad.numpy() for a in t]

    r64, r32 = ref(torch.float64), ref(torch.float32)
    assert_all([close("attn dev B%d H%d L%d p=%.1f %s" % (B, H, L, p, n), host(g), a, b)
                for n, g, a, b in zip(("out", "dq", "dk", "dv"), got, r64, r32)])


@pytest.mark.parametrize("B,H,L", ATTN_DEV_SHAPES)
def test_causal_attn_dev_kept_set_element_for_element(ops, B, H, L):
    """The kept set itself, read off the output: with q = 0 every row i spreads 1 / i over its i columns, and with v_j = 2^(j % 16)
    in channel j // 16 the output of row i is (its kept columns as four 16-bit sets) x 2 / i at p = 0.5 (keep scale 2: every sum
    is a sum of small integers, exact in float32).  Column 64 of L = 65 is attended by nobody."""
    p = 0.5
    assert L <= 65
    vj = np.zeros((L, 4), np.float32)
    for j in range(min(L, 64)):
        vj[j, j // 16] = float(1 << (j % 16))
    v = np.tile(vj[None, :, None, :], (B, 1, H, 1)).reshape(B * L, H * 4)
    q = np.zeros_like(v)
    k = np.random.RandomState(2830).randn(B * L, H * 4).astype(np.float32)
    counter, ordinal = COUNTERS[1], ORDINALS[0]
    out = ops.causal_attn(dev(q), dev(k), dev(v), B, L, H, p, rng=ops.StepRng(seed_ctr(counter), ordinal))
    out = host(out).astype(np.float64).reshape(B, L, H, 4)
    keep = psr.attn_keep_mask(B * H, L, p, SEED, ops.dropout_step_offset(counter, ordinal)).reshape(B, H, L, L)
    assert 0 < keep[:, :, np.tril_indices(L, -1)[0], np.tril_indices(L, -1)[1]].mean() < 1 or L == 2
    for b in range(B):
        for h in range(H):
            for i in range(L):
                sets = np.rint(out[b, i, h] * i / 2.0).astype(np.int64)
                want = [sum(1 << (j % 16) for j in range(i) if j // 16 == c and keep[b, h, i, j]) for c in range(4)]
                assert sets.tolist() == want, (b, h, i)
                assert np.abs(out[b, i, h] * i / 2.0 - sets).max() < 0.05                # (an integer up to rounding of 1 / i)


# ---- the model of the step tests -------------------------------------------------------------------------------------------
N_ROWS, B_STEP, C_STEP, Z = 32, 8, 16, 40


def _model(seed=2840, **kw):
    from utils.utils import importing_model
    cfg = dict(model_name="pixelcnn", number_components=C_STEP, training_set_size=N_ROWS, batch_size=B_STEP)
    cfg.update(kw)
    args = smoke_case.vae_args(**cfg)
    torch.manual_seed(seed)
    model = importing_model(args)(args)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    return args, model.cuda().train(), sd


def _dataset(seed, n=N_ROWS):
    x = torch.from_numpy(gi.binary_images(seed, n))
    return torch.utils.data.TensorDataset(x, torch.arange(n).reshape(-1, 1), torch.zeros(n))


class EpsFeed:
    """the model's noise hook over static buffers (a captured launch reads them at every replay): draw k of a step is buffer k"""

    def __init__(self, per_step=2):
        self.bufs = [torch.zeros((B_STEP, Z), device="cuda") for _ in range(per_step)]
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


def _runner(args, model, ds, lr, seed):
    """the model's runner, built under torch.manual_seed(seed): its Philox key is torch's seed at that moment"""
    from utils.optimizer import AdamNormGrad
    from utils.training import _graphed_step
    loader = torch.utils.data.DataLoader(ds, batch_size=B_STEP, shuffle=False)
    torch.manual_seed(seed)
    runner = _graphed_step(args, model, AdamNormGrad(model.parameters(), lr=lr), loader)
    assert runner is not None and runner.seed == seed and runner.dedup is None and not runner.no_exemplars
    return runner


# ---- 2. replay = the same step issued launch by launch ------------------------------------------------------------------------
def test_captured_step_matches_eager():
    """Runner A: three warm-up calls, then four replays.  Runner B, on a twin with the same state dict and built under the same
    seed, issues the same seven steps launch by launch and never captures.  (step_eagerly serves a runner only once its graph
    exists; a runner whose warm-up never ends issues every call in the same form -- the captured launches, the control block, the
    captured optimizer form from call 1 on -- so that is what B is.  An eighth step compares A's step_eagerly with B as well.)
    Same batches, same injected eps, same exemplar draws (the CPU generator is re-seeded before each trajectory): the same bits."""
    ds = _dataset(2841)
    args, model, sd = _model()
    _, twin, _ = _model()
    twin.load_state_dict(copy.deepcopy(sd))
    eps = np.random.RandomState(2842).standard_normal((8, 2, B_STEP, Z)).astype(np.float32)
    betas = [0.25, 0.25, 0.5, 0.5, 0.5, 0.75, 1.0, 1.0]
    x_all, i_all = ds.tensors[0], ds.tensors[1]
    batch = lambda it: (x_all[(it % 4) * B_STEP:(it % 4 + 1) * B_STEP], i_all[(it % 4) * B_STEP:(it % 4 + 1) * B_STEP])

    def trajectory(m, endless_warmup):
        feed = m._draw_eps = EpsFeed()
        runner = _runner(m.args, m, ds, 5e-4, 2843)
        if endless_warmup:
            runner.warmup_steps = 1 << 30
        torch.manual_seed(2844)                                    # the exemplar draws of the seven steps
        outs = []
        for it in range(7):
            feed.load(eps[it])
            outs.append(runner(*batch(it), betas[it]).tolist())
        return runner, feed, outs

    ra, fa, got = trajectory(model, False)
    assert ra.graph is not None and not ra.failed and ra.replays == 4 and ra.by_index
    rb, fb, want = trajectory(twin, True)
    assert rb.graph is None and not rb.failed and rb.replays == 0 and rb._calls == 7
    got, want = np.asarray(got), np.asarray(want)
    print("captured vs eager pixelcnn: (loss, -RE, KL) per step\n", got, "\n", want)
    assert np.isfinite(got).all() and np.array_equal(got, want)
    for (n, p), (_, q) in zip(model.named_parameters(), twin.named_parameters()):
        assert torch.equal(p, q), n
    # step 8: the captured runner's launch-by-launch form against B's
    outs = []
    for runner, feed, step in ((ra, fa, ra.step_eagerly), (rb, fb, rb)):
        torch.manual_seed(2845)
        feed.load(eps[7])
        outs.append(step(*batch(7), betas[7]).tolist())
    assert outs[0] == outs[1] and ra.replays == 4
    for (n, p), (_, q) in zip(model.named_parameters(), twin.named_parameters()):
        assert torch.equal(p, q), n


# ---- 3. the masks move ------------------------------------------------------------------------------------------------------------
def test_masks_move_between_replays():
    """lr = 0, one batch, one injected noise, one exemplar draw: the dropout masks are all that can move the loss between two
    replays (a counter frozen into the graph would repeat it); a runner built under the same seed reproduces the first replay's
    loss at the same call number, bit for bit"""
    ds = _dataset(2851)
    eps = np.random.RandomState(2852).standard_normal((2, B_STEP, Z)).astype(np.float32)
    xb, ib = ds.tensors[0][:B_STEP], ds.tensors[1][:B_STEP]

    def losses(n_calls):
        args, model, _ = _model(seed=2853)
        feed = model._draw_eps = EpsFeed()
        runner = _runner(args, model, ds, 0.0, 2854)
        out = []
        for _ in range(n_calls):
            torch.manual_seed(2855)                                # the same exemplar draw in every call
            feed.load(eps)
            out.append(runner(xb, ib, 0.5).tolist())
        assert runner.graph is not None and not runner.failed and runner.replays == n_calls - runner.warmup_steps
        return out

    first = losses(5)                                              # calls 3 and 4 are replays
    assert first[3][0] != first[4][0] and first[3][1] != first[4][1], first
    assert len({o[0] for o in first}) == 5, first                  # ... and no warm-up call shares a mask with them either
    again = losses(4)
    assert again[3] == first[3] and again[:3] == first[:3], (first, again)


# ---- 4. a replayed step without dropout against the restatement -----------------------------------------------------------------
def test_replayed_step_without_dropout_matches_ref():
    """every nn.Dropout.p = 0, lr = 0 (the weights stay the state dict's), no leave-one-out mask (the restatement has none): the
    (loss, -RE, KL) of one replayed step against tests/pixelsnail_ref.py::pixelcnn_loss in float64 on the batch, the injected eps
    and the exemplar rows the step's control block holds; tolerance of test_model_loss_and_gradients_match_ref"""
    beta = 0.5
    ds = _dataset(2861)
    args, model, sd = _model(seed=2862, no_mask=True)
    n_drop = 0
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p, n_drop = 0.0, n_drop + 1
    assert n_drop == 8
    eps = np.random.RandomState(2863).standard_normal((2, B_STEP, Z)).astype(np.float32)
    feed = model._draw_eps = EpsFeed()
    runner = _runner(args, model, ds, 0.0, 2864)
    xb, ib = ds.tensors[0][B_STEP:2 * B_STEP], ds.tensors[1][B_STEP:2 * B_STEP]
    for _ in range(runner.warmup_steps + 1):
        feed.load(eps)
        out = runner(xb, ib, beta).tolist()
    assert runner.graph is not None and not runner.failed and runner.replays == 1
    rows = runner.rows[:C_STEP].cpu().numpy()
    assert rows.min() >= 0 and rows.max() < N_ROWS and np.array_equal(runner.idx_flat.cpu().numpy(), ib.reshape(-1).numpy())
    assert int(runner.seed_ctr[1]) == runner.warmup_steps
    ex = ds.tensors[0].numpy()[rows]

    def ref(dtype):
        s = {k: v.to(dtype).clone() for k, v in sd.items()}
        with torch.no_grad():
            loss, RE, KL = psr.pixelcnn_loss(s, *(torch.from_numpy(np.ascontiguousarray(a)).to(dtype) for a in (xb.numpy(), eps[0], eps[1], ex)),
                                             beta=beta)
        return [np.array([t.mean().item()], dtype=np.float64 if dtype == torch.float64 else np.float32) for t in (loss, -RE, KL)]

    r64, r32 = ref(torch.float64), ref(torch.float32)
    assert_all([close("replayed step, no dropout: " + n, np.array([g]), a, b) for n, g, a, b in zip(("loss", "-RE", "KL"), out, r64, r32)])


# ---- 5. routing ------------------------------------------------------------------------------------------------------------------
def test_routing_and_the_host_counter():
    from evae import ops
    from evae.graph import GraphedTrainStep
    from utils.optimizer import AdamNormGrad
    from utils.training import _graphed_step, train_one_epoch
    N = 6 * B_STEP
    ds = _dataset(2871, N)
    loader = torch.utils.data.DataLoader(ds, batch_size=B_STEP, shuffle=False)
    args, model, _ = _model(seed=2872, training_set_size=N, warmup=2)
    opt = AdamNormGrad(model.parameters(), lr=5e-4)
    runner = _graphed_step(args, model, opt, loader)
    assert isinstance(runner, GraphedTrainStep) and not runner.no_exemplars and (runner.lo, runner.hi) == (0, C_STEP)
    # every other pixelcnn configuration steps eagerly (the decision is taken on the arguments: a stand-in model carries them)
    for change in (dict(approximate_prior=True), dict(prior="standard"), dict(prior="vampprior"), dict(use_hip_graph=False)):
        other = copy.copy(args)
        vars(other).update(change)
        assert _graphed_step(other, types.SimpleNamespace(args=other), opt, loader) is None, change
    n0 = ops._DROPOUT_CALLS[0]
    res = train_one_epoch(1, args, loader, model, opt)
    assert np.isfinite(res).all()
    assert list(model._graphed_steps.values()) == [runner]
    assert runner.graph is not None and not runner.failed and runner.replays == 6 - runner.warmup_steps
    assert ops._DROPOUT_CALLS[0] == n0                             # the epoch's 48 masks came from the control block
    # outside a runner the host counter serves as before: evaluation draws nothing, training-mode generation one mask per dropout
    # layer and decoder pass
    x = ds.tensors[0][:2].cuda()
    model.eval()
    with torch.no_grad():
        loss, _, _ = model.calculate_loss((x, None), dataset=ds)
    assert bool(torch.isfinite(loss).all()) and ops._DROPOUT_CALLS[0] == n0
    model.train()
    z = torch.randn(1, Z, device="cuda")
    mean = model.pixelcnn_generate(z, z)
    assert mean.shape == (1, 784) and bool(((mean > 0) & (mean < 1)).all())
    assert ops._DROPOUT_CALLS[0] == n0 + 8 * 784
    # ... and an eager training step: eight
    loss, _, _ = model.calculate_loss((x, ds.tensors[1][:2].cuda()), average=True, dataset=ds)
    assert bool(torch.isfinite(loss)) and ops._DROPOUT_CALLS[0] == n0 + 8 * 784 + 8
