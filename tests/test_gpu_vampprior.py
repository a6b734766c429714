"""The VampPrior on the HIP path (csrc/evae_mixture.hip behind evae.ops.mixture_* / pseudo_inputs and models.BaseModel.log_p_z)
against the fp64 restatement tests/vampprior_ref.py and the reference golden G24.

Bars are the exemplar prior's own (tests/test_gpu_kernels.py::test_prior_fwd/bwd_matches_oracle): 1e-5 on logp and the matrix,
1e-4 on the gradients, as rel() = max |a - b| / max |b|."""
import math

import numpy as np
import pytest
import torch

import golden_inputs as gi
import smoke_case
import vampprior_ref as vr

pytestmark = pytest.mark.gpu

FWD_BAR, BWD_BAR = 1e-5, 1e-4
SHAPES = [(1, 1, 40), (5, 7, 3), (37, 301, 40), (100, 500, 40), (257, 1000, 40), (3, 1500, 33), (64, 1000, 8), (130, 70, 256),
          (20, 150, 294), (9, 70, 512)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def ops():
    from evae import ops as o
    return o


def check_against_ref(ops, z, mu, lv, n_components, gout, tag=""):
    """forward (logp, matrix) and the three gradients of one input set against fp64; prints each figure before it asserts"""
    zt, mt, lt, gt = dev(z), dev(mu), dev(lv), dev(gout)
    logp, token, prob = ops.mixture_lse_fwd(zt, mt, lt, n_components, want_prob=True)
    dz, dmu, dlv = ops.mixture_lse_bwd(zt, mt, lt, n_components, token, gt)
    ref_p = vr.matrix(z, mu, lv, n_components)
    ref_lp = vr.logp_of(ref_p)
    rdz, rdmu, rdlv = vr.grads(z, mu, lv, n_components, gout)
    got = [host(t) for t in (logp, prob, dz, dmu, dlv)]
    assert all(np.isfinite(a).all() for a in got), tag
    fin = np.isfinite(ref_p)
    figs = dict(logp=rel(got[0], ref_lp), prob=rel(got[1][fin], ref_p[fin]), dz=rel(got[2], rdz), dmu=rel(got[3], rdmu),
                dlv=rel(got[4], rdlv))
    print("vampprior %s %s: %s" % (tag, (z.shape[0], mu.shape[0], z.shape[1]), {k: "%.2e" % v for k, v in figs.items()}))
    assert figs["logp"] < FWD_BAR and figs["prob"] < FWD_BAR, (tag, figs)
    assert figs["dz"] < BWD_BAR and figs["dmu"] < BWD_BAR and figs["dlv"] < BWD_BAR, (tag, figs)
    return logp, ref_lp


@pytest.mark.parametrize("B,C,zd", SHAPES)
def test_mixture_fwd_bwd_matches_ref(ops, B, C, zd):
    z, mu, lv, gout = vr.inputs(2400 + B + C + zd, B, C, zd)
    assert lv.min() == -6.0 and lv.max() == 2.0
    check_against_ref(ops, z, mu, lv, C, gout)


def test_mixture_matches_reference_golden(ops, golden):
    """G24(a) straight from the file, through the autograd Function"""
    g = golden("g24_vampprior")
    z, mu, lv = (dev(g[k]).requires_grad_(True) for k in ("a_z", "a_mu", "a_lv"))
    C = mu.shape[0]
    logp = ops.mixture_logp(z, mu, lv, C)
    (logp * dev(g["a_gout"])).sum().backward()
    with torch.no_grad():
        prob = ops.mixture_lse_fwd(z, mu, lv, C, want_prob=True)[2]
    assert rel(host(logp), g["a_logp"]) < FWD_BAR
    assert rel(host(prob), g["a_prob"]) < FWD_BAR
    assert rel(host(z.grad), g["a_dz"]) < BWD_BAR
    assert rel(host(mu.grad), g["a_dmu"]) < BWD_BAR
    assert rel(host(lv.grad), g["a_dlv"]) < BWD_BAR


def test_autograd_skips_unwanted_gradients(ops):
    z, mu, lv, gout = vr.inputs(7, 37, 301, 40)
    zt, mt, lt = dev(z).requires_grad_(True), dev(mu), dev(lv)
    (ops.mixture_logp(zt, mt, lt, 301) * dev(gout)).sum().backward()
    assert mt.grad is None and lt.grad is None
    assert rel(host(zt.grad), vr.grads(z, mu, lv, 301, gout)[0]) < BWD_BAR
    zt, mt, lt = dev(z), dev(mu).requires_grad_(True), dev(lv).requires_grad_(True)
    (ops.mixture_logp(zt, mt, lt, 301) * dev(gout)).sum().backward()
    _, rdmu, rdlv = vr.grads(z, mu, lv, 301, gout)
    assert rel(host(mt.grad), rdmu) < BWD_BAR and rel(host(lt.grad), rdlv) < BWD_BAR


def test_n_components_is_an_argument(ops):
    """number_components = 500 with an embedding of 301 components: logp shifts by exactly log(301 / 500)"""
    z, mu, lv, gout = vr.inputs(11, 37, 301, 40)
    lp500, ref500 = check_against_ref(ops, z, mu, lv, 500, gout, tag="n=500")
    ref301 = vr.forward(z, mu, lv, 301)
    assert np.allclose(ref500 - ref301, math.log(301.0 / 500.0), rtol=0, atol=1e-9)
    lp301 = ops.mixture_lse_fwd(dev(z), dev(mu), dev(lv), 301)[0]
    assert rel(host(lp301), ref301) < FWD_BAR


def test_far_queries(ops):
    """every p_ij below -1e5: the maximum is subtracted before anything is exponentiated"""
    z, mu, lv, gout = vr.inputs(13, 37, 301, 40)
    z = (z + 50.0).astype(np.float32)
    assert vr.matrix(z, mu, lv, 301).max() < -1e5
    check_against_ref(ops, z, mu, lv, 301, gout, tag="far")


def test_zero_upstream_rows(ops):
    z, mu, lv, gout = vr.inputs(17, 100, 500, 40)
    gout[20:61] = 0.0
    zt, mt, lt = dev(z), dev(mu), dev(lv)
    _, token, _ = ops.mixture_lse_fwd(zt, mt, lt, 500)
    dz, dmu, dlv = ops.mixture_lse_bwd(zt, mt, lt, 500, token, dev(gout))
    assert (host(dz)[20:61] == 0.0).all()
    rdz, rdmu, rdlv = vr.grads(z, mu, lv, 500, gout)
    assert rel(host(dz), rdz) < BWD_BAR and rel(host(dmu), rdmu) < BWD_BAR and rel(host(dlv), rdlv) < BWD_BAR
    # ... and those rows contribute nothing: the component gradients are those of the other rows alone, bit for bit
    keep = np.r_[0:20, 61:100]
    zk = dev(z[keep])
    _, tk, _ = ops.mixture_lse_fwd(zk, mt, lt, 500)
    _, dmu_k, dlv_k = ops.mixture_lse_bwd(zk, mt, lt, 500, tk, dev(gout[keep]), need=(False, True, True))
    assert torch.equal(dmu, dmu_k) and torch.equal(dlv, dlv_k)


def test_evaluator_shape_sampled(ops):
    B, C, zd = 4096, 500, 40
    z, mu, lv, _ = vr.inputs(19, B, C, zd)
    logp = host(ops.mixture_lse_fwd(dev(z), dev(mu), dev(lv), C)[0])
    pick = np.random.RandomState(B).choice(B, size=96, replace=False)
    assert np.isfinite(logp).all()
    assert rel(logp[pick], vr.forward(z[pick], mu, lv, C)) < FWD_BAR


def test_backward_is_deterministic(ops):
    z, mu, lv, gout = vr.inputs(23, 257, 1000, 40)
    zt, mt, lt, gt = dev(z), dev(mu), dev(lv), dev(gout)
    runs = []
    for _ in range(2):
        lp, token, _ = ops.mixture_lse_fwd(zt, mt, lt, 1000)
        runs.append((lp,) + ops.mixture_lse_bwd(zt, mt, lt, 1000, token, gt))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_single_stream_graph_capture(ops):
    """mixture_logp forward + backward captured on ONE stream (no parallel branches); the replay on refilled static inputs is
    bit-equal to the eager result on the same inputs"""
    B, C, zd = 100, 500, 40
    za, mua, lva, ga = vr.inputs(29, B, C, zd)
    zb, mub, lvb, gb = vr.inputs(31, B, C, zd)
    sz, sm, sl, sg = dev(za).requires_grad_(True), dev(mua).requires_grad_(True), dev(lva).requires_grad_(True), dev(ga)

    def step():
        lp = ops.mixture_logp(sz, sm, sl, C)
        grads = torch.autograd.grad((lp * sg).sum(), (sz, sm, sl))
        return (lp,) + tuple(grads)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                    # warm-up: workspaces are allocated before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = step()
    with torch.no_grad():
        for dst, src in ((sz, zb), (sm, mub), (sl, lvb), (sg, gb)):
            dst.copy_(dev(src))
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in static_out]
    eager = step()
    for a, b in zip(replayed, eager):
        assert torch.equal(a, b)
    assert rel(host(replayed[0]), vr.forward(zb, mub, lvb, C)) < FWD_BAR


@pytest.mark.parametrize("D,C", [(64, 77), (784, 500), (48, 5)])
def test_pseudo_inputs(ops, D, C):
    rs = np.random.RandomState(D + C)
    w = rs.uniform(-0.6, 1.6, size=(D, C)).astype(np.float32)
    flat = w.reshape(-1)
    flat[rs.choice(flat.size, size=max(4, flat.size // 10), replace=False)] = 0.0
    flat[rs.choice(flat.size, size=max(4, flat.size // 10), replace=False)] = 1.0
    assert (w < 0).any() and (w > 1).any() and ((w > 0) & (w < 1)).any() and (w == 0).any() and (w == 1).any()
    g = rs.standard_normal((C, D)).astype(np.float32)
    wt = dev(w).requires_grad_(True)
    x = ops.pseudo_inputs(wt)
    x.backward(dev(g))
    wr = dev(w).requires_grad_(True)
    xr = torch.nn.functional.hardtanh(wr.t(), 0.0, 1.0)
    xr.backward(dev(g))
    assert x.shape == (C, D) and torch.equal(x, torch.clamp(wr.detach().t(), 0.0, 1.0)) and torch.equal(x, xr)
    assert torch.equal(wt.grad, wr.grad)
    # ... and to what the model computed before: the identity pushed through the bias-free hardtanh layer
    lin = torch.nn.functional.linear(torch.eye(C, device="cuda"), wr.detach())
    assert torch.equal(x, torch.nn.functional.hardtanh(lin, 0.0, 1.0))


def _vamp_model(cls, model_name, C, z, hidden=32, input_size=(1, 8, 8)):
    args = smoke_case.vae_args(prior="vampprior", model_name=model_name, input_size=list(input_size), hidden_size=hidden, z1_size=z,
                               z2_size=z, number_components=C, training_set_size=100, batch_size=16, pseudoinputs_mean=0.05,
                               pseudoinputs_std=0.01, use_training_data_init=False)
    return args, cls(args).cuda()


MEM_BOUND = 16 << 20


@pytest.mark.parametrize("with_grad", [False, True])
def test_log_p_z_memory(ops, with_grad):
    """model.log_p_z at B = 4096 against an embedding of 500 components, z = 40: the peak allocation above the starting level
    stays under 16 MiB (the [B x C x z] fp32 tensor of the torch composition alone is 328 MB).  The workspaces are cached by
    evae.ops._workspace and grow geometrically: one small call warms them, the growth to this size is inside the bound."""
    from models.VAE import VAE
    B, C, zd = 4096, 500, 40
    args, model = _vamp_model(VAE, "vae", C, zd)
    z, mu, lv, _ = vr.inputs(37, B, C, zd)
    zt, mt, lt = dev(z), dev(mu), dev(lv)
    small = dev(z[:8]).requires_grad_(with_grad)
    with torch.set_grad_enabled(with_grad):
        warm = model.log_p_z((small, None), (mt, lt))
        if with_grad:
            warm.sum().backward()
    zt.requires_grad_(with_grad)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    start = torch.cuda.memory_allocated()
    with torch.set_grad_enabled(with_grad):
        lp = model.log_p_z((zt, None), (mt, lt))
        if with_grad:
            lp.sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - start
    print("log_p_z peak above start (grad=%s): %.2f MiB" % (with_grad, peak / 2.0 ** 20))
    assert peak < MEM_BOUND
    assert rel(host(lp)[:64], vr.forward(z[:64], mu, lv, C)) < FWD_BAR
    if with_grad:
        assert zt.grad is not None and torch.isfinite(zt.grad).all()


def test_log_p_z_matrix_and_sum(ops):
    """log_p_z(sum=False): the kernel's matrix without a gradient, the torch composition with one -- the same values"""
    from models.VAE import VAE
    args, model = _vamp_model(VAE, "vae", 77, 8)
    z, mu, lv, _ = vr.inputs(41, 16, 77, 8)
    ref = vr.matrix(z, mu, lv, 77)
    with torch.no_grad():
        prob = model.log_p_z((dev(z), None), (dev(mu), dev(lv)), sum=False)
    assert prob.shape == (16, 77) and rel(host(prob), ref) < FWD_BAR
    zt = dev(z).requires_grad_(True)
    prob_g = model.log_p_z((zt, None), (dev(mu), dev(lv)), sum=False)
    assert prob_g.requires_grad and rel(host(prob_g), ref) < FWD_BAR
    with torch.no_grad():                          # no embedding: the components come from the model's own pseudo-inputs
        own = model.log_p_z((dev(z), None), None)
        pmu, plv = model.q_z(model.pseudo_inputs(), prior=True)
    assert rel(host(own), vr.forward(z, host(pmu), host(plv), 77)) < FWD_BAR


@pytest.mark.parametrize("model_name", ["vae", "hvae_2level"])
def test_models_match_reference_golden(golden, model_name):
    """G24(b): calculate_loss, every gradient norm, the full pseudo-input gradient and evaluate_loss of a VampPrior model with 77
    components against the reference on identical weights, batch and eps"""
    from models.VAE import VAE
    from models.HVAE_2level import VAE as HVAE
    from utils.evaluation import evaluate_loss
    g = golden("g24_vampprior")
    B, D = 16, 64
    args, model = _vamp_model(VAE if model_name == "vae" else HVAE, model_name, 77, 8)
    sd = {k[len(model_name) + 4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(model_name + "_sd_")}
    assert set(sd) == set(model.state_dict().keys())
    model.load_state_dict(sd)
    model.train()
    eps = torch.from_numpy(g["eps"]).cuda()
    model._draw_eps = lambda like: eps[:like.shape[0]]
    x = torch.from_numpy(gi.binary_images(242, B, D)).cuda()
    loss, RE, KL = model.calculate_loss((x, torch.arange(B).reshape(-1, 1).cuda()), 0.7, average=False)
    loss.mean().backward()
    for name, t in (("loss", loss), ("RE", RE), ("KL", KL)):
        assert rel(host(t), g[model_name + "_" + name]) < 1e-4, name
    for n, p in model.named_parameters():
        ref = float(g[model_name + "_gnorm_" + n])
        got = 0.0 if p.grad is None else p.grad.double().norm().item()
        assert abs(got - ref) <= 1e-3 * max(ref, 1e-6), n
    assert rel(host(model.means.linear.weight.grad), g[model_name + "_grad_means.linear.weight"]) < 1e-4
    model.eval()
    model._draw_eps = lambda like: torch.zeros_like(like)
    test = torch.from_numpy(gi.binary_images(243, 24, D))
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(test, torch.zeros(24)), batch_size=8)
    with torch.no_grad():
        ev = evaluate_loss(args, model, loader, dataset=None)
    assert rel(np.asarray(ev), g[model_name + "_eval"]) < 1e-4


def test_calculate_likelihood(golden):
    """The IWAE estimate of the G24 vae (S = 64, 6 test rows, a fixed eps stream) against the same computation with log_p_z
    replaced by the fp64 restatement over the model's own embedding"""
    from models.VAE import VAE
    from utils.evaluation import calculate_likelihood, load_all_pseudo_input
    g = golden("g24_vampprior")
    args, model = _vamp_model(VAE, "vae", 77, 8)
    model.load_state_dict({k[len("vae") + 4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("vae_sd_")})
    model.eval()
    test = torch.from_numpy(gi.binary_images(243, 6, 64))
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(test, torch.zeros(6)), batch_size=6)

    def fixed_eps():
        gen = torch.Generator(device="cuda")
        gen.manual_seed(7)
        return lambda like: torch.randn(like.shape, generator=gen, device=like.device, dtype=like.dtype)

    with torch.no_grad():
        emb = load_all_pseudo_input(args, model, None)
        mu, lv = host(emb[0]), host(emb[1])
        assert mu.shape == (77, 8)
        model._draw_eps = fixed_eps()
        got = calculate_likelihood(args, model, loader, S=64, exemplars_embedding=emb)
        model._draw_eps = fixed_eps()
        model.log_p_z = lambda z, exemplars_embedding, sum=True, test=None: dev(vr.forward(host(z[0]), mu, lv, 77).astype(np.float32))
        want = calculate_likelihood(args, model, loader, S=64, exemplars_embedding=emb)
    print("calculate_likelihood: %.6f vs %.6f" % (got, want))
    assert np.isfinite(got) and abs(got - want) <= 1e-4 * abs(want)
