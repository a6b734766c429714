"""BaseModel with the reference's API (reference models/BaseModel.py:16-271): loss assembly, the
exemplar prior, exemplar-set sampling, the latent cache and the kNN-approximate prior -- computed by the
MI355X kernels of libevae_hip.so (evae.ops).  What changed underneath, not in behaviour:

* log_p_z never materialises the [B x C] matrix: distance + leave-one-out mask + log-sum-exp are one
  fused kernel (evae.ops.PriorLogP), differentiated by recomputation from the saved row LSE.
* the training images stay resident in HBM (one upload per dataset); the exemplar gather of
  reference :247 is folded into the A-tile load of the first encoder GEMM (`rows=`), so no [C x D]
  copy is made and nothing crosses PCIe per step.
* the approximate prior's distance + top-K (:263-264) is the fused fp64-accumulated top-K kernel.
* with torch.distributed initialised and args.shard_exemplars=True, the exemplar set is sharded across
  ranks and the per-shard partial log-sum-exps are merged after one RCCL all-gather (evae.shard).

* the VampPrior (--prior vampprior) scores z against its per-component-variance mixture in one fused kernel
  (evae.ops.MixtureLogP, csrc/evae_mixture.hip) and reads its pseudo-inputs as a transposing clamp of the `means` weight
  (pseudo_inputs()) in place of the identity GEMM; the training step of `vae` / `hvae_2level` replays from one hipGraph
  (utils/training.py::vampprior_step_eligible), the same launches as the eager step;
  the convolutional models' step stays eager, and nothing of it is sharded.
* the standard-normal prior (--prior standard) trains `vae` through one autograd node on one stream (evae/fused_std.py: the batch
  rows' chain with the latent block as one launch each way, csrc/evae_latent_std.hip) and `hvae_2level` through its modular path,
  both replayed from one hipGraph (utils/training.py::standard_step_eligible); the convolutional models' step stays eager.

Out of scope: the image-generation helpers keep their names and run on plain torch ops."""
import math
import os
from abc import ABC, abstractmethod

import numpy as np
import torch
import torch.nn as nn

from evae import fused_std, fused_vae, handoff, ops, shard
from utils.distributions import (log_bernoulli, log_normal_diag, log_normal_standard, log_logistic_256,
                                 log_normal_diag_vectorized)
from utils.nn import NonLinear, he_init, normal_init


class BaseModel(nn.Module, ABC):
    def __init__(self, args):
        super().__init__()
        print("constructor")
        self.args = args
        if self.args.prior == 'vampprior':
            self.add_pseudoinputs()
        if self.args.prior == 'exemplar_prior':
            self.prior_log_variance = torch.nn.Parameter(torch.randn((1)))
        d_in = int(np.prod(self.args.input_size))
        if self.args.input_type == 'binary':
            self.p_x_mean = NonLinear(self.args.hidden_size, d_in, activation=nn.Sigmoid())
        elif self.args.input_type in ('gray', 'continuous'):
            self.p_x_mean = NonLinear(self.args.hidden_size, d_in)
            self.p_x_logvar = NonLinear(self.args.hidden_size, d_in,
                                        activation=nn.Hardtanh(min_val=-4.5, max_val=0))
            self.decoder_logstd = torch.nn.Parameter(torch.tensor([0.], requires_grad=True))
        self._resident = {}          # id(dataset) -> device copy of dataset.tensors[0]
        self._resident_u8 = {}       # id(dataset) -> uint8 device store (or None when the data are not k/255)
        self.create_model(args)
        self.he_initializer()

    # ------------------------------------------------------------------ construction
    def he_initializer(self):
        print("he initializer")
        for m in self.modules():
            if isinstance(m, nn.Linear):
                he_init(m)

    @abstractmethod
    def create_model(self, args):
        pass

    @abstractmethod
    def kl_loss(self, latent_stats, exemplars_embedding, dataset, cache, x_indices):
        pass

    # ------------------------------------------------------------------ loss
    def reconstruction_loss(self, x, x_mean, x_logvar):
        if self.args.input_type == 'binary':
            return log_bernoulli(x, x_mean, dim=1)
        if self.args.input_type in ('gray', 'continuous'):
            if self.args.use_logit is True:
                return log_normal_diag(x, x_mean, x_logvar, dim=1)
            return log_logistic_256(x, x_mean, x_logvar, dim=1)
        raise Exception('Wrong input type!')

    def _fused_config(self):
        """the part of _fused_path that only depends on the configuration"""
        a = self.args
        # the approximate prior rides the same node with its B * k static exemplar slots (leave-one-out mask on, one device)
        approx_ok = a.approximate_prior is False or (a.no_mask is False and not self._sharded())
        return (getattr(self, '_use_fused', True) and a.model_name == 'vae' and a.prior == 'exemplar_prior'
                and a.input_type == 'binary' and approx_ok and a.no_attention is False
                and not getattr(a, 'same_variational_var', False))

    def _fused_path(self, x, x_indices, exemplars_embedding, dataset, cache=None):
        """The one-node implementation (evae/fused_vae.py) covers the headline configuration: MLP `vae`,
        exemplar prior, exact or kNN-approximate exemplar sets, binary inputs, training mode."""
        if self.args.approximate_prior and (cache is None or cache[0].requires_grad):
            return False
        return (self._fused_config() and self.training and exemplars_embedding is None and dataset is not None
                and x_indices is not None and x.is_cuda and torch.is_grad_enabled())

    def _calculate_loss_fused(self, x, x_indices, beta, dataset, average, cache=None):
        a = self.args
        C = a.number_components
        sharded = self._sharded()
        lo, hi = shard.bounds(C) if sharded else (0, C)
        # the step runner's word about this step (evae/graph.py), looked up once; an eager step carries a hand-off of its own
        # (bench.py still clears a `_exemplar_indices_override` on the model: that attribute is no longer read)
        h = handoff.current() or handoff.StepHandoff()
        if h.rows is not None:            # graph-captured step: gather list [local exemplars | staging rows], #local
            ex_local = h.rows[:h.n_rows]
        else:
            exemplars_indices = torch.randint(low=0, high=a.training_set_size, size=(C,))   # reference :245
            eager_dd = self._dedup_draws(exemplars_indices[lo:hi]) if not exemplars_indices.is_cuda else None
            if eager_dd is not None:
                ex_local, h.dedup = eager_dd       # (the distinct rows; their tables reach the node's forward on the hand-off)
            else:
                ex_local = self._indices_to_device(exemplars_indices[lo:hi])
        # the image store the exemplar rows are gathered from: bytes when the data are k/255 (4x less HBM, and the first
        # layer then runs on the bf16 matrix pipe, csrc/evae_dense_u8.hip), fp32 rows otherwise
        u8 = self.resident_u8(dataset, x.shape[0])
        x2 = x.reshape(x.shape[0], -1).float()
        if u8 is not None and not h.batch_staged and not torch.cuda.is_current_stream_capturing():
            # eager call: the batch goes into the byte store's staging rows as round(255 x), so x itself has to be k/255 (what
            # the loaders and dynamic binarisation hand out); a batch that is not -- augmented, noisy -- takes the fp32 store
            # for this call instead of being quantised silently (a capture cannot read a flag back: the captured step checks its
            # loader's first batch instead, evae/graph.py::_refresh, and steps eagerly when that is not k/255)
            # The verdict costs a device-to-host read: it is taken for the first batches of a dataset and every 32nd after that
            # (EVAE_CHECK_BATCH=1: every batch) -- a loader hands out one kind of image
            cnt = self._u8_checks = getattr(self, '_u8_checks', {})
            kq = id(dataset)
            nq = cnt.get(kq, 0)
            cnt[kq] = nq + 1
            if nq < 4 or nq % 32 == 0 or os.environ.get("EVAE_CHECK_BATCH", "0") == "1" or cnt.get((kq, "bad"), False):
                q = torch.round(x2 * self.U8_DIV)
                bad = not bool(((q >= 0) & (q <= 255) & (q / self.U8_DIV == x2)).all())
                cnt[(kq, "bad")] = bad or cnt.get((kq, "bad"), False)      # sticky: a loader that once handed out other images is
                                                                            # checked on every batch from then on
                if bad:
                    u8 = None
        if u8 is not None:
            data_ext, n_data = u8[0], u8[1]
        else:
            data_ext, n_data = self.resident_data_ext(dataset, x.shape[0])
        if a.training_set_size > n_data:
            # the reference's dataset.tensors[0][exemplars_indices] raises here; the row-gather GEMM would read staging rows
            raise IndexError("training_set_size %d exceeds the %d rows of the dataset" % (a.training_set_size, n_data))
        # the captured step draws eps in its prologue launch; `_eps_override` is the noise hook of a model without a runner (tests)
        eps = h.eps if h.eps is not None else getattr(self, '_eps_override', None)
        if eps is None or tuple(eps.shape) != (x2.shape[0], a.z1_size):
            eps = self._draw_eps(torch.empty((x2.shape[0], a.z1_size), device=x.device))
        named = dict(self.named_parameters())
        params = [named[n] for n in fused_vae.PARAM_ORDER]
        beta = beta if torch.is_tensor(beta) else float(beta)
        approx_cache = cache[0] if a.approximate_prior else None  # ex_local is then the candidate draw (reference :258)
        with handoff.active(h):           # (the runner's, which is active already, or this eager step's own)
            return fused_vae.VaeExactLoss.apply(x2, x_indices.reshape(-1), data_ext, n_data, ex_local, C, eps,
                                                beta, (2 if getattr(a, 'shard_batch', False) else 1) if sharded else 0,
                                                bool(a.no_mask), bool(average), None if a.approximate_prior else h.rows, h.batch_staged,
                                                approx_cache, int(a.approximate_k), *params)

    def _fused_std_config(self):
        """whether the configuration is the one evae/fused_std.py covers: MLP `vae`, standard-normal prior, binary inputs, gated
        layers, a log-variance head (the exclusions of _fused_config)"""
        a = self.args
        return (getattr(self, '_use_fused', True) and a.model_name == 'vae' and a.prior == 'standard'
                and a.input_type == 'binary' and a.no_attention is False
                and not getattr(a, 'same_variational_var', False))

    def _calculate_loss_fused_std(self, x, beta, average):
        """The one-node, one-stream step of the standard-normal prior (evae/fused_std.py); beta and the noise come from the step's
        hand-off when a runner installed one, as on the exemplar prior's node."""
        h = handoff.current() or handoff.StepHandoff()
        x2 = x.reshape(x.shape[0], -1).float()
        eps = h.eps if h.eps is not None else getattr(self, '_eps_override', None)
        if eps is None or tuple(eps.shape) != (x2.shape[0], self.args.z1_size):
            eps = self._draw_eps(torch.empty((x2.shape[0], self.args.z1_size), device=x.device))
        named = dict(self.named_parameters())
        params = [named[n] for n in fused_std.PARAM_ORDER]
        beta = beta if torch.is_tensor(beta) else float(beta)
        with handoff.active(h):           # (the runner's, which is active already, or this eager step's own)
            return fused_std.VaeStandardLoss.apply(x2, eps, beta, bool(average), *params)

    def calculate_loss(self, x, beta=1., average=False, exemplars_embedding=None, cache=None, dataset=None):
        x, x_indices = x
        if self._fused_path(x, x_indices, exemplars_embedding, dataset, cache):
            return self._calculate_loss_fused(x, x_indices, beta, dataset, average, cache)
        if self._fused_std_config() and self.training and x.is_cuda and torch.is_grad_enabled():
            return self._calculate_loss_fused_std(x, beta, average)
        if self.training and self.args.prior == 'exemplar_prior' and self._data_parallel():
            self._data_parallel_step()
        x_flat = x.reshape(x.shape[0], -1) if x.dim() != 2 else x
        if self._decoder_beside_prior(x, exemplars_embedding, dataset):
            # The decoder p(x | z) and the reconstruction term need z and nothing of the prior; the prior's exemplar set (top-k over the
            # cache, a device-to-host read of the neighbour list, ~100 images re-encoded -- small launches that fill no machine) needs
            # mu and nothing of the decoder: the decoder goes to a side stream.  Autograd runs every node's backward on the stream of
            # its forward, so the two backward halves overlap the same way, and the host's wait for the neighbour list no longer
            # idles the GPU (reference models/BaseModel.py:54-77, same modules, same arithmetic).  EVAE_DECODER_STREAM=0: one stream.
            main = torch.cuda.current_stream()
            side = ops.model_side_stream(x.device)
            mu, logvar = self.q_z(x)
            z = self.reparameterize(mu, logvar)
            side.wait_stream(main)
            z.record_stream(side)
            with torch.cuda.stream(side):
                x_mean, x_logvar = self.p_x(z)
                RE = self.reconstruction_loss(x_flat, x_mean, x_logvar)
            KL = self.kl_loss((z, mu, logvar), exemplars_embedding, dataset, cache, x_indices)
            main.wait_stream(side)
            RE.record_stream(main)
        else:
            x_mean, x_logvar, latent_stats = self.forward(x)
            RE = self.reconstruction_loss(x_flat, x_mean, x_logvar)
            KL = self.kl_loss(latent_stats, exemplars_embedding, dataset, cache, x_indices)
        loss = -RE + beta * KL
        if average:
            loss, RE, KL = torch.mean(loss), torch.mean(RE), torch.mean(KL)
        return loss, RE, KL

    def _decoder_beside_prior(self, x, exemplars_embedding, dataset):
        a = self.args
        return (os.environ.get("EVAE_DECODER_STREAM", "1") != "0" and self.training and x.is_cuda and torch.is_grad_enabled()
                and a.model_name == 'single_conv' and a.prior == 'exemplar_prior' and exemplars_embedding is None and dataset is not None
                and not self._sharded() and not torch.cuda.is_current_stream_capturing())

    def importance_sample_losses(self, data, S, exemplars_embedding):
        """-ELBO of S importance samples for each row of `data` [g x D] -> [g * S], sample s of image i at row i * S + s
        (what utils.evaluation.calculate_likelihood needs; the reference builds it by expanding the image S times and
        calling calculate_loss, utils/evaluation.py:88-90).  Subclasses whose encoder only sees x encode each image
        once instead of S times."""
        x = data.reshape(data.size(0), -1).repeat_interleave(S, dim=0)
        return self.calculate_loss((x, None), exemplars_embedding=exemplars_embedding)[0]

    def _draw_eps(self, like):
        """Standard-normal noise from the device generator (reference :81); tests override this to inject
        identical eps into the reference, the oracle and this model."""
        h = handoff.current()
        if (h is not None and h.eps is not None and self.args.prior in ('vampprior', 'standard') and self.args.model_name == 'vae'
                and self.training and tuple(h.eps.shape) == tuple(like.shape)):
            # a captured VampPrior or standard-prior step of `vae`, the one model with ONE draw per step: the noise its prologue
            # launch drew (evae/graph.py).  hvae_2level draws z2 and z1 with the same shape and must not get one buffer twice
            return h.eps
        g = getattr(self, '_eps_generator', None)      # evaluation over a sharded cache: the same stream on every rank (evae/shard.py)
        if g is not None:
            return torch.randn(like.shape, generator=g, device=like.device, dtype=like.dtype)
        return torch.randn_like(like)

    def reparameterize(self, mu, logvar):
        z, _ = ops.ReparamLogQ.apply(mu, logvar, self._draw_eps(mu))
        return z

    # ------------------------------------------------------------------ priors
    def pseudo_inputs(self):
        """The VampPrior's pseudo-inputs [C x D] (reference :130-140: self.means(self.idle_input), the identity pushed through a
        bias-free hardtanh layer).  On the GPU: clamp(W^T, 0, 1) by one transposing kernel, the same bits without the GEMMs."""
        w = self.means.linear.weight
        if w.is_cuda:
            return ops.pseudo_inputs(w)
        return self.means(self.idle_input)

    def _vampprior_components(self, exemplars_embedding):
        if exemplars_embedding is None:
            return self.q_z(self.pseudo_inputs(), prior=True)
        return exemplars_embedding

    def log_p_z_vampprior(self, z, exemplars_embedding):
        """[B x C] matrix log N(z_i | mu_j, exp(lv_j)) - log(number_components) (reference :84-96).  Differentiable like the
        reference's: with a gradient requested it is the torch composition, otherwise one pass of the fused kernel."""
        C = self.args.number_components
        z_p_mean, z_p_logvar = self._vampprior_components(exemplars_embedding)
        if z.is_cuda and not (torch.is_grad_enabled() and (z.requires_grad or z_p_mean.requires_grad or z_p_logvar.requires_grad)):
            return ops.mixture_lse_fwd(z, z_p_mean, z_p_logvar, C, want_prob=True)[2]
        return log_normal_diag(z.unsqueeze(1), z_p_mean.unsqueeze(0), z_p_logvar.unsqueeze(0), dim=2) - math.log(C)

    def _sharded(self):
        return bool(getattr(self.args, 'shard_exemplars', False)) and shard.is_active()

    def _data_parallel(self):
        """args.shard_batch in an active group: every rank trains on its own batch, the exemplars stay sharded"""
        return bool(getattr(self.args, 'shard_batch', False)) and self._sharded()

    def _data_parallel_step(self):
        """What a training step on the modular path settles before its first launch when the ranks hold different batches: the
        approximate prior is refused (shard.sharded_topk merges candidate lists as if every rank held the same query rows) --
        before any collective, so no rank is left waiting for another --, and the eager dropout masks get the rank in their seed."""
        if self.args.approximate_prior:
            raise ValueError("approximate_prior=True cannot be combined with shard_batch=True: the sharded top-k merges the ranks' "
                             "candidate lists for one common set of query rows; use the exact exemplar prior, or shard_exemplars alone")
        shard.fold_rank_into_noise()

    def log_p_z_exemplar(self, z, z_indices, exemplars_embedding, test):
        """[B x C] matrix of log N(z_i | c_j, exp(logvar)) - log(C - #masked_i), -inf on leave-one-out hits
        (reference :98-109).  Kept for API parity (log_p_z(sum=False)) -- the loss path uses the fused kernel in log_p_z.
        Differentiable like the reference's: with a gradient requested the matrix is composed from the differentiable
        distance (utils.distributions.log_normal_diag_vectorized), otherwise it is one pass of the fused kernel."""
        centers, center_log_variance, center_indices = exemplars_embedding
        masked = (test is False) and (self.args.no_mask is False) and z_indices is not None
        lv_row = center_log_variance[0, :]
        if torch.is_grad_enabled() and (z.requires_grad or centers.requires_grad or lv_row.requires_grad):
            prob, _ = log_normal_diag_vectorized(z, centers, lv_row.unsqueeze(0))
            denominator = torch.full((len(z),), float(len(centers)), device=z.device)
            if masked:
                ci = center_indices.to(z.device).reshape(1, -1)
                mask = (z_indices.reshape(-1, 1) == ci) | (ci == ops.PRIOR_MASK_ALL)
                prob = prob.masked_fill(mask, float('-inf'))
                denominator = denominator - mask.sum(dim=1)
            return prob - torch.log(denominator).unsqueeze(1)
        _, _, nmask, prob = ops.prior_lse_fwd(z.detach(), centers.detach(), lv_row.detach(),
                                              z_indices if masked else None,
                                              center_indices.to(z.device) if masked else None, want_prob=True)
        denominator = float(len(centers)) - nmask
        return prob - torch.log(denominator).unsqueeze(1)

    def log_p_z(self, z, exemplars_embedding, sum=True, test=None):
        z, z_indices = z
        if test is None:
            test = not self.training
        if self.args.prior == 'standard':
            return log_normal_standard(z, dim=1)
        if self.args.prior == 'vampprior':
            if sum and z.is_cuda:
                z_p_mean, z_p_logvar = self._vampprior_components(exemplars_embedding)
                return ops.mixture_logp(z, z_p_mean, z_p_logvar, self.args.number_components)
            prob = self.log_p_z_vampprior(z, exemplars_embedding)
            if not sum:
                return prob
            prob_max, _ = torch.max(prob, 1)
            return prob_max + torch.log(torch.sum(torch.exp(prob - prob_max.unsqueeze(1)), 1))
        if self.args.prior != 'exemplar_prior':
            raise Exception('Wrong name of the prior!')
        if not sum:
            return self.log_p_z_exemplar(z, z_indices, exemplars_embedding, test)
        centers, center_log_variance, center_indices = exemplars_embedding
        masked = (test is False) and (self.args.no_mask is False) and z_indices is not None
        # only row 0 is used (reference :101).  When the log-variance is the model's ONE prior value expanded over the exemplars
        # (q_z(prior=True) tags it), the row is taken from the value itself: its gradient then comes back through a 40-element
        # sum instead of a zero-filled [C x z] buffer, a row copy and a reduction over it (three launches, ~20 us at 11 500 rows)
        src = getattr(center_log_variance, "_evae_prior_scalar", None)
        # (the tag is trusted only while the tensor still IS the stride-0 expansion of that one value: any op that produced new
        # storage dropped the tag, and this check refuses a tag someone copied onto other data -- ADVICE r03)
        if (src is not None and src.numel() == 1 and center_log_variance.dim() == 2 and center_log_variance.stride(0) == 0
                and center_log_variance.stride(1) == 0
                and center_log_variance.untyped_storage().data_ptr() == src.untyped_storage().data_ptr()):
            lv_row = src.reshape(1).expand(center_log_variance.shape[1]).contiguous()
        else:
            lv_row = center_log_variance[0, :].contiguous()
        zi = z_indices.reshape(-1) if masked else None
        ci = center_indices.to(z.device).reshape(-1) if masked else None
        emb_sharded = getattr(exemplars_embedding, 'sharded_total', None)
        if emb_sharded is not None:
            if not test and getattr(self.args, 'shard_batch', False) and shard.is_active():
                # every rank holds its own batch (args.shard_batch): the queries of all ranks meet this rank's shard
                return shard.ShardedPriorLogPBatch.apply(z, centers, lv_row, zi, ci, emb_sharded)
            return shard.ShardedPriorLogP.apply(z, centers, lv_row, zi, ci, emb_sharded)
        return ops.prior_logp(z, centers, lv_row, zi, ci)

    def add_pseudoinputs(self):
        nonlinearity = nn.Hardtanh(min_val=0.0, max_val=1.0)
        self.means = NonLinear(self.args.number_components, int(np.prod(self.args.input_size)), bias=False,
                               activation=nonlinearity)
        if self.args.use_training_data_init:
            self.means.linear.weight.data = self.args.pseudoinputs_mean
        else:
            normal_init(self.means.linear, self.args.pseudoinputs_mean, self.args.pseudoinputs_std)
        self.idle_input = torch.eye(self.args.number_components, self.args.number_components).to(self.args.device)

    # ------------------------------------------------------------------ generation helpers (not accelerated)
    def generate_z_interpolate(self, exemplars_embedding=None, dim=0):
        emb, _, _ = exemplars_embedding
        steps = 10
        step = (emb[1] - emb[0]) / steps
        return torch.stack([emb[0] + i * step for i in range(steps)], dim=0)

    def generate_z(self, N=25, dataset=None):
        if self.args.prior == 'standard':
            return torch.randn(N, self.args.z1_size, device=self.args.device)
        if self.args.prior == 'vampprior':
            means = self.pseudo_inputs()[0:N]
            mu, logvar = self.q_z(means)
            return self.reparameterize(mu, logvar)
        rand_indices = torch.randint(low=0, high=self.args.training_set_size, size=(N,))
        exemplars = dataset.tensors[0][rand_indices]
        mu, logvar = self.q_z(exemplars.to(self.args.device), prior=True)
        return self.reparameterize(mu, logvar.contiguous())

    def reference_based_generation_z(self, N=25, reference_image=None):
        pseudo, log_var = self.q_z(reference_image.to(self.args.device), prior=True)
        pseudo = pseudo.unsqueeze(1).expand(-1, N, -1).reshape(-1, pseudo.shape[-1])
        log_var = log_var[0].unsqueeze(0).expand(len(pseudo), -1)
        z = self.reparameterize(pseudo.contiguous(), log_var.contiguous())
        return z.reshape(-1, N, pseudo.shape[1])

    def reconstruct_x(self, x):
        x_reconstructed, _, z = self.forward(x)
        if self.args.model_name == 'pixelcnn':              # reference :178-179: sampled from the decoder, not its teacher-forced mean
            x_reconstructed = self.pixelcnn_generate(z[0].reshape(-1, self.args.z1_size), z[3].reshape(-1, self.args.z2_size))
        return x_reconstructed

    def logit_inverse(self, x):
        lambd = self.args.lambd
        return (torch.sigmoid(x) - lambd) / (1 - 2 * lambd)

    def generate_x(self, N=25, dataset=None):
        return self.generate_x_from_z(self.generate_z(N=N, dataset=dataset))

    def reference_based_generation_x(self, N=25, reference_image=None):
        return self.generate_x_from_z(self.reference_based_generation_z(N=N, reference_image=reference_image))

    def generate_x_interpolate(self, exemplars_embedding, dim=0):
        zs = self.generate_z_interpolate(exemplars_embedding, dim=dim)
        return self.generate_x_from_z(zs, with_reparameterize=False)

    def reshape_variance(self, variance, shape):
        return variance[0] * torch.ones(shape).to(self.args.device)

    # ------------------------------------------------------------------ encoder
    def _is_conv(self):
        return 'conv' in self.args.model_name or self.args.model_name == 'pixelcnn'      # (reference :206)

    def _encode_rows(self, layers, x, rows=None):
        """Run an encoder stack; for dense stacks `rows` gathers x[rows] inside the first layer's GEMM."""
        if rows is None:
            return layers(x)
        if self._is_conv():
            return layers(x[rows])          # conv stacks: gather first, then the HIP convolution kernels (utils/nn.py)
        mods = list(layers)
        if x.dtype == torch.uint8:          # the byte store (resident_u8): pixel = byte / U8_DIV, first layer on the byte kernels
            h = mods[0](x, rows=rows, x_scale=1.0 / self.U8_DIV)
        else:
            h = mods[0](x, rows=rows)
        for m in mods[1:]:
            h = m(h)
        return h

    def _exemplar_store(self, dataset):
        """What the exemplar rows are gathered from on the modular path: the uint8 store when the data are k/255 and the
        encoder starts with a plain GatedDense (utils/nn.py: gate on, no activation), the fp32 copy otherwise."""
        if not self._is_conv() and os.environ.get("EVAE_U8_MODULAR", "1") != "0":
            first = list(self.q_z_layers)[0]
            if type(first).__name__ == "GatedDense" and first.no_attention is False and first.activation is None \
                    and first.h.weight.shape[1] % 16 == 0:
                u8 = self.resident_u8(dataset)
                if u8 is not None:
                    return u8[0][:u8[1]]
        return self.resident_data(dataset)

    def q_z(self, x, prior=False, rows=None):
        """q(z|x) mean / log-variance (reference :205-221).  `rows` (extension): int64 device indices; the
        encoder then reads x[rows] without materialising the gathered copy."""
        if self._is_conv():
            x = x.view(-1, self.args.input_size[0], self.args.input_size[1], self.args.input_size[2])
        h = self._encode_rows(self.q_z_layers, x, rows)
        if self.args.model_name in ('convhvae_2level', 'pixelcnn'):
            h = h.reshape(h.size(0), -1)         # conv outputs may be channels-last tensors
        z_q_mean = self.q_z_mean(h)
        n = h.shape[0]
        if prior is True and self.args.prior == 'exemplar_prior':
            z_q_logvar = self.prior_log_variance.expand(n, self.args.z1_size)
        else:
            z_q_logvar = self.q_z_logvar(h)
        z_q_logvar = z_q_logvar.reshape(-1, self.args.z1_size)
        if prior is True and self.args.prior == 'exemplar_prior':
            z_q_logvar._evae_prior_scalar = self.prior_log_variance       # (see log_p_z)
        if hasattr(self.q_z_layers, 'clear_heads'):
            self.q_z_layers.clear_heads()        # (fully_conv: a head weight nobody fetched -- q_z_logvar's under prior=True -- must not outlive the pass)
        return z_q_mean.reshape(-1, self.args.z1_size), z_q_logvar

    def cache_z(self, dataset, prior=True, cuda=True):
        """Encode the whole dataset in 10 000-row chunks (reference :223-241) from the HBM-resident copy."""
        data = self.resident_data(dataset)
        step = 10000
        zs, lvs = [], []
        for s in range(0, len(data), step):
            m, lv = self.q_z(data[s:s + step], prior=prior)
            zs.append(m)
            lvs.append(lv)
        return torch.cat(zs, dim=0), torch.cat(lvs, dim=0)

    def cache_z_shard(self, dataset, prior=True):
        """This rank's contiguous row block of cache_z (cached / eval mode): rows [lo, hi) of the dataset encoded in
        10 000-row chunks -> ShardedEmbedding((z [n_local x z], logvar, arange(lo, hi)), total = N).  log_p_z merges the ranks'
        partial log-sum-exps (shard.ShardedPriorLogP); the log-variance keeps at least one row (only row 0 is read, reference
        BaseModel.py:101), so an empty block is a valid embedding too."""
        data = self.resident_data(dataset)
        lo, hi = shard.shard_rows(len(data))
        step = 10000
        zs, lvs = [], []
        for s in range(lo, hi, step):
            m, lv = self.q_z(data[s:min(s + step, hi)], prior=prior)
            zs.append(m)
            lvs.append(lv)
        if zs:
            z, lv = torch.cat(zs, dim=0), torch.cat(lvs, dim=0)
        else:
            z = torch.zeros((0, self.args.z1_size), device=data.device)
            lv = self.q_z(data[:1], prior=prior)[1]
        idx = torch.arange(lo, hi, device=data.device)
        return shard.ShardedEmbedding((z, lv, idx), total=len(data))

    STAGING_ROWS = 1024      # rows kept behind the resident dataset for the current batch (fused path)

    def resident_data_ext(self, dataset, batch_rows=0):
        """(buffer [(N + STAGING_ROWS) x D], N): device-resident fp32 copy of dataset.tensors[0], uploaded once
        per dataset object, followed by staging rows the fused training path copies the batch into."""
        src = dataset.tensors[0]
        key = id(dataset)
        hit = self._resident.get(key)
        need = max(self.STAGING_ROWS, int(batch_rows))
        if hit is None or hit[0] is not src or hit[1].shape[0] < src.shape[0] + need:
            flat = src.reshape(src.shape[0], -1)
            buf = torch.empty((flat.shape[0] + need, flat.shape[1]), device=self.args.device, dtype=torch.float32)
            buf[:flat.shape[0]].copy_(flat)
            buf[flat.shape[0]:].zero_()
            self._resident[key] = (src, buf)
        return self._resident[key][1], src.shape[0]

    U8_DIV = 255.0

    def resident_u8(self, dataset, batch_rows=0):
        """(store [(N + staging) x D] uint8, N, 255.0) when every value of dataset.tensors[0] is k/255 exactly (what
        reference utils/load_data/base_load_data.py:39-40 produces for binary / grey inputs) and rows are 16-byte multiples;
        None otherwise (logit-transformed or (k + 0.5)/256 data stay fp32).  Checked and uploaded once per dataset object.
        EVAE_U8_STORE=0 turns the byte store off."""
        if os.environ.get("EVAE_U8_STORE", "1") == "0":
            return None
        src = dataset.tensors[0]
        key = id(dataset)
        n = src.shape[0]
        need = max(self.STAGING_ROWS, int(batch_rows))
        hit = self._resident_u8.get(key)
        if hit is not None and hit[0] is src and (hit[1] is None or hit[1].shape[0] >= n + need):
            return None if hit[1] is None else (hit[1], n, self.U8_DIV)
        flat = src.reshape(n, -1)
        D = flat.shape[1]
        buf = None
        if D % 16 == 0 and flat.dtype == torch.float32 and n > 0:
            store = torch.zeros((n + need) * D + 64, dtype=torch.uint8, device=self.args.device)   # + slack behind the last row
            buf = store[:(n + need) * D].view(n + need, D)
            bad = torch.zeros((), dtype=torch.int64, device=self.args.device)     # accumulated on the device: ONE sync per dataset
            for s0 in range(0, n, 8192):
                f = flat[s0:s0 + 8192].to(self.args.device)
                q = torch.round(f * self.U8_DIV)
                bad += ((q < 0) | (q > 255) | (q / self.U8_DIV != f)).sum()
                buf[s0:s0 + f.shape[0]] = q.clamp_(0, 255).to(torch.uint8)
            if int(bad) != 0:
                buf = store = None
        self._resident_u8[key] = (src, buf)
        return None if buf is None else (buf, n, self.U8_DIV)

    def resident_data(self, dataset):
        """Device-resident fp32 view [N x D] of dataset.tensors[0]."""
        buf, n = self.resident_data_ext(dataset)
        return buf[:n]

    def _indices_to_device(self, idx_cpu):
        """CPU int64 index vector -> device, without stalling the stream: `.to(device)` of pageable memory waits for the
        GPU to drain (0.46 ms per eager step at the headline configuration).  Two pinned staging buffers take turns; an
        event per buffer says when its upload has been consumed."""
        if idx_cpu.is_cuda:
            return idx_cpu
        st = self.__dict__.setdefault('_idx_staging', {'k': 0, 'pin': [None, None], 'ev': [None, None]})
        k = st['k'] = st['k'] ^ 1
        n = idx_cpu.numel()
        if st['pin'][k] is None or st['pin'][k].numel() < n:
            st['pin'][k] = torch.empty(max(n, 1024), dtype=torch.int64).pin_memory()
            st['ev'][k] = torch.cuda.Event()
        st['ev'][k].synchronize()
        pin = st['pin'][k][:n]
        pin.copy_(idx_cpu.reshape(-1))
        out = torch.empty(n, dtype=torch.int64, device=self.args.device)
        out.copy_(pin, non_blocking=True)
        st['ev'][k].record()
        return out.reshape(idx_cpu.shape)

    def _dedup_draws(self, local_cpu, pad=8):
        """This process's exemplar draws (CPU int64 [Cl], drawn WITH replacement as the reference does, :245) -> (rows [Cd] device: the
        DISTINCT rows among them, padded to a multiple of `pad` with multiplicity 0; tables (draws, inv, rep, mult) on the device) --
        or None when duplicates are rare (< 8 % of the draws), the set is small, or EVAE_DEDUP / EVAE_DEDUP_EAGER = 0.  The eager
        counterpart of the captured step's distinct-row tables (evae/graph.py): the encoder runs over `rows`, the prior still sees
        every draw (evae.ops.expand_rows / the `dedup` field of evae/handoff.py), the loss and gradients are those of encoding every draw.  Works
        per shard: a rank deduplicates ITS slice of the common draw (r06; VERDICT r05 missing #2)."""
        a = self.args
        Cl = int(local_cpu.numel())
        if (os.environ.get("EVAE_DEDUP", "1") == "0" or os.environ.get("EVAE_DEDUP_EAGER", "1") == "0" or Cl < 1024
                or a.prior != 'exemplar_prior' or a.approximate_prior or int(a.z1_size) % 4 != 0):
            return None
        import ctypes as C_
        lib = ops._lib.load()
        st = self.__dict__.setdefault('_dedup_staging', {'k': 0, 'pin': [None, None], 'ev': [None, None]})
        k = st['k'] = st['k'] ^ 1
        cap = (Cl + pad - 1) // pad * pad
        words = cap + Cl + Cl + cap + (cap + 1) // 2            # rows | draws | inv | rep | mult (fp32 pairs)
        if st['pin'][k] is None or st['pin'][k].numel() < words:
            st['pin'][k] = torch.empty(words, dtype=torch.int64).pin_memory()
            st['ev'][k] = torch.cuda.Event()
        st['ev'][k].synchronize()
        h = st['pin'][k][:words]
        o_draw, o_inv, o_rep, o_mult = cap, cap + Cl, cap + 2 * Cl, 2 * cap + 2 * Cl
        h[o_draw:o_inv].copy_(local_cpu.reshape(-1))
        mult = h[o_mult:].view(torch.float32)
        nu = lib.evae_host_dedup(C_.c_void_p(h[o_draw:].data_ptr()), Cl, int(a.training_set_size), cap, C_.c_void_p(h.data_ptr()),
                                 C_.c_void_p(h[o_inv:].data_ptr()), C_.c_void_p(h[o_rep:].data_ptr()), C_.c_void_p(mult.data_ptr()))
        if nu < 0:
            ops._lib.check(nu, "evae_host_dedup")
        Cd = (nu + pad - 1) // pad * pad
        if Cd > 0.92 * Cl:
            return None
        dev = torch.empty(words, dtype=torch.int64, device=a.device)
        dev.copy_(h, non_blocking=True)
        st['ev'][k].record()
        tables = (dev[o_draw:o_inv], dev[o_inv:o_rep], dev[o_rep:o_rep + Cd], dev[o_mult:].view(torch.float32)[:Cd])
        return dev[:Cd], tables

    # ------------------------------------------------------------------ exemplar sets
    def get_exemplar_set(self, z_mean, z_log_var, dataset, cache, x_indices):
        if self.args.approximate_prior is False:
            h = handoff.current()
            if h is not None and h.rows is not None:
                # graph-captured step (evae/graph.py): this rank's indices already sit in a static device buffer
                local = h.rows[:h.n_rows]
                centres, logvar = self.q_z(self._exemplar_store(dataset), prior=True, rows=local)
                dd = h.dedup
                if dd is not None:
                    # the gather list holds the DISTINCT rows of the draw (evae/graph.py; of this rank's slice of it when
                    # sharded): the prior gets every draw's encoding, log-variance and index -- what the reference's
                    # one-encoding-per-draw hands it (:243-254)
                    centres, logvar, local = self._expand_draws(centres, dd)
                if self._sharded():
                    return shard.ShardedEmbedding((centres, logvar, local), total=self.args.number_components)
                return (centres, logvar, local)
            # same CPU-generator draw, with replacement, as the reference (:245)
            exemplars_indices = torch.randint(low=0, high=self.args.training_set_size,
                                              size=(self.args.number_components,))
            return self._encode_exemplars(dataset, exemplars_indices)
        return self.get_approximate_nearest_exemplars(z=(z_mean, z_log_var, x_indices), dataset=dataset, cache=cache)

    def _expand_draws(self, centres, dd):
        """encodings of the distinct rows -> (encodings, log-variance, dataset indices) of every draw"""
        draws, inv, rep, mult = dd
        centres = ops.expand_rows(centres, inv, rep, mult)
        logvar = self.prior_log_variance.expand(draws.numel(), self.args.z1_size)
        logvar._evae_prior_scalar = self.prior_log_variance
        return centres, logvar, draws

    def _encode_exemplars(self, dataset, exemplars_indices):
        data = self._exemplar_store(dataset)
        lo, hi = shard.bounds(len(exemplars_indices)) if self._sharded() else (0, len(exemplars_indices))
        local_cpu = exemplars_indices[lo:hi]
        dd = self._dedup_draws(local_cpu, pad=1) if (not local_cpu.is_cuda and torch.is_grad_enabled() and self.training) else None
        if dd is not None:
            rows, tables = dd
            centres, _ = self.q_z(data, prior=True, rows=rows)
            centres, logvar, local = self._expand_draws(centres, tables)
        else:
            local = self._indices_to_device(local_cpu)
            centres, logvar = self.q_z(data, prior=True, rows=local)
        if self._sharded():
            return shard.ShardedEmbedding((centres, logvar, local), total=len(exemplars_indices))
        return (centres, logvar, local)

    def get_approximate_nearest_exemplars(self, z, cache, dataset):
        """kNN-pruned exemplar set (reference :256-271): candidates drawn with replacement, the batch's own
        cache rows refreshed, top-k per batch row, union re-encoded with gradient, cache rows refreshed.

        On one device with the leave-one-out mask on, the union is kept in a FIXED list of B * k slots instead of the
        data-dependent `unique`: every slot is re-encoded, the repeats of a position carry c_idx = PRIOR_MASK_ALL, which the
        prior kernels exclude from the mixture and count like leave-one-out hits -- so the denominator is #unique - #hits as
        in the reference, while every shape is static and the whole step can be captured into a hipGraph."""
        h = handoff.current()
        captured = h is not None and h.rows is not None
        if captured:                             # captured step: the candidate draw already sits in a static device buffer
            exemplars_indices = h.rows[:h.n_rows]
        else:
            exemplars_indices = self._indices_to_device(torch.randint(low=0, high=self.args.training_set_size,
                                                                      size=(self.args.number_components,)))
        z, _, indices = z
        cached_z, cached_log_variance = cache
        cached_z[indices.reshape(-1)] = z.detach() if not cached_z.requires_grad else z
        data = self._exemplar_store(dataset)
        if self._sharded():
            # the candidate list is split over the ranks: local top-k over this rank's slice, one all-gather of the
            # R x k (value, candidate position) lists per row, merge -- the exact global top-k on every rank
            lo, hi = shard.bounds(exemplars_indices.numel())
            nearest_indices, _ = shard.sharded_topk(z.detach(), cached_z[exemplars_indices[lo:hi], :].detach(),
                                                    self.args.approximate_k, index_base=lo)
        else:
            sub_cache = cached_z[exemplars_indices, :]
            nearest_indices, _ = ops.pairdist_topk(z.detach(), sub_cache.detach(), self.args.approximate_k, want_val=False)
            # static slots: always for the dense encoders (a repeated slot costs one thin GEMM row), for the convolutional
            # ones only inside a captured step -- re-encoding up to B * k images where `unique` leaves a few dozen is not free
            static = self.args.no_mask is False and (not self._is_conv() or captured)
            if static and nearest_indices.numel() > ops.SELECT_EXEMPLARS_MAX:
                # evae_select_exemplars keeps all B * k positions of a call in one block's LDS: beyond its limit the
                # data-dependent `unique` form below takes over (not capturable: a captured step refuses this size up front)
                if captured:
                    raise RuntimeError("approximate prior: batch_size * approximate_k = %d exceeds the %d static slots a "
                                       "captured step supports; run with use_hip_graph=False"
                                       % (nearest_indices.numel(), ops.SELECT_EXEMPLARS_MAX))
                static = False
            if static:
                sel_rows, c_idx = ops.select_exemplars(nearest_indices.view(-1), exemplars_indices)
                exemplars_z, log_variance = self.q_z(data, prior=True, rows=sel_rows)
                cached_z[sel_rows] = exemplars_z.detach() if not cached_z.requires_grad else exemplars_z
                return (exemplars_z, log_variance, c_idx)
        nearest_indices = torch.unique(nearest_indices.view(-1))
        exemplars_indices = exemplars_indices[nearest_indices].view(-1)
        exemplars_z, log_variance = self.q_z(data, prior=True, rows=exemplars_indices)
        cached_z[exemplars_indices] = exemplars_z.detach() if not cached_z.requires_grad else exemplars_z
        return (exemplars_z, log_variance, exemplars_indices)
