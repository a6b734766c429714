"""Gaussian mixture of the latent space on the device in fp64 (csrc/evae_gmm.hip), behind scikit-learn's names:

    from evae.mixture import GaussianMixture                 # instead of sklearn.mixture
    gm = GaussianMixture(n_components=10, random_state=0).fit(z)     # z [N x d] tensor or array
    gm.score_samples(z_test); gm.predict_proba(z_test); gm.sample(64)

What is computed is scikit-learn's GaussianMixture for covariance_type 'full', 'diag' and 'spherical': the E-step through the
upper-triangular precision factors (precisions_cholesky_), the M-step with covariances about the new means (two passes, never
E[xx] - mu mu^T), reg_covar on the diagonal, and scikit-learn's loop and stop -- E-step, M-step, then |bound - previous| < tol,
so lower_bound_ is the bound under the parameters before the last M-step.  Equal inputs and equal random_state give bit-equal
attributes.  The iterations run on the device: the host issues check_every of them blind -- every kernel returns at once after
the record's done flag is set -- and reads the 64-byte record once per batch.

Not carried over: covariance_type='tied' (ValueError), warm_start, init_params 'k-means++' / 'random_from_data', verbose.  The
k-means of init_params='kmeans' is evae.cluster.KMeans, whose seeds differ from scikit-learn's for the same random_state.
K <= 256, N <= 2^20, d <= 96 for 'full' (the factor of a component lives in LDS) and <= 256 for 'diag' / 'spherical'; a shape
whose responsibilities plus workspace exceed 1 GiB is refused.  Wider latents go through evae.pca first or use 'diag'."""
import numpy as np
import torch

from . import ops
from ._fit import _blind_batches, _generator, _int_at_least, _rows, _shape
from ._lib import EvaeError
from .cluster import KMeans

COVARIANCE_TYPES = ('full', 'diag', 'spherical')
INIT_PARAMS = ('kmeans', 'random')

ILL_DEFINED = ("Fitting the mixture model failed because some components have ill-defined empirical covariance (for instance "
               "caused by singleton or collapsed samples). Try to decrease the number of components, increase reg_covar, or "
               "scale the input data. The first such component is %d.")


def _f64(a):
    """tensor or array -> float64 CPU tensor (an initialisation the caller brings)"""
    t = a.detach().cpu() if torch.is_tensor(a) else torch.as_tensor(np.asarray(a, dtype=np.float64))
    return t.to(torch.float64).contiguous()


def n_parameters(n_components, n_features, covariance_type):
    """free parameters of the model: scikit-learn's _n_parameters"""
    K, d = int(n_components), int(n_features)
    cov = {'full': K * d * (d + 1) // 2, 'diag': K * d, 'spherical': K}[covariance_type]
    return cov + K * d + K - 1


class GaussianMixture:
    def __init__(self, n_components=1, covariance_type='full', tol=1e-3, reg_covar=1e-6, max_iter=100, n_init=1,
                 init_params='kmeans', weights_init=None, means_init=None, precisions_init=None, random_state=None, check_every=4,
                 device=None):
        """init_params: 'kmeans' (the labels of evae.cluster.KMeans(n_components, n_init=1, random_state=random_state + run) as
        one-hot responsibilities; a fresh seed per run when random_state is None) or 'random' (uniform responsibilities in
        float64, normalised per row).  weights_init [K], means_init [K x d], precisions_init ([K x d x d], [K x d] or [K]) replace
        what the initial M-step gave, as scikit-learn's.  n_init: runs; the one of highest lower bound wins (ties: the first).
        random_state seeds a CPU torch.Generator all draws come from; None draws a seed.  check_every: iterations issued between
        two reads of the device's record.  device: where a host array given to fit goes (default cuda)."""
        n_components = _int_at_least("GaussianMixture", "n_components", n_components, 1)
        if covariance_type == 'tied':
            raise ValueError("GaussianMixture: covariance_type='tied' is not carried over; 'full', 'diag' or 'spherical' expected")
        if covariance_type not in COVARIANCE_TYPES:
            raise ValueError("GaussianMixture: covariance_type=%r; 'full', 'diag' or 'spherical' expected" % (covariance_type,))
        if init_params not in INIT_PARAMS:
            raise ValueError("GaussianMixture: init_params=%r; 'kmeans' or 'random' expected" % (init_params,))
        if n_components > ops.gmm_max_components():
            raise ValueError("GaussianMixture: n_components=%d above the cap of %d" % (n_components, ops.gmm_max_components()))
        max_iter = _int_at_least("GaussianMixture", "max_iter", max_iter, 1)
        n_init = _int_at_least("GaussianMixture", "n_init", n_init, 1)
        check_every = _int_at_least("GaussianMixture", "check_every", check_every, 1)
        if not float(tol) >= 0.0:
            raise ValueError("GaussianMixture: tol=%r; a number >= 0 expected" % (tol,))
        if not float(reg_covar) >= 0.0:
            raise ValueError("GaussianMixture: reg_covar=%r; a number >= 0 expected" % (reg_covar,))
        if weights_init is not None:
            w = _f64(weights_init)
            if tuple(w.shape) != (n_components,):
                raise ValueError("GaussianMixture: weights_init of shape %s, [%d] expected" % (tuple(w.shape), n_components))
            if bool((w < 0).any()) or bool((w > 1).any()) or abs(float(w.sum()) - 1.0) > 1e-8:
                raise ValueError("GaussianMixture: weights_init must lie in [0, 1] and sum to 1")
        if means_init is not None and (len(_shape(means_init)) != 2 or _shape(means_init)[0] != n_components):
            raise ValueError("GaussianMixture: means_init of shape %s for n_components=%d" % (_shape(means_init), n_components))
        if precisions_init is not None:
            want = {'full': 3, 'diag': 2, 'spherical': 1}[covariance_type]
            if len(_shape(precisions_init)) != want or _shape(precisions_init)[0] != n_components:
                raise ValueError("GaussianMixture: precisions_init of shape %s for n_components=%d, covariance_type=%r"
                                 % (_shape(precisions_init), n_components, covariance_type))
        self.n_components, self.covariance_type, self.tol, self.reg_covar = n_components, covariance_type, float(tol), float(reg_covar)
        self.max_iter, self.n_init, self.init_params = max_iter, n_init, init_params
        self.weights_init, self.means_init, self.precisions_init = weights_init, means_init, precisions_init
        self.random_state, self.check_every, self.device = random_state, check_every, device
        self.weights_ = self.means_ = self.covariances_ = self.precisions_cholesky_ = None
        self.converged_ = self.n_iter_ = self.lower_bound_ = self.n_features_in_ = None
        self._params = None

    # ------------------------------------------------------------------------------------------------------------ checks
    def _check(self, shape):
        """what is known from the arguments and the shape: refused before any launch"""
        if len(shape) != 2:
            raise ValueError("GaussianMixture: a [N x d] input expected, got %s" % (shape,))
        N, d = shape
        K, ctype = self.n_components, self.covariance_type
        if N < 2:
            raise ValueError("GaussianMixture: N=%d; at least 2 points expected" % N)
        if N < K:
            raise ValueError("GaussianMixture: n_components=%d for N=%d points" % (K, N))
        if N > ops.gmm_max_points():
            raise ValueError("GaussianMixture: N=%d above the cap of %d points" % (N, ops.gmm_max_points()))
        if not 1 <= d <= ops.gmm_max_features(ctype):
            raise ValueError("GaussianMixture: %d features outside [1, %d] for covariance_type=%r; reduce them with evae.pca%s"
                             % (d, ops.gmm_max_features(ctype), ctype, " or use 'diag'" if ctype == 'full' else ""))
        try:
            ops.gmm_check_sizes(N, d, K, ctype, "GaussianMixture")
        except EvaeError as e:
            raise ValueError(str(e))
        if self.means_init is not None and _shape(self.means_init) != (K, d):
            raise ValueError("GaussianMixture: means_init of shape %s, [%d x %d] expected" % (_shape(self.means_init), K, d))
        if self.precisions_init is not None:
            want = {'full': (K, d, d), 'diag': (K, d), 'spherical': (K,)}[ctype]
            if _shape(self.precisions_init) != want:
                raise ValueError("GaussianMixture: precisions_init of shape %s, %s expected" % (_shape(self.precisions_init), want))

    def _raise_if_failed(self, record):
        if record[5] >= 0.0:
            raise ValueError(ILL_DEFINED % int(record[5]))

    # ------------------------------------------------------------------------------------------------------------ the fit
    def _factor_of_precisions(self):
        """precisions_init -> scikit-learn's precisions_cholesky_ of it, float64 on the host (an initialisation, once)"""
        prec = _f64(self.precisions_init)
        if self.covariance_type != 'full':
            return torch.sqrt(prec)
        flipped = torch.flip(prec, dims=(1, 2))
        return torch.flip(torch.linalg.cholesky(flipped), dims=(1, 2)).contiguous()

    def _initial(self, x, g, run, ws):
        """the parameters one run starts from: a fresh buffer"""
        N, d = x.shape
        K, ctype = self.n_components, self.covariance_type
        params = ops.gmm_params(d, K, ctype, x.device)
        views = ops.gmm_views(params, d, K, ctype)
        given_all = self.weights_init is not None and self.means_init is not None and self.precisions_init is not None
        if not given_all:
            state = ops.gmm_state(x.device)
            if self.init_params == 'kmeans':
                seed = None if self.random_state is None else int(self.random_state) + run
                labels = KMeans(K, n_init=1, random_state=seed).fit(x).labels_
                ops.gmm_mstep(x, params, K, ctype, self.reg_covar, state, labels=labels, ws=ws)
            else:
                resp = torch.rand((N, K), dtype=torch.float64, generator=g)
                resp /= resp.sum(dim=1, keepdim=True)
                ops.gmm_mstep(x, params, K, ctype, self.reg_covar, state, log_resp=torch.log(resp).to(x.device), ws=ws)
            if self.precisions_init is None:
                self._raise_if_failed(state.cpu().numpy())
        else:
            params.zero_()
        if self.weights_init is not None:
            views['weights'].copy_(_f64(self.weights_init))
        if self.means_init is not None:
            views['means'].copy_(_f64(self.means_init))
        if self.precisions_init is not None:
            views['precisions_cholesky'].copy_(self._factor_of_precisions())
        if self.means_init is not None or self.precisions_init is not None:
            ops.gmm_prepare(params, d, K, ctype)
        return params

    def _em(self, x, params, ws, log_resp, logp):
        """params in place -> the record: batches of check_every blind steps, one read of the record per batch"""
        state = ops.gmm_state(x.device)
        return _blind_batches(lambda: ops.gmm_step(x, params, self.n_components, self.covariance_type, log_resp, logp,
                                                   self.reg_covar, self.tol, state, ws), state, self.max_iter, self.check_every)

    def _fit(self, X):
        self._check(_shape(X))
        x = _rows(X, self.device)
        N, d = x.shape
        K, ctype = self.n_components, self.covariance_type
        with torch.no_grad():
            ws = ops.gmm_workspace(N, d, K, ctype, x.device)
            log_resp = torch.empty((N, K), dtype=torch.float64, device=x.device)
            logp = torch.empty(N, dtype=torch.float64, device=x.device)
            g = _generator(self.random_state)
            best = None
            for run in range(self.n_init):
                params = self._initial(x, g, run, ws)
                record = self._em(x, params, ws, log_resp, logp)
                self._raise_if_failed(record)
                if best is None or record[3] > best[0]:
                    best = (float(record[3]), params, int(record[0]), bool(record[2] != 0.0))
            self.lower_bound_, self._params, self.n_iter_, self.converged_ = best
            views = ops.gmm_views(self._params, d, K, ctype)
            self.weights_, self.means_ = views['weights'], views['means']
            self.covariances_, self.precisions_cholesky_ = views['covariances'], views['precisions_cholesky']
            self.n_features_in_ = d
            ops.gmm_estep(x, self._params, K, ctype, ws, log_resp, logp)          # the labels belong to the final parameters
            return ops.gmm_argmax(log_resp)

    def fit(self, X, y=None):
        """X [N x d] -> self.  weights_ [K], means_ [K x d], covariances_ and precisions_cholesky_ ([K x d x d], [K x d] or [K])
        float64 on the device; converged_, n_iter_, lower_bound_ of the winning run.  Reaching max_iter sets converged_ = False
        and is not an error.  ValueError (scikit-learn's) when a component's covariance is not positive definite."""
        self._fit(X)
        return self

    def fit_predict(self, X, y=None):
        """fit, then int32 [N] labels on the device from one closing E-step under the final parameters"""
        return self._fit(X)

    # ------------------------------------------------------------------------------------------------------------ densities
    def _estep(self, X):
        if self._params is None:
            raise EvaeError("GaussianMixture: fit first")
        shape = _shape(X)
        if len(shape) != 2 or shape[1] != self.n_features_in_:
            raise ValueError("GaussianMixture: a [N x %d] input expected, got %s" % (self.n_features_in_, shape))
        with torch.no_grad():
            return ops.gmm_estep(_rows(X, self.device), self._params, self.n_components, self.covariance_type)

    def score_samples(self, X):
        """[N x d] -> float64 [N] on the device: log p(x_i)"""
        return self._estep(X)[1]

    def score(self, X, y=None):
        """the mean of score_samples (a fixed-order fp64 sum on the device), as a float"""
        return float(self._estep(X)[2].item())

    def predict_proba(self, X):
        """[N x d] -> float64 [N x K] on the device: the responsibilities.  exp(log_resp) carries the rounding of log p(x_i), the
        same for a whole row (|log p| eps, tens of eps); divided by its own sum a row adds up to 1 within K eps."""
        r = torch.exp(self._estep(X)[0])
        return r / r.sum(dim=1, keepdim=True)

    def predict(self, X):
        """[N x d] -> int32 [N] on the device: the component of largest responsibility, the lowest on a tie"""
        with torch.no_grad():
            return ops.gmm_argmax(self._estep(X)[0])

    def _n_parameters(self):
        return n_parameters(self.n_components, self.n_features_in_, self.covariance_type)

    def bic(self, X):
        n = _shape(X)[0]
        return -2.0 * self.score(X) * n + self._n_parameters() * float(np.log(n))

    def aic(self, X):
        return -2.0 * self.score(X) * _shape(X)[0] + 2.0 * self._n_parameters()

    # ------------------------------------------------------------------------------------------------------------ sampling
    def sample_draws(self, n_samples=1):
        """-> (components int32 [n] ascending, normals float64 [n x d]) on the host: component counts by a multinomial over
        weights_ and standard normals, both from a CPU generator seeded with random_state"""
        if self._params is None:
            raise EvaeError("GaussianMixture: fit first")
        n = _int_at_least("GaussianMixture", "n_samples", n_samples, 1)
        if n > ops.gmm_max_points():
            raise ValueError("GaussianMixture: n_samples=%d above the cap of %d" % (n, ops.gmm_max_points()))
        g = _generator(self.random_state)
        w = self.weights_.cpu().clamp_min(0.0)
        draws = torch.multinomial(w, n, replacement=True, generator=g)
        counts = torch.bincount(draws, minlength=self.n_components)
        comp = torch.repeat_interleave(torch.arange(self.n_components, dtype=torch.int32), counts)
        eps = torch.randn((n, self.n_features_in_), dtype=torch.float64, generator=g)
        return comp, eps

    def sample(self, n_samples=1):
        """-> (z float32 [n x d] on the device, components int32 [n] on the device, ascending): z_i = mu_c + L_c eps_i with
        L_c = (P_c^T)^-1 the factor of the component's covariance, in fp64, rounded once"""
        comp, eps = self.sample_draws(n_samples)
        dev = self._params.device
        comp, eps = comp.to(dev), eps.to(dev)
        with torch.no_grad():
            return ops.gmm_sample(self._params, self.n_features_in_, self.n_components, self.covariance_type, comp, eps), comp
