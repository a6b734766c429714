"""PCA of the latent space on the device in fp64 (csrc/evae_pca.hip), behind scikit-learn's names:

    from evae.pca import PCA              # instead of: from sklearn.decomposition import PCA
    Y = PCA(n_components=2).fit_transform(z)           # z [N x d] tensor or array -> [N x 2] float32 tensor on the device

What is computed is svd_solver='covariance_eigh' of scikit-learn: the covariance (ddof 1) of the rows centred in fp64, its
eigen-decomposition by a one-workgroup cyclic Jacobi, eigenvalues clamped at 0, components in descending order with the sign
rule of svd_flip(u_based_decision=False) -- in every component the entry of largest magnitude is positive.  d is at most
ops.pca_max_features() = 256 (the widest latent), N at most ops.pca_max_points().  Not carried over: whiten, svd_solver,
n_components as a fraction or 'mle'.  TSNE(init='pca') (evae/tsne.py) is the first user."""
import numpy as np
import torch

from . import ops
from ._lib import EvaeError


class PCA:
    def __init__(self, n_components=None, device=None):
        """n_components: an int in [1, d], or None for d.  device: where a host array given to fit goes (default cuda)."""
        if n_components is not None and (isinstance(n_components, bool) or not isinstance(n_components, (int, np.integer))
                                         or n_components < 1):
            raise ValueError("PCA: n_components=%r; an int >= 1 or None expected" % (n_components,))
        self.n_components, self.device = n_components, device
        self.mean_ = self.components_ = self.explained_variance_ = self.explained_variance_ratio_ = self.singular_values_ = None
        self.n_samples_ = self.n_features_in_ = self.n_components_ = self.n_sweeps_ = None

    def _tensor(self, X):
        if not torch.is_tensor(X):
            X = torch.as_tensor(np.asarray(X, dtype=np.float32), device=self.device or 'cuda')
        return X

    def fit(self, X, y=None):
        """X [N x d] -> self.  mean_ [d], components_ [k x d], explained_variance_ (ddof 1), explained_variance_ratio_ and
        singular_values_ [k] are float64 tensors on the device.  The solver's record and the eigenvalues are read from the device
        once; EvaeError if the solver did not converge within ops.pca_max_sweeps().  An input without variance (all rows equal)
        has no ratios to give: explained_variance_ratio_ is then all zeros, not 0 / 0."""
        X = self._tensor(X)
        if X.dim() == 2 and self.n_components is not None and self.n_components > X.shape[1]:      # before any launch
            raise ValueError("PCA: n_components=%d for %d features" % (self.n_components, X.shape[1]))
        with torch.no_grad():
            mean, cov = ops.pca_moments(X)
            N, d = X.shape
            k = d if self.n_components is None else int(self.n_components)
            evals, evecs, info = ops.pca_eigh(cov)
            record = torch.cat((info, evals)).cpu().numpy()              # the one read
            if record[1] != 1.0:
                raise EvaeError("PCA: the Jacobi solver did not converge in %d sweeps (largest |g_p . g_q| / (|g_p| |g_q|) = %g)"
                                % (int(record[0]), record[2]))
            self.mean_, self.components_ = mean, evecs[:k].contiguous()
            self.explained_variance_ = evals[:k].contiguous()
            if record[4:].sum() > 0.0:                                   # decided on the record already read
                self.explained_variance_ratio_ = self.explained_variance_ / evals.sum()
            else:
                self.explained_variance_ratio_ = torch.zeros_like(self.explained_variance_)
            self.singular_values_ = torch.sqrt(self.explained_variance_ * (N - 1))
        self._explained_variance_host = record[4:4 + k].copy()           # for callers that branch on it without a second read
                                                                         # (TSNE(init='pca'))
        self.n_samples_, self.n_features_in_, self.n_components_, self.n_sweeps_ = N, d, k, int(record[0])
        return self

    def _fitted(self):
        if self.components_ is None:
            raise EvaeError("PCA: fit first")

    def transform(self, X):
        """[N x d] -> [N x k] float32 on the device"""
        self._fitted()
        with torch.no_grad():
            return ops.pca_project(self._tensor(X), self.mean_, self.components_)

    def fit_transform(self, X, y=None):
        X = self._tensor(X)
        return self.fit(X).transform(X)

    def inverse_transform(self, Y):
        """[N x k] -> [N x d] float32 on the device"""
        self._fitted()
        with torch.no_grad():
            return ops.pca_reconstruct(self._tensor(Y), self.mean_, self.components_)
