"""Exact t-SNE on the device (csrc/evae_tsne.hip), behind scikit-learn's constructor names:

    from evae.tsne import TSNE            # instead of: from sklearn.manifold import TSNE
    Y = TSNE(random_state=0).fit_transform(z)          # z [N x zd] tensor or array -> [N x 2] tensor on the device

What is computed is method='exact' of scikit-learn -- all N^2 pairs, every iteration, no Barnes-Hut tree -- with its
gradient-descent rule (gains, momentum 0.5 during the exaggerated phase and 0.8 after it, learning_rate 'auto') plus the
re-centring of the embedding after every step.  Not carried over: the early exits (`min_grad_norm`,
`n_iter_without_progress`: all n_iter iterations always run, so n_iter_ == n_iter), init='pca', metrics other than the
squared Euclidean distance, n_components other than 2, method='barnes_hut'.

The cap on N: a row of distances has to fit one workgroup's LDS during the precision search (64 B + 4 N <= 160 KiB), so
N <= 32768 (ops.tsne_max_points()).  The dense buffers at the cap: the [N x N] float32 matrix that holds the distances, then
the conditionals, then P, in place, 4 N^2 B = 4 GiB, plus 64 N B of per-point sums and 24 N B of descent state."""
import numpy as np
import torch

from . import ops

EXAGGERATED_ITERS = 250      # scikit-learn's _EXPLORATION_MAX_ITER
_INIT_STD = 1e-4


class TSNE:
    def __init__(self, n_components=2, perplexity=30.0, early_exaggeration=12.0, learning_rate='auto', n_iter=1000,
                 random_state=None, init='random', exaggerated_iters=EXAGGERATED_ITERS, device=None):
        """exaggerated_iters: how many of the n_iter iterations run with early_exaggeration and momentum 0.5 (scikit-learn
        fixes 250; short runs in tests and documents shorten it in proportion).  init: 'random' -- N(0, 1e-4^2) from a
        torch.Generator on the device seeded with random_state -- or a [N x 2] tensor / array.  device: where a host array
        given to fit_transform goes (default cuda)."""
        if n_components != 2:
            raise ValueError("TSNE: n_components=%r; the kernels embed in 2 dimensions only" % (n_components,))
        if not (torch.is_tensor(init) or isinstance(init, np.ndarray) or init == 'random'):
            raise ValueError("TSNE: init must be 'random' or a [N x 2] tensor (init='pca' is not carried over)")
        if learning_rate != 'auto' and not float(learning_rate) > 0:
            raise ValueError("TSNE: learning_rate must be 'auto' or positive")
        if int(n_iter) < 1 or not 0 <= int(exaggerated_iters):
            raise ValueError("TSNE: n_iter >= 1 and exaggerated_iters >= 0 expected")
        self.n_components, self.perplexity, self.early_exaggeration = 2, float(perplexity), float(early_exaggeration)
        self.learning_rate, self.n_iter, self.random_state, self.init = learning_rate, int(n_iter), random_state, init
        self.exaggerated_iters, self.device = int(exaggerated_iters), device
        self.embedding_ = self.kl_divergence_ = self.n_iter_ = self.learning_rate_ = None

    def _initial(self, N, device):
        if torch.is_tensor(self.init) or isinstance(self.init, np.ndarray):
            Y = torch.as_tensor(self.init).to(device=device, dtype=torch.float32).clone().contiguous()
            if tuple(Y.shape) != (N, 2):
                raise ValueError("TSNE: init of shape %s for %d points" % (tuple(Y.shape), N))
            return Y
        gen = torch.Generator(device=device)
        if self.random_state is None:
            gen.seed()
        else:
            gen.manual_seed(int(self.random_state))
        return torch.randn((N, 2), generator=gen, device=device, dtype=torch.float32) * _INIT_STD

    def fit_transform(self, X, y=None):
        """X [N x zd] tensor or array -> the embedding [N x 2], float32 on the device; sets embedding_, kl_divergence_ (KL(P || Q)
        at the returned embedding, un-exaggerated P), n_iter_ and learning_rate_."""
        shape = tuple(X.shape) if torch.is_tensor(X) else np.shape(X)
        if len(shape) != 2:
            raise ValueError("TSNE: a [N x zd] input expected, got %s" % (shape,))
        N = shape[0]
        if self.perplexity >= N:
            raise ValueError("TSNE: perplexity %g must be less than the number of points %d" % (self.perplexity, N))
        if N > ops.tsne_max_points():
            raise ValueError("TSNE: %d points; the exact kernels take at most %d (a row of distances in one workgroup's LDS; "
                             "the dense matrix is 4 N^2 bytes)" % (N, ops.tsne_max_points()))
        if not torch.is_tensor(X):
            X = torch.as_tensor(np.asarray(X, dtype=np.float32), device=self.device or 'cuda')
        if self.learning_rate == 'auto':
            lr = max(N / self.early_exaggeration / 4.0, 50.0)
        else:
            lr = float(self.learning_rate)
        self.learning_rate_ = lr
        with torch.no_grad():
            P, _ = ops.tsne_affinities(X, self.perplexity)
            Y = self._initial(N, P.device)
            velocity = torch.zeros_like(Y)
            gains = torch.ones_like(Y)
            for it in range(self.n_iter):
                early = it < self.exaggerated_iters
                part = ops.tsne_forces(P, Y, self.early_exaggeration if early else 1.0, False)
                ops.tsne_update(part, Y, velocity, gains, 0.5 if early else 0.8, lr)
            stats = ops.tsne_stats(ops.tsne_forces(P, Y, 1.0, True), True)
        self.kl_divergence_ = float(stats[1].item())
        self.n_iter_ = self.n_iter
        self.embedding_ = Y
        return Y

    def fit(self, X, y=None):
        self.fit_transform(X)
        return self
