"""Exact t-SNE on the device (csrc/evae_tsne.hip), behind scikit-learn's constructor names:

    from evae.tsne import TSNE            # instead of: from sklearn.manifold import TSNE
    Y = TSNE(random_state=0).fit_transform(z)          # z [N x zd] tensor or array -> [N x 2] tensor on the device

What is computed is method='exact' of scikit-learn -- all N^2 pairs, every iteration, no Barnes-Hut tree -- with its
gradient-descent rule (gains, momentum 0.5 during the exaggerated phase and 0.8 after it, learning_rate 'auto') plus the
re-centring of the embedding after every step.  Not carried over: the early exits (`min_grad_norm`,
`n_iter_without_progress`: all n_iter iterations always run, so n_iter_ == n_iter), metrics other than the squared Euclidean
distance, n_components other than 2, method='barnes_hut'.  init='pca' (scikit-learn's default since 1.2; here 'random' stays
the default) starts from the first two principal components of the input (evae/pca.py, svd_solver 'full' up to rounding, not
scikit-learn's 'randomized'), rescaled so that the population standard deviation of the first column is 1e-4; no generator is
touched, so the embedding does not depend on random_state.

The cap on N: a row of distances has to fit one workgroup's LDS during the precision search (64 B + 4 N <= 160 KiB), so
N <= 32768 (ops.tsne_max_points()).  The dense buffers at the cap: the [N x N] float32 matrix that holds the distances, then
the conditionals, then P, in place, 4 N^2 B = 4 GiB, plus 64 N B of per-point sums and 24 N B of descent state.

method='neighbours' (csrc/evae_tsne_nn.hip) lifts that cap to ops.tsne_nn_max_points(): scikit-learn's large-N
formulation without its tree.  P lives only on each point's k = min(N - 1, floor(3 perplexity) + 1) nearest neighbours (its
_joint_probabilities_nn, symmetrised, in CSR), the attractive sum runs over those non-zeros, the repulsive sum and Z stay exact
over all N^2 pairs (Barnes-Hut at angle 0).  No [N x N] buffer exists; k <= 256, i.e. perplexity up to 85.  The descent loop,
learning rate, init and attributes are the same, and equal random_state still gives bit-equal embeddings.  method='exact' is
the default and is untouched.

trustworthiness / continuity / embedding_quality below (csrc/evae_nn_rank.hip) score an embedding against its input
without reference to P, so the two methods -- or any later change to either -- can be compared: scikit-learn's trustworthiness,
its mirror image and the share of preserved neighbours, exact integers from one counting pass per direction over all N^2 pairs."""
import numpy as np
import torch

from . import ops
from .pca import PCA

EXAGGERATED_ITERS = 250      # scikit-learn's _EXPLORATION_MAX_ITER
_INIT_STD = 1e-4
METHODS = ('exact', 'neighbours')


class TSNE:
    def __init__(self, n_components=2, perplexity=30.0, early_exaggeration=12.0, learning_rate='auto', n_iter=1000,
                 random_state=None, init='random', exaggerated_iters=EXAGGERATED_ITERS, device=None, method='exact'):
        """exaggerated_iters: how many of the n_iter iterations run with early_exaggeration and momentum 0.5 (scikit-learn
        fixes 250; short runs in tests and documents shorten it in proportion).  init: 'random' -- N(0, 1e-4^2) from a
        torch.Generator on the device seeded with random_state --, 'pca' -- the input's first two principal components with the
        first column's standard deviation scaled to 1e-4, independent of random_state -- or a [N x 2] tensor / array.  device:
        where a host array given to fit_transform goes (default cuda).  method: 'exact' (dense P, N <= ops.tsne_max_points()) or 'neighbours' (P on
        the nearest neighbours only, repulsion still exact; N <= ops.tsne_nn_max_points(), perplexity <= 85)."""
        if method not in METHODS:
            raise ValueError("TSNE: method=%r; the choices are 'exact' and 'neighbours' (there is no tree: 'barnes_hut' is not "
                             "carried over)" % (method,))
        if method == 'neighbours' and int(3.0 * float(perplexity) + 1) > ops.tsne_nn_max_neighbours():
            raise ValueError("TSNE: perplexity %g needs %d neighbours; method='neighbours' takes at most %d (perplexity up to 85)"
                             % (perplexity, int(3.0 * float(perplexity) + 1), ops.tsne_nn_max_neighbours()))
        if n_components != 2:
            raise ValueError("TSNE: n_components=%r; the kernels embed in 2 dimensions only" % (n_components,))
        if not (torch.is_tensor(init) or isinstance(init, np.ndarray) or init in ('random', 'pca')):
            raise ValueError("TSNE: init must be 'random', 'pca' or a [N x 2] tensor")
        if learning_rate != 'auto' and not float(learning_rate) > 0:
            raise ValueError("TSNE: learning_rate must be 'auto' or positive")
        if int(n_iter) < 1 or not 0 <= int(exaggerated_iters):
            raise ValueError("TSNE: n_iter >= 1 and exaggerated_iters >= 0 expected")
        self.n_components, self.perplexity, self.early_exaggeration = 2, float(perplexity), float(early_exaggeration)
        self.learning_rate, self.n_iter, self.random_state, self.init = learning_rate, int(n_iter), random_state, init
        self.exaggerated_iters, self.device, self.method = int(exaggerated_iters), device, method
        self.embedding_ = self.kl_divergence_ = self.n_iter_ = self.learning_rate_ = None

    def _initial(self, N, device, X=None):
        if isinstance(self.init, str) and self.init == 'pca':
            if X is None or X.dim() != 2 or X.shape[1] < 2:
                raise ValueError("TSNE: init='pca' needs an input with at least 2 features")
            pca = PCA(n_components=2).fit(X)
            lambda_1 = float(pca._explained_variance_host[0])      # from the one read of fit
            if not lambda_1 > 0.0:
                raise ValueError("TSNE: init='pca' on an input without variance (all points equal)")
            # np.std of the first projected column: the population standard deviation, sqrt(lambda_1 (N - 1) / N)
            return ops.pca_project(X, pca.mean_, pca.components_, scale=_INIT_STD / np.sqrt(lambda_1 * (N - 1) / N))
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
        from_pca = isinstance(self.init, str) and self.init == 'pca'
        if from_pca and shape[1] < 2:
            raise ValueError("TSNE: init='pca' needs an input with at least 2 features, got %d" % shape[1])
        if self.perplexity >= N:
            raise ValueError("TSNE: perplexity %g must be less than the number of points %d" % (self.perplexity, N))
        if self.method == 'neighbours' and N > ops.tsne_nn_max_points():
            raise ValueError("TSNE: %d points; method='neighbours' takes at most %d" % (N, ops.tsne_nn_max_points()))
        if self.method == 'exact' and N > ops.tsne_max_points():
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
            # init='pca' can refuse its input (no variance): ahead of the affinity stage, which is the large allocation
            Y = self._initial(N, X.device, X) if from_pca else None
            if self.method == 'neighbours':
                csr = ops.tsne_nn_affinities(X, self.perplexity)[:3]

                def forces(Y, exaggeration, want_kl):
                    return ops.tsne_nn_forces(*csr, Y, exaggeration, want_kl)
            else:
                P, _ = ops.tsne_affinities(X, self.perplexity)

                def forces(Y, exaggeration, want_kl):
                    return ops.tsne_forces(P, Y, exaggeration, want_kl)
            if Y is None:
                Y = self._initial(N, X.device)
            velocity = torch.zeros_like(Y)
            gains = torch.ones_like(Y)
            for it in range(self.n_iter):
                early = it < self.exaggerated_iters
                part = forces(Y, self.early_exaggeration if early else 1.0, False)
                ops.tsne_update(part, Y, velocity, gains, 0.5 if early else 0.8, lr)
            stats = ops.tsne_stats(forces(Y, 1.0, True), True)
        self.kl_divergence_ = float(stats[1].item())
        self.n_iter_ = self.n_iter
        self.embedding_ = Y
        return Y

    def fit(self, X, y=None):
        self.fit_transform(X)
        return self


# ------------------------------------------------------------------------------------------------
# Quality of an embedding, independent of P (csrc/evae_nn_rank.hip): scikit-learn's trustworthiness and its mirror
# image, as exact integers from the device.  Neither an [N x N] matrix nor a sorted row exists at any point.
# ------------------------------------------------------------------------------------------------
def _pair(X, X_embedded, n_neighbors, who):
    """both spaces as float32 tensors on one device, converted as fit_transform converts its input; scikit-learn's bound on k"""
    device = next((t.device for t in (X, X_embedded) if torch.is_tensor(t)), 'cuda')
    out = []
    for a in (X, X_embedded):
        if not torch.is_tensor(a):
            a = torch.as_tensor(np.asarray(a, dtype=np.float32), device=device)
        if a.dim() != 2:
            raise ValueError("%s: [N x d] inputs expected, got %s" % (who, tuple(a.shape)))
        out.append(a)
    N, k = out[0].shape[0], int(n_neighbors)
    if out[1].shape[0] != N:
        raise ValueError("%s: %d points in X, %d in X_embedded" % (who, N, out[1].shape[0]))
    if k < 1 or k >= N / 2:
        raise ValueError("%s: n_neighbors (%d) should be at least 1 and less than n_samples / 2 (%g)" % (who, k, N / 2))
    return out[0], out[1], N, k


def _rank_sums(chosen_in, ranked_in, k):
    """the k nearest neighbours in one space, ranked in the other -> (nbr [N x k], the two integer totals of nn_rank's row sums)"""
    with torch.no_grad():
        nbr = ops.tsne_knn(chosen_in, k)[0]
        totals = ops.nn_rank(ranked_in, nbr)[1].sum(dim=0).tolist()       # read once: two Python integers
    return nbr, int(totals[0]), int(totals[1])


def _score(penalty, N, k):
    """scikit-learn's expression, in its order, in Python float64"""
    return 1.0 - penalty * (2.0 / (N * k * (2.0 * N - 3.0 * k - 1.0)))


def trustworthiness(X, X_embedded, n_neighbors=5):
    """sklearn.manifold.trustworthiness (Venna & Kaski) under squared Euclidean distance: 1 - 2 / (N k (2N - 3k - 1)) x the sum,
    over every point's k nearest neighbours in the embedding, of max(0, rank in X - k).  1 = no neighbour of the embedding is a
    stranger in the input space.  Ties are ordered by index, in both spaces."""
    X, Y, N, k = _pair(X, X_embedded, n_neighbors, "trustworthiness")
    return _score(_rank_sums(Y, X, k)[1], N, k)


def continuity(X, X_embedded, n_neighbors=5):
    """trustworthiness with the two spaces swapped: the input space's neighbours, ranked in the embedding.  1 = no neighbourhood
    of the input space is torn apart."""
    X, Y, N, k = _pair(X, X_embedded, n_neighbors, "continuity")
    return _score(_rank_sums(X, Y, k)[1], N, k)


def _label_accuracy(nbr, labels):
    """leave-one-out majority vote of every point's k neighbours' labels, ties to the lowest class: integer index plumbing"""
    labels = torch.as_tensor(np.asarray(labels) if not torch.is_tensor(labels) else labels).to(nbr.device).reshape(-1)
    if labels.numel() != nbr.shape[0]:
        raise ValueError("embedding_quality: %d labels for %d points" % (labels.numel(), nbr.shape[0]))
    classes, cls = torch.unique(labels, sorted=True, return_inverse=True)
    C = classes.numel()
    votes = torch.zeros((nbr.shape[0], C), dtype=torch.int64, device=nbr.device)
    votes.scatter_add_(1, cls[nbr.long()], torch.ones(nbr.shape, dtype=torch.int64, device=nbr.device))
    order = votes * C + (C - 1 - torch.arange(C, device=nbr.device))       # distinct within a row: most votes, then lowest class
    return int((order.argmax(dim=1) == cls).sum().item()) / nbr.shape[0]


def embedding_quality(X, X_embedded, n_neighbors=5, labels=None):
    """-> dict(trustworthiness, continuity, neighbourhood_preservation, n_neighbors, n_samples[, label_accuracy]).
    neighbourhood_preservation: the share of the k embedding-neighbours that are among the k input-neighbours too.
    label_accuracy (with labels [N]): the share of points whose label wins the vote of their k embedding-neighbours."""
    X, Y, N, k = _pair(X, X_embedded, n_neighbors, "embedding_quality")
    nbr, penalty, hits = _rank_sums(Y, X, k)
    out = dict(trustworthiness=_score(penalty, N, k), continuity=_score(_rank_sums(X, Y, k)[1], N, k),
               neighbourhood_preservation=hits / (N * k), n_neighbors=k, n_samples=N)
    if labels is not None:
        out['label_accuracy'] = _label_accuracy(nbr, labels)
    return out
