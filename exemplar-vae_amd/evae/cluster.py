"""k-means of the latent space on the device in fp64, and the scores of a clustering (csrc/evae_kmeans.hip), behind
scikit-learn's names:

    from evae.cluster import KMeans, clustering_quality     # instead of sklearn.cluster / sklearn.metrics
    km = KMeans(n_clusters=10, random_state=0).fit(z)        # z [N x d] tensor or array; labels_ int32 on the device
    clustering_quality(z, km.labels_, labels_true=y)         # nmi, ari, purity, silhouette

What is computed is scikit-learn's KMeans(algorithm='lloyd') without sample weights: the assignment by direct differences in
fp64, cluster means from fixed-order fp64 sums, its rule for empty clusters (the points of largest distance, one each, subtracted
from their donors), its two stopping rules (no label changed; sum |c_new - c_old|^2 <= tol x the mean variance of the features)
and k-means++ seeding by D^2 sampling.  Equal inputs and equal random_state give bit-equal centres and labels.  The iterations
run on the device: the host issues check_every of them blind -- every kernel returns at once after the record's done flag is set
-- and reads the 64-byte record once per batch.

Not carried over: algorithm='elkan', the greedy local trials of scikit-learn's k-means++ (one candidate per centre here, so the
seeds differ from scikit-learn's for the same random_state), sample_weight, MiniBatchKMeans.  K <= ops.kmeans_max_clusters() =
1024, d <= ops.kmeans_max_features() = 256, N <= ops.kmeans_max_points() = 2^20; the silhouette takes N <=
ops.tsne_nn_max_points() and works in strips, so no [N x N] buffer exists."""
import numpy as np
import torch

from . import ops
from ._fit import _blind_batches, _generator, _int_at_least, _rows, _shape
from ._lib import EvaeError


class KMeans:
    def __init__(self, n_clusters=8, init='k-means++', n_init='auto', max_iter=300, tol=1e-4, random_state=None, check_every=8,
                 device=None):
        """init: 'k-means++' (D^2 sampling, ops.kmeans_seed), 'random' (K distinct rows) or a [K x d] tensor / array.
        n_init: runs from different seeds, the one of lowest inertia wins (ties: the first); 'auto' = 1 / 10 / 1 for those three.
        tol: relative to the mean population variance of the features, as scikit-learn's.  random_state seeds a CPU
        torch.Generator all uniforms (float64) and row choices come from; None draws a seed.  check_every: iterations issued
        between two reads of the device's record.  device: where a host array given to fit goes (default cuda)."""
        n_clusters = _int_at_least("KMeans", "n_clusters", n_clusters, 1)
        if isinstance(init, str):
            if init not in ('k-means++', 'random'):
                raise ValueError("KMeans: init=%r; 'k-means++', 'random' or a [K x d] tensor expected" % (init,))
        elif not (torch.is_tensor(init) or isinstance(init, np.ndarray)):
            raise ValueError("KMeans: init=%r; 'k-means++', 'random' or a [K x d] tensor expected" % (init,))
        elif len(_shape(init)) != 2 or _shape(init)[0] != n_clusters:
            raise ValueError("KMeans: init of shape %s for n_clusters=%d" % (_shape(init), n_clusters))
        if not (n_init == 'auto' or (not isinstance(n_init, (bool, str)) and isinstance(n_init, (int, np.integer)) and n_init >= 1)):
            raise ValueError("KMeans: n_init=%r; 'auto' or an int >= 1 expected" % (n_init,))
        max_iter = _int_at_least("KMeans", "max_iter", max_iter, 1)
        check_every = _int_at_least("KMeans", "check_every", check_every, 1)
        if not float(tol) >= 0.0:
            raise ValueError("KMeans: tol=%r; a number >= 0 expected" % (tol,))
        self.n_clusters, self.init, self.n_init, self.max_iter, self.tol = n_clusters, init, n_init, max_iter, float(tol)
        self.random_state, self.check_every, self.device = random_state, check_every, device
        self.cluster_centers_ = self.labels_ = self.inertia_ = self.n_iter_ = self.n_relocations_ = None
        self.n_features_in_ = None

    def _check(self, shape):
        """what is known from the shape: refused before any launch"""
        if len(shape) != 2:
            raise ValueError("KMeans: a [N x d] input expected, got %s" % (shape,))
        N, d = shape
        if N < 2:
            raise ValueError("KMeans: N=%d; at least 2 points expected" % N)
        if N > ops.kmeans_max_points():
            raise ValueError("KMeans: N=%d above the cap of %d points" % (N, ops.kmeans_max_points()))
        if not 1 <= d <= ops.kmeans_max_features():
            raise ValueError("KMeans: %d features outside [1, %d]" % (d, ops.kmeans_max_features()))
        if self.n_clusters > min(N, ops.kmeans_max_clusters()):
            raise ValueError("KMeans: n_clusters=%d outside [1, min(N=%d, %d)]" % (self.n_clusters, N, ops.kmeans_max_clusters()))
        if not isinstance(self.init, str) and _shape(self.init) != (self.n_clusters, d):
            raise ValueError("KMeans: init of shape %s, [%d x %d] expected" % (_shape(self.init), self.n_clusters, d))

    def _runs(self):
        if self.n_init != 'auto':
            return int(self.n_init) if isinstance(self.init, str) else 1          # a given init has one run to make
        return 10 if isinstance(self.init, str) and self.init == 'random' else 1

    def _seeds(self, x, g, ws):
        """the initial centres of one run, float64 [K x d] on the device (a fresh tensor: the run overwrites it)"""
        K = self.n_clusters
        if not isinstance(self.init, str):
            c = self.init if torch.is_tensor(self.init) else torch.as_tensor(np.asarray(self.init, dtype=np.float64))
            return c.to(device=x.device, dtype=torch.float64).contiguous().clone()
        if self.init == 'random':
            idx = torch.randperm(x.shape[0], generator=g)[:K].to(x.device)        # K distinct rows: index plumbing
            return x[idx].double().contiguous()
        u = torch.rand(K, dtype=torch.float64, generator=g).to(x.device)
        return ops.kmeans_seed(x, K, u, ws)[1]

    def _lloyd(self, x, centres, tol_abs, ws):
        """centres in place -> (n_iter, relocations): batches of check_every blind steps, one read of the record per batch"""
        N, K = x.shape[0], self.n_clusters
        labels = torch.empty(N, dtype=torch.int32, device=x.device)
        d2 = torch.empty(N, dtype=torch.float64, device=x.device)
        order = torch.empty(N, dtype=torch.int32, device=x.device)
        start = torch.empty(K + 1, dtype=torch.int32, device=x.device)
        state = ops.kmeans_state(x.device)
        record = _blind_batches(lambda: ops.kmeans_step(x, centres, labels, d2, order, start, tol_abs, state, ws), state,
                                self.max_iter, self.check_every)
        return int(record[0]), int(record[5])

    def fit(self, X, y=None):
        """X [N x d] -> self.  cluster_centers_ float64 [K x d] and labels_ int32 [N] on the device; inertia_ (float), n_iter_,
        n_relocations_ (points moved into empty clusters over the winning run).  labels_ and inertia_ belong to
        cluster_centers_: one closing assignment.  Reaching max_iter is not an error."""
        self._check(_shape(X))
        x = _rows(X, self.device)
        N, d = x.shape
        with torch.no_grad():
            tol_abs = 0.0
            if self.tol > 0.0:
                cov = ops.pca_moments(x)[1]
                tol_abs = self.tol * float((torch.diagonal(cov) * ((N - 1.0) / N)).mean().item())
            ws = ops.kmeans_workspace(N, d, self.n_clusters, x.device)
            g = _generator(self.random_state)
            best = None
            for _ in range(self._runs()):
                centres = self._seeds(x, g, ws)
                n_iter, relocations = self._lloyd(x, centres, tol_abs, ws)
                labels, d2 = ops.kmeans_assign(x, centres)
                inertia = float(ops.kmeans_inertia(d2).item())
                if best is None or inertia < best[0]:
                    best = (inertia, centres, labels, n_iter, relocations)
        self.inertia_, self.cluster_centers_, self.labels_, self.n_iter_, self.n_relocations_ = best
        self.n_features_in_ = d
        return self

    def _fitted(self):
        if self.cluster_centers_ is None:
            raise EvaeError("KMeans: fit first")

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_

    def predict(self, X):
        """[N x d] -> int32 [N] on the device: the nearest of cluster_centers_"""
        self._fitted()
        with torch.no_grad():
            return ops.kmeans_assign(_rows(X, self.device), self.cluster_centers_)[0]

    def transform(self, X):
        """[N x d] -> float32 [N x K] on the device: the distances to cluster_centers_"""
        self._fitted()
        with torch.no_grad():
            return ops.kmeans_transform(_rows(X, self.device), self.cluster_centers_)

    def fit_transform(self, X, y=None):
        return self.fit(X).transform(X)


# ---------------------------------------------------------------------------------------------------------------- scores
def _codes(labels, device):
    """arbitrary integer labels -> (int32 codes 0 .. K - 1 in the order of the sorted distinct labels, K): index plumbing"""
    t = labels if torch.is_tensor(labels) else torch.as_tensor(np.asarray(labels))
    if t.dim() != 1 or t.is_floating_point() or t.is_complex():
        raise ValueError("cluster scores: a 1-d vector of integer labels expected, got %s %s" % (t.dtype, tuple(t.shape)))
    t = t.to(device)
    classes, inverse = torch.unique(t, sorted=True, return_inverse=True)
    return inverse.to(torch.int32).contiguous(), int(classes.numel())


def _device_of(*xs):
    for x in xs:
        if torch.is_tensor(x) and x.is_cuda:
            return x.device
    return torch.device('cuda')


def contingency_matrix(labels_true, labels_pred):
    """-> int64 [classes x clusters] on the device, rows and columns in the order of the sorted distinct labels"""
    dev = _device_of(labels_true, labels_pred)
    a, Ka = _codes(labels_true, dev)
    b, Kb = _codes(labels_pred, dev)
    if a.numel() != b.numel():
        raise ValueError("cluster scores: %d true labels for %d predicted ones" % (a.numel(), b.numel()))
    with torch.no_grad():
        return ops.cluster_contingency(a, Ka, b, Kb)


def _scores(labels_true, labels_pred):
    with torch.no_grad():
        out = ops.cluster_scores(contingency_matrix(labels_true, labels_pred)).cpu().numpy()      # the one read
    return dict(zip(ops.CLUSTER_SCORES, (float(v) for v in out)))


def normalized_mutual_info_score(labels_true, labels_pred):
    """arithmetic-mean normalisation, scikit-learn's default; 1 for one class and one cluster"""
    return _scores(labels_true, labels_pred)["nmi"]


def adjusted_rand_score(labels_true, labels_pred):
    return _scores(labels_true, labels_pred)["ari"]


def purity_score(labels_true, labels_pred):
    """every predicted cluster counted for its most frequent class: sum_j max_i n_ij / N"""
    return _scores(labels_true, labels_pred)["purity"]


def _sorted_by_label(X, labels, who):
    x = _rows(X, None)
    if x.dim() != 2:
        raise ValueError("%s: a [N x d] input expected, got %s" % (who, tuple(x.shape)))
    codes, K = _codes(labels, x.device)
    if codes.numel() != x.shape[0]:
        raise ValueError("%s: %d labels for %d points" % (who, codes.numel(), x.shape[0]))
    if not 2 <= K <= x.shape[0] - 1:
        raise ValueError("%s: %d distinct labels; between 2 and N - 1 = %d expected" % (who, K, x.shape[0] - 1))
    order, start, _ = ops.kmeans_update(x, codes, K)
    return x, order, start


def silhouette_samples(X, labels, strip_rows=0):
    """-> float64 [N] on the device: (b - a) / max(a, b) per sample with Euclidean distances, 0 for the only member of a
    cluster.  ValueError unless 2 <= distinct labels <= N - 1 (scikit-learn's rule)."""
    with torch.no_grad():
        x, order, start = _sorted_by_label(X, labels, "silhouette_samples")
        return ops.silhouette_samples(x, order, start, strip_rows)


def silhouette_score(X, labels, strip_rows=0):
    """the mean of silhouette_samples (a fixed-order fp64 sum on the device), as a float"""
    with torch.no_grad():
        s = silhouette_samples(X, labels, strip_rows)
        return float(ops.kmeans_inertia(s).item()) / s.numel()


def clustering_quality(X, labels_pred, labels_true=None, silhouette=True):
    """-> dict(n_samples, n_clusters[, nmi, ari, purity, n_classes][, silhouette]): the scores against labels_true when they are
    given, the silhouette of labels_pred in X unless switched off (it is the one part that costs N^2 distances)."""
    dev = _device_of(X, labels_pred)
    codes, K = _codes(labels_pred, dev)
    out = {"n_samples": int(codes.numel()), "n_clusters": K}
    if labels_true is not None:
        s = _scores(labels_true, labels_pred)
        out.update(nmi=s["nmi"], ari=s["ari"], purity=s["purity"], n_classes=_codes(labels_true, dev)[1])
    if silhouette:
        out["silhouette"] = silhouette_score(X, labels_pred)
    return out
