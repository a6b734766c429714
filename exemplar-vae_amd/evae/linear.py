"""Linear probe of the latent space on the device in fp64 (csrc/evae_logreg.hip), behind scikit-learn's names:

    from evae.linear import LogisticRegression               # instead of sklearn.linear_model
    clf = LogisticRegression(C=1.0).fit(z_train, y_train)    # z [N x d] tensor or array, y [N] labels
    clf.score(z_test, y_test); clf.predict_proba(z_test)

What is computed is scikit-learn's objective for multinomial (softmax) regression with an L2 penalty and an unpenalised
intercept: with a_n = (x_n, 1) and lambda = 1 / C,

    f(W) = sum_n [ lse_k(a_n . w_k) - a_n . w_{y_n} ] + (lambda / 2) sum_k sum_{c<d} W_kc^2

minimised by L-BFGS from W = 0 (`history` pairs, scaling s.y / y.y of the newest pair, 1 / max|G| before any, a pair with
s.y <= 0 skipped) with an Armijo search (c1 = 1e-4) over the fixed grid t = 2^-j, j < line_steps: the device evaluates all the
trial losses in one launch and takes the first j that passes.  The fit stops when max|G| / N <= tol.  That is this
implementation's rule: n_iter_ is not scikit-learn's, whose L-BFGS has another line search and another stop.  Equal inputs give
bit-equal attributes.  The iterations run on the device: the host issues check_every of them blind -- every kernel returns at
once after the record's done flag is set -- and reads the 64-byte record once per batch.

Differences from scikit-learn: K = 2 is a two-row softmax, not the one-row sigmoid, so coef_ is [K x d] and intercept_ [K]
ALWAYS (scikit-learn's binary coef_ is coef_[1] - coef_[0] of this one, its decision_function the difference of the two
columns); probabilities and predictions are the same.  Not carried over: other penalties and solvers, class_weight,
sample_weight, warm_start, l1_ratio, multi_class (ValueError where scikit-learn takes an argument).  K <= 256, d <= 256,
N <= 2^20; a shape whose logits (twice [N x K] float64) plus workspace exceed 1 GiB is refused."""
import warnings

import numpy as np
import torch

from . import ops
from ._fit import _blind_batches, _int_at_least, _rows, _shape
from ._lib import EvaeError


class LogisticRegression:
    def __init__(self, C=1.0, tol=1e-4, max_iter=100, fit_intercept=True, history=10, line_steps=12, check_every=10, penalty='l2',
                 class_weight=None, warm_start=False, device=None):
        """C: inverse of the penalty's strength, finite and positive.  tol: the fit stops when max|G| / N <= tol.  max_iter:
        iterations (line searches) at most; reaching it warns.  history: pairs the L-BFGS recursion keeps.  line_steps: trial steps
        t = 2^-j, j < line_steps, of a search.  check_every: iterations issued between two reads of the device's record.  device:
        where a host array given to fit goes (default cuda).  penalty, class_weight, warm_start: only scikit-learn's defaults."""
        if penalty != 'l2':
            raise ValueError("LogisticRegression: penalty=%r is not carried over; 'l2' expected" % (penalty,))
        if class_weight is not None:
            raise ValueError("LogisticRegression: class_weight is not carried over")
        if warm_start:
            raise ValueError("LogisticRegression: warm_start is not carried over")
        if isinstance(C, bool) or not isinstance(C, (int, float, np.integer, np.floating)) or not np.isfinite(C) or not C > 0:
            raise ValueError("LogisticRegression: C=%r; a finite number > 0 expected" % (C,))
        if not float(tol) >= 0.0:
            raise ValueError("LogisticRegression: tol=%r; a number >= 0 expected" % (tol,))
        self.max_iter = _int_at_least("LogisticRegression", "max_iter", max_iter, 1)
        self.history = _int_at_least("LogisticRegression", "history", history, 1)
        self.line_steps = _int_at_least("LogisticRegression", "line_steps", line_steps, 1)
        self.check_every = _int_at_least("LogisticRegression", "check_every", check_every, 1)
        if self.history > ops.logreg_max_history():
            raise ValueError("LogisticRegression: history=%d above the cap of %d" % (self.history, ops.logreg_max_history()))
        if self.line_steps > ops.logreg_max_line_steps():
            raise ValueError("LogisticRegression: line_steps=%d above the cap of %d" % (self.line_steps, ops.logreg_max_line_steps()))
        self.C, self.tol, self.fit_intercept, self.device = float(C), float(tol), bool(fit_intercept), device
        self.classes_ = self.coef_ = self.intercept_ = self.line_steps_ = None
        self.n_iter_ = self.converged_ = self.loss_ = self.n_features_in_ = None
        self._W = None

    # ------------------------------------------------------------------------------------------------------------ the fit
    def _labels(self, y, N):
        """y -> (classes_ (sorted unique labels, numpy), int32 [N] in [0, K), still on the host)"""
        y = y.detach().cpu().numpy() if torch.is_tensor(y) else np.asarray(y)
        if y.ndim != 1 or y.shape[0] != N:
            raise ValueError("LogisticRegression: y of shape %s for %d rows" % (y.shape, N))
        classes, idx = np.unique(y, return_inverse=True)
        if classes.shape[0] < 2:
            raise ValueError("LogisticRegression: %d class(es) in y; at least 2 expected" % classes.shape[0])
        if classes.shape[0] > ops.logreg_max_classes():
            raise ValueError("LogisticRegression: %d classes above the cap of %d" % (classes.shape[0], ops.logreg_max_classes()))
        return classes, torch.as_tensor(idx.reshape(-1).astype(np.int32))

    def fit(self, X, y):
        """X [N x d], y [N] -> self.  classes_ (sorted unique labels); coef_ [K x d] and intercept_ [K] float64 on the device (K
        >= 2 rows always; zeros for the intercept when fit_intercept=False); n_iter_ (line searches done), converged_ (max|G| / N
        <= tol was reached), loss_ (f at the coefficients), line_steps_ (int32 [n_iter_]: the j of every search).  Reaching
        max_iter, a search none of whose steps passes, or a gradient that is not finite (entries of X that are not) sets
        converged_ = False and raises a RuntimeWarning that says which."""
        shape = _shape(X)
        if len(shape) != 2:
            raise ValueError("LogisticRegression: a [N x d] input expected, got %s" % (shape,))
        N, d = shape
        if not 1 <= N <= ops.logreg_max_points():
            raise ValueError("LogisticRegression: N=%d outside [1, %d]" % (N, ops.logreg_max_points()))
        if not 1 <= d <= ops.logreg_max_features():
            raise ValueError("LogisticRegression: %d features outside [1, %d]; reduce them with evae.pca" % (d, ops.logreg_max_features()))
        classes, yi = self._labels(y, N)
        K, fi, m, T = classes.shape[0], self.fit_intercept, self.history, self.line_steps
        try:
            ops.logreg_check_sizes(N, d, K, fi, m, T, "LogisticRegression")
        except EvaeError as e:
            raise ValueError(str(e))
        x = _rows(X, self.device)
        yi = yi.to(x.device)
        lam = 1.0 / self.C
        with torch.no_grad():
            f64 = dict(dtype=torch.float64, device=x.device)
            W = torch.zeros((K, d + (1 if fi else 0)), **f64)
            Z, ZD = torch.empty((N, K), **f64), torch.empty((N, K), **f64)
            solver = ops.logreg_solver(d, K, fi, m, x.device)
            state = ops.logreg_state(x.device)
            ws = ops.logreg_workspace(N, d, K, fi, T, x.device)
            ring = torch.full((self.max_iter,), -1, dtype=torch.int32, device=x.device)
            ops.logreg_begin(x, yi, W, Z, ZD, fi, solver, m, lam, self.tol, T, state, ws, labels_checked=True)
            record = _blind_batches(lambda: ops.logreg_step(x, yi, W, Z, ZD, fi, solver, m, lam, self.tol, T, state, ring, ws,
                                                            labels_checked=True), state, self.max_iter, self.check_every)
        self.classes_, self.n_features_in_ = classes, d
        self._W = W
        self.coef_ = W[:, :d]
        self.intercept_ = W[:, d] if fi else torch.zeros(K, **f64)
        self.n_iter_, self.converged_, self.loss_ = int(record[0]), bool(record[2] != 0.0), float(record[3])
        self.line_steps_ = ring[:self.n_iter_].clone()
        if record[6] != 0.0:
            warnings.warn("LogisticRegression: no step of the line search of iteration %d passed (line_steps=%d); the fit stopped "
                          "there" % (self.n_iter_, T), RuntimeWarning, stacklevel=2)
        elif not self.converged_ and not np.isfinite(float(ops.logreg_views(solver, d, K, fi, m)['scal'][2])):
            warnings.warn("LogisticRegression: the gradient is not finite after iteration %d (max|G| / N is not a number); are "
                          "all entries of X finite?  The fit stopped there" % self.n_iter_, RuntimeWarning, stacklevel=2)
        elif not self.converged_:
            warnings.warn("LogisticRegression: max_iter=%d reached before max|G| / N <= tol=%g; increase max_iter"
                          % (self.max_iter, self.tol), RuntimeWarning, stacklevel=2)
        return self

    # ------------------------------------------------------------------------------------------------------------ decisions
    def decision_function(self, X):
        """[N x d] -> float64 [N x K] on the device: x_n . w_k + b_k (K columns also for two classes)"""
        if self._W is None:
            raise EvaeError("LogisticRegression: fit first")
        shape = _shape(X)
        if len(shape) != 2 or shape[1] != self.n_features_in_:
            raise ValueError("LogisticRegression: a [N x %d] input expected, got %s" % (self.n_features_in_, shape))
        with torch.no_grad():
            return ops.logreg_logits(_rows(X, self.device), self._W, self.fit_intercept)

    def predict_log_proba(self, X):
        """[N x d] -> float64 [N x K] on the device: z_nk - lse(z_n)"""
        with torch.no_grad():
            return ops.logreg_softmax(self.decision_function(X))[0]

    def predict_proba(self, X):
        """[N x d] -> float64 [N x K] on the device: exp of predict_log_proba, divided by its own sum: a row adds up to 1
        within (K + 4) eps"""
        r = torch.exp(self.predict_log_proba(X))
        return r / r.sum(dim=1, keepdim=True)

    def predict_index(self, X):
        """[N x d] -> int32 [N] on the device: the index into classes_ of the largest decision value, the lowest on a tie"""
        with torch.no_grad():
            return ops.logreg_softmax(self.decision_function(X))[1]

    def predict(self, X):
        """[N x d] -> the labels (entries of classes_) as a numpy array [N]; ties go to the lowest class"""
        return self.classes_[self.predict_index(X).cpu().numpy()]

    def score(self, X, y):
        """mean accuracy of predict(X) against y, as a float"""
        y = y.detach().cpu().numpy() if torch.is_tensor(y) else np.asarray(y)
        return float((self.predict(X) == y).mean())
