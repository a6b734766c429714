"""What the iterated drivers (evae/cluster.py's KMeans, evae/mixture.py's GaussianMixture, evae/linear.py's LogisticRegression) share: how an input becomes rows on
the device, the generator behind random_state, and the loop that issues steps blind and reads the device's record once per
batch.  Private to the package."""
import numpy as np
import torch


def _rows(X, device):
    """tensor or array -> contiguous float32 tensor on the device (an array or a host tensor goes to `device`, default cuda: the
    same data is taken the same way whichever of the three it comes as)"""
    if not torch.is_tensor(X):
        X = torch.as_tensor(np.ascontiguousarray(np.asarray(X, dtype=np.float32)), device=device or 'cuda')
    elif not X.is_cuda:
        X = X.to(device or 'cuda')
    if X.dtype != torch.float32:
        X = X.float()
    return X if X.is_contiguous() else X.contiguous()


def _shape(X):
    return tuple(X.shape) if torch.is_tensor(X) else np.shape(X)


def _int_at_least(who, name, v, low):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < low:
        raise ValueError("%s: %s=%r; an int >= %d expected" % (who, name, v, low))
    return int(v)


def _generator(random_state):
    """a CPU generator seeded with random_state; None draws a seed"""
    g = torch.Generator()
    if random_state is None:
        g.seed()
    else:
        g.manual_seed(int(random_state))
    return g


def _blind_batches(step, state, max_iter, check_every):
    """step() up to max_iter times in batches of check_every, the record `state` read once per batch -> the last record
    (numpy).  Every kernel of a step returns at once after the record's done flag (record[1]) is set, so the steps of a batch
    that come after it cost launches only."""
    issued, record = 0, None
    while issued < max_iter:
        batch = min(check_every, max_iter - issued)
        for _ in range(batch):
            step()
        issued += batch
        record = state.cpu().numpy()                                              # the one read of the batch
        if record[1] != 0.0:
            break
    return record
