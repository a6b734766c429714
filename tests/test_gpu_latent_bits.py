"""GPU: bit identity of the latent-analysis entry points (PCA moments, k-means, the strip-wise scores and neighbour search, the
Gaussian mixture) against tests/golden/latent_bits.json.

The kernels behind these entries share their building blocks (csrc/evae_latent.h) and promise one thing beyond accuracy: every
floating-point sum has a fixed order, so equal inputs give bit-equal outputs.  The other test files hold the accuracy; this one
holds IDENTITY only: the SHA-256 of every output tensor's bytes, at the smallest shapes at which each shared piece can take
another path (a second chunk of one row, idle lanes of a column group, one group only, a second tile of one centre, the first
width that asks for more LDS, a column loop that runs twice, a last strip of two rows).  Decisions inside these runs (an
arg-min, a stop) have no asserted margin here.

The JSON was recorded by record() below from the code as it stood BEFORE the shared header existed, and names the hipcc and
torch.version.hip it was recorded under.  It is never edited to make a test pass: on a mismatch an expression moved, and the
fix is to write it as it was.  Inputs come from numpy.random.default_rng(seed) here, so there is no input file."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "latent_bits.json")
GMM_TYPES = ('full', 'diag', 'spherical')


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def blobs(rng, N, d, K):
    """N float32 rows around K centres, every centre owning rows, each row times its own power of two from 2^-16 .. 2^16: a
    column's values span 32 binades, so its fp64 sum ROUNDS and its bits depend on the order of the additions (unscaled rows
    of O(1) add exactly in fp64, in any order).  -> (x, the int32 label of every row)"""
    labels = rng.permutation(np.arange(N) % K).astype(np.int32)
    centres = 3.0 * rng.standard_normal((K, d))
    x = (centres[labels] + rng.standard_normal((N, d))) * np.exp2(rng.integers(-16, 17, (N, 1)))
    return x.astype(np.float32), labels


def overlapping(rng, N, d, K):
    """N float32 rows of K components that OVERLAP (centres 2.5 / sqrt(d) apart per feature, unit noise, rows scaled by
    2^-2 .. 2^2) and starting labels that ignore the components: the first responsibilities are fractional and every one of the
    EM steps below moves the parameters (well separated blobs give responsibilities of exactly 0 and 1 and a fixed point).
    -> (x, the int32 starting label of every row)"""
    true = rng.integers(0, K, N)
    centres = 2.5 * rng.standard_normal((K, d)) / np.sqrt(d)
    x = (centres[true] + rng.standard_normal((N, d))) * np.exp2(rng.integers(-2, 3, (N, 1)))
    return x.astype(np.float32), rng.permutation(np.arange(N) % K).astype(np.int32)


# reg_covar of the mixture cases: large enough that 100 rows per component in 96 features do not fit their own rows to
# responsibilities of exactly 0 and 1 (at 1e-3 they do, and the steps stop moving)
GMM_REG = 0.5


# ---------------------------------------------------------------- the cases: name -> {output name: tensor}
def pca_case(N, d):
    def run():
        from evae import ops
        rng = np.random.default_rng(1000 + N + d)
        x = rng.standard_normal((N, d)) * rng.uniform(0.5, 2.0, d) + rng.standard_normal(d)
        x = dev((x * np.exp2(rng.integers(-16, 17, (N, 1)))).astype(np.float32))     # the fp64 column sums round (see blobs)
        mean, cov = ops.pca_moments(x)
        return dict(mean=mean, cov=cov)
    return run


def kmeans_run(x, labels0, init):
    """assign, update, seed and three steps from `init`; every output of every call"""
    from evae import ops
    N, d = x.shape
    K = init.shape[0]
    out = {}
    x, centres = dev(x), dev(init)
    out["assign.labels"], out["assign.d2"] = ops.kmeans_assign(x, centres)
    out["update.order"], out["update.start"], out["update.sums"] = ops.kmeans_update(x, dev(labels0), K)
    u = dev(np.random.default_rng(7).random(K))
    out["seed.idx"], out["seed.centres"] = ops.kmeans_seed(x, K, u)
    labels = torch.empty(N, dtype=torch.int32, device='cuda')
    d2 = torch.empty(N, dtype=torch.float64, device='cuda')
    order = torch.empty(N, dtype=torch.int32, device='cuda')
    start = torch.empty(K + 1, dtype=torch.int32, device='cuda')
    state, ws = ops.kmeans_state('cuda'), ops.kmeans_workspace(N, d, K, 'cuda')
    for step in (1, 2, 3):
        ops.kmeans_step(x, centres, labels, d2, order, start, 0.0, state, ws)
        for name, t in (("centres", centres), ("labels", labels), ("d2", d2), ("order", order), ("start", start), ("state", state)):
            out["step%d.%s" % (step, name)] = t.clone()
    return out


def kmeans_case(N, d, K):
    def run():
        rng = np.random.default_rng(2000 + N + d + K)
        x, labels = blobs(rng, N, d, K)
        return kmeans_run(x, labels, x[:K].astype(np.float64))
    return run


def kmeans_empty_case():
    """two of the four given centres lie far from every row: both clusters start empty and are relocated in the first step"""
    rng = np.random.default_rng(2999)
    x, labels = blobs(rng, 600, 8, 4)
    init = x[:4].astype(np.float64)
    init[2:] += 1.0e9                                        # the rows reach 2^16 x O(10)
    return kmeans_run(x, labels, init)


def inertia_case(N):
    def run():
        from evae import ops
        return dict(inertia=ops.kmeans_inertia(dev(np.random.default_rng(3000 + N).random(N) * 10.0)))
    return run


def strip_case(strip_rows):
    def run():
        from evae import ops
        N, d, K, k = 130, 7, 3, 5
        x, labels = blobs(np.random.default_rng(4000), N, d, K)
        x = dev(x)
        order, start, _ = ops.kmeans_update(x, dev(labels), K)
        idx, d2 = ops.tsne_knn(x, k, strip_rows)
        rank, row_sums = ops.nn_rank(x, idx, strip_rows)
        return {"silhouette": ops.silhouette_samples(x, order, start, strip_rows), "knn.idx": idx, "knn.d2": d2,
                "rank": rank, "rank.row_sums": row_sums}
    return run


def gmm_case(N, d, K, ctype):
    def run():
        from evae import ops
        rng = np.random.default_rng(5000 + N + d + K)
        x, labels = overlapping(rng, N, d, K)
        x, labels = dev(x), dev(labels)
        out = {}
        params = ops.gmm_params(d, K, ctype, 'cuda')
        params.zero_()
        state, ws = ops.gmm_state('cuda'), ops.gmm_workspace(N, d, K, ctype, 'cuda')
        ops.gmm_mstep(x, params, K, ctype, GMM_REG, state, labels=labels, ws=ws)
        out["mstep.params"], out["mstep.state"] = params.clone(), state.clone()
        log_resp, logp, mean_logp = ops.gmm_estep(x, params, K, ctype, ws=ws)
        out["estep.log_resp"], out["estep.logp"], out["estep.mean_logp"] = log_resp.clone(), logp.clone(), mean_logp
        state = ops.gmm_state('cuda')
        for step in (1, 2, 3):
            ops.gmm_step(x, params, K, ctype, log_resp, logp, GMM_REG, 0.0, state, ws)
            for name, t in (("params", params), ("log_resp", log_resp), ("logp", logp), ("state", state)):
                out["step%d.%s" % (step, name)] = t.clone()
        return out
    return run


CASES = {}
for _N, _d in ((1025, 1), (2049, 17), (3, 256)):
    CASES["pca_moments-%d-%d" % (_N, _d)] = pca_case(_N, _d)
for _N, _d, _K in ((65, 1, 1), (513, 40, 33), (1100, 65, 10)):
    CASES["kmeans-%d-%d-%d" % (_N, _d, _K)] = kmeans_case(_N, _d, _K)
CASES["kmeans-empty-600-8-4"] = kmeans_empty_case
for _N in (1, 512, 513):
    CASES["kmeans_inertia-%d" % _N] = inertia_case(_N)
STRIP_ROWS = (64, 0)
for _s in STRIP_ROWS:
    CASES["strips-130-7-3-5-rows%d" % _s] = strip_case(_s)
for _t in GMM_TYPES:
    for _N, _d, _K in ((65, 1, 1), (513, 17, 5)):
        CASES["gmm-%s-%d-%d-%d" % (_t, _N, _d, _K)] = gmm_case(_N, _d, _K, _t)
CASES["gmm-full-200-96-2"] = gmm_case(200, 96, 2, 'full')
CASES["gmm-diag-600-256-3"] = gmm_case(600, 256, 3, 'diag')


def hashes(name):
    return {k: sha(t) for k, t in CASES[name]().items()}


# ---------------------------------------------------------------- the tests
@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_case_is_recorded(recorded):
    assert sorted(recorded["cases"]) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_bits(name, recorded):
    want, got = recorded["cases"][name], hashes(name)
    assert sorted(got) == sorted(want), "%s: outputs %s, recorded %s" % (name, sorted(got), sorted(want))
    moved = [k for k in sorted(got) if got[k] != want[k]]
    print("%s: %d outputs, %d differ" % (name, len(got), len(moved)))
    assert not moved, "%s: the bits of %s differ from the recording (made under %s)" % (name, moved, recorded["recorded_under"])


def test_strip_settings_agree():
    """the strip-wise entries do not depend on strip_rows: three strips (the last of two rows) against the automatic one strip"""
    a, b = (hashes("strips-130-7-3-5-rows%d" % s) for s in STRIP_ROWS)
    moved = [k for k in sorted(a) if a[k] != b[k]]
    assert not moved, "strip_rows %d and %d disagree in %s" % (STRIP_ROWS + (moved,))


# ---------------------------------------------------------------- recording
def record(path=GOLDEN):
    """Writes the JSON from the code beside this file.  Run it on the tree whose bits are to be held, never to mend a failure."""
    import subprocess
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "exemplar-vae_amd"))
    hipcc = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--version"], stdout=subprocess.PIPE,
                           universal_newlines=True, check=True).stdout.strip().splitlines()
    doc = {"recorded_under": {"hipcc": " | ".join(l.strip() for l in hipcc[:2]), "torch.version.hip": torch.version.hip},
           "cases": {name: hashes(name) for name in sorted(CASES)}}
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d cases to %s" % (len(doc["cases"]), path))


if __name__ == "__main__":
    record(*sys.argv[1:2])
