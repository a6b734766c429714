// PCA of the latent space on gfx950, all arithmetic in fp64 (evae/pca.py, TSNE(init='pca'); DESIGN 3.7c has the formulas, the
// termination argument and the measurements).  No floating-point atomics; every sum has a fixed order.
//
//   moments:  pass 1, one block per chunk of kChunkRows rows: column sums -> ws; one block adds the chunks in index order -> mean.
//             pass 2, one block per (chunk, 16 x 16 tile with tile row <= tile column): the rows, centred in fp64, go through LDS
//             64 at a time and every thread owns one (i, j) of the tile -> ws; the finish launch adds the chunks in index order,
//             divides by N - 1 and writes cov[i][j] and cov[j][i] from the one value.
//   eigh:     ONE workgroup, one-sided (Hestenes) cyclic Jacobi: G = cov, V = I, both stored by columns; a wave takes a pair
//             (p, q) of the round-robin round, reduces |g_p|^2, |g_q|^2 and g_p . g_q over its lanes and rotates the two columns
//             of G and of V.  The m / 2 pairs of a round are disjoint, a barrier separates rounds.  A sweep in which no pair was
//             above 2^-52 |g_p| |g_q| ends the loop; the loop's bound is the compile-time kMaxSweeps.  Then, in the same launch:
//             Rayleigh quotients against the caller's cov, a counting rank per column, the sign rule, the rows of evecs.
//             G and V sit in LDS for d <= kLdsMaxD and in the caller's workspace above; the code is the same (a template flag
//             picks the pointer).
//   project / reconstruct: 16 rows per block, staged in LDS as doubles; a thread owns (row, output column) items.
#include "evae_latent.h"

namespace evae {

constexpr int kPcaMaxD = 256;
constexpr int kPcaMaxN = 1 << 20;
constexpr int kChunkRows = 1024;
// One-sided Jacobi on G = cov works in the metric of cov^2, so a wide spectrum costs sweeps: 5 .. 27 on the matrices of
// tests/test_gpu_pca.py (27: d = 256, condition 2.5e5; 15: d = 24, condition 1e12).
constexpr int kMaxSweeps = 64;
constexpr int kLdsMaxD = 96;                 // 2 * 96^2 * 8 B = 144 KiB of the workgroup's 160 KiB
constexpr int kPcaThreads = 256;
constexpr int kTile = 16;                    // kTile^2 == kPcaThreads
constexpr int kStageRows = 64;
constexpr int kRowsPerBlock = 16;
constexpr int kEighMaxWaves = 16;
constexpr int kPerLane = kPcaMaxD / 64;      // entries of a column per lane of the wave that owns it
constexpr double kEps = 2.220446049250313e-16;   // 2^-52

// ---------------------------------------------------------------- moments
// sums [chunks x d]: thread (g, c) adds rows g, g + G, .. of its chunk in column c; the G partial sums are added in order of g.
__global__ __launch_bounds__(kPcaThreads) void pca_colsum_kernel(const float* __restrict__ x, int N, int d, int W,
                                                                 double* __restrict__ sums) {
  __shared__ double part[kPcaThreads];
  const int tid = threadIdx.x, c = tid & (W - 1), g = tid / W, G = kPcaThreads / W;
  const int r0 = blockIdx.x * kChunkRows, r1 = min(N, r0 + kChunkRows);
  double s = 0.0;
  if (c < d)
    for (int r = r0 + g; r < r1; r += G) s += (double)x[(size_t)r * d + c];
  const bool owner = g == 0 && c < d;
  const double t = group_fold(s, part, c, W, G, owner);
  if (owner) sums[(size_t)blockIdx.x * d + c] = t;
}

__global__ __launch_bounds__(kPcaThreads) void pca_mean_kernel(const double* __restrict__ sums, int chunks, int N, int d,
                                                               double* __restrict__ mean) {
  const int c = threadIdx.x;
  if (c >= d) return;
  double t = 0.0;
  for (int ch = 0; ch < chunks; ++ch) t += sums[(size_t)ch * d + c];
  mean[c] = t / (double)N;
}

// gram [chunks x d x d]: only the entries of the tiles with tile row <= tile column are written
__global__ __launch_bounds__(kPcaThreads) void pca_gram_kernel(const float* __restrict__ x, int N, int d,
                                                               const double* __restrict__ mean, double* __restrict__ gram) {
  __shared__ double A[kStageRows * kTile];
  __shared__ double B[kStageRows * kTile];
  const int tid = threadIdx.x, ty = tid / kTile, tx = tid % kTile;
  int ti = 0, rest = blockIdx.x;                       // blockIdx.x counts the tiles (ti, tj), ti <= tj, row by row
  const int T = (d + kTile - 1) / kTile;
  while (rest >= T - ti) {
    rest -= T - ti;
    ++ti;
  }
  const int tj = ti + rest;
  const int r0 = blockIdx.y * kChunkRows, r1 = min(N, r0 + kChunkRows);
  double acc = 0.0;
  for (int s0 = r0; s0 < r1; s0 += kStageRows) {
    for (int e = tid; e < kStageRows * kTile; e += kPcaThreads) {
      const int r = s0 + e / kTile, cc = e % kTile;
      const int ca = ti * kTile + cc, cb = tj * kTile + cc;
      A[e] = (r < r1 && ca < d) ? (double)x[(size_t)r * d + ca] - mean[ca] : 0.0;
      B[e] = (r < r1 && cb < d) ? (double)x[(size_t)r * d + cb] - mean[cb] : 0.0;
    }
    __syncthreads();
#pragma unroll 8
    for (int r = 0; r < kStageRows; ++r) acc = fma(A[r * kTile + ty], B[r * kTile + tx], acc);
    __syncthreads();
  }
  const int i = ti * kTile + ty, j = tj * kTile + tx;
  if (i < d && j < d) gram[((size_t)blockIdx.y * d + i) * d + j] = acc;
}

__global__ __launch_bounds__(kPcaThreads) void pca_cov_finish_kernel(const double* __restrict__ gram, int chunks, int N, int d,
                                                                     double* __restrict__ cov) {
  const int idx = blockIdx.x * kPcaThreads + threadIdx.x;
  if (idx >= d * d) return;
  const int i = idx / d, j = idx % d;
  if (i > j) return;
  double t = 0.0;
  for (int ch = 0; ch < chunks; ++ch) t += gram[((size_t)ch * d + i) * d + j];
  t /= (double)(N - 1);
  cov[(size_t)i * d + j] = t;
  cov[(size_t)j * d + i] = t;
}

// ---------------------------------------------------------------- eigen-solver
// pair `i` of round `r` among m players (m even): player m - 1 stays, the others move round the circle
__device__ __forceinline__ void round_robin_pair(int m, int r, int i, int& p, int& q) {
  const int n = m - 1;
  int a = i == 0 ? n : (r + i) % n;
  int b = (r + n - i) % n;
  p = min(a, b);
  q = max(a, b);
}

template <bool kLds>
__global__ __launch_bounds__(64 * kEighMaxWaves) void pca_eigh_kernel(const double* cov, int d, double* evals, double* evecs,
                                                                      double* info, double* ws) {
  extern __shared__ __attribute__((aligned(16))) double pca_smem[];
  __shared__ int rotated[kMaxSweeps];
  __shared__ double wave_off[kEighMaxWaves];
  __shared__ double lam[kPcaMaxD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x, nw = nthreads >> 6;
  double* G = kLds ? pca_smem : ws;                    // column c: G[c * d .. c * d + d)
  double* V = G + d * d;

  for (int e = tid; e < d * d; e += nthreads) {
    G[e] = cov[e];                                     // symmetric: by columns == by rows
    V[e] = (e / d == e % d) ? 1.0 : 0.0;
  }
  for (int e = tid; e < kMaxSweeps; e += nthreads) rotated[e] = 0;
  __syncthreads();

  const int m = d + (d & 1), pairs = m / 2;
  int sweeps = 0, converged = 0;
  double off = 0.0;
  for (int sweep = 0; sweep < kMaxSweeps; ++sweep) {
    double wmax = 0.0;
    int nrot = 0;
    for (int r = 0; r < m - 1; ++r) {
      for (int pi = wave; pi < pairs; pi += nw) {
        int p, q;
        round_robin_pair(m, r, pi, p, q);
        if (q >= d) continue;                          // the bye of an odd d
        double* gp = G + p * d;
        double* gq = G + q * d;
        double a[kPerLane], b[kPerLane];                // the two columns stay in registers from the sums to the rotation
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
        for (int u = 0; u < kPerLane; ++u) {
          const int k = lane + 64 * u;
          a[u] = k < d ? gp[k] : 0.0;
          b[u] = k < d ? gq[k] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < kPerLane; ++u) {
          alpha = fma(a[u], a[u], alpha);
          beta = fma(b[u], b[u], beta);
          gamma = fma(a[u], b[u], gamma);
        }
        alpha = wave_sum(alpha);
        beta = wave_sum(beta);
        gamma = wave_sum(gamma);
        const double scale = sqrt(alpha) * sqrt(beta);
        const double ag = fabs(gamma);
        if (scale > 0.0) wmax = fmax(wmax, ag / scale);
        if (ag <= kEps * scale) continue;              // wave-uniform: the three sums are the same in every lane
        ++nrot;
        // The pair is counted even if the rotation below comes out as the identity (zeta overflowing to inf, or t below the
        // rounding of c): that needs column norms next to the denormal range, such a matrix never reports convergence, and
        // it ends safely at the sweep bound with info[1] = 0.
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double az = fabs(zeta);
        double t = az > 1e150 ? 0.5 / az : 1.0 / (az + sqrt(1.0 + az * az));
        if (zeta < 0.0) t = -t;
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
        double* vp = V + p * d;
        double* vq = V + q * d;
#pragma unroll
        for (int u = 0; u < kPerLane; ++u) {
          const int k = lane + 64 * u;
          if (k < d) {
            gp[k] = c * a[u] - s * b[u];
            gq[k] = s * a[u] + c * b[u];
            const double va = vp[k], vb = vq[k];
            vp[k] = c * va - s * vb;
            vq[k] = s * va + c * vb;
          }
        }
      }
      __syncthreads();
    }
    if (lane == 0) {
      wave_off[wave] = wmax;
      if (nrot) atomicAdd(&rotated[sweep], nrot);      // an integer count: its order does not matter
    }
    __syncthreads();
    off = 0.0;
    for (int w = 0; w < nw; ++w) off = fmax(off, wave_off[w]);
    const int total = rotated[sweep];                  // the same value in every thread of the workgroup
    sweeps = sweep + 1;
    __syncthreads();                                   // wave_off is written again in the next sweep
    if (total == 0) {
      converged = 1;
      break;
    }
  }

  // Rayleigh quotients against the caller's matrix, clamped at 0
  for (int j = wave; j < d; j += nw) {
    const double* v = V + j * d;
    double acc = 0.0;
    for (int i = lane; i < d; i += 64) {
      double w = 0.0;
      for (int k = 0; k < d; ++k) w = fma(cov[(size_t)k * d + i], v[k], w);
      acc = fma(v[i], w, acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) lam[j] = acc > 0.0 ? acc : 0.0;     // (a NaN goes to 0 too)
  }
  __syncthreads();

  // place of column j in the descending order (ties by index), the sign rule, row `place` of evecs
  for (int j = wave; j < d; j += nw) {
    const double lj = lam[j];
    int before = 0;
    for (int k = lane; k < d; k += 64) before += (lam[k] > lj) || (lam[k] == lj && k < j);
    const int place = wave_sum(before);
    const double* v = V + j * d;
    double best = -1.0;
    int where = kNoIndex;
    for (int i = lane; i < d; i += 64) {
      const double a = fabs(v[i]);
      if (a > best) {
        best = a;
        where = i;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ob = __shfl_xor(best, o, 64);
      const int ow = __shfl_xor(where, o, 64);
      if (ob > best || (ob == best && ow < where)) {
        best = ob;
        where = ow;
      }
    }
    const double sign = (where < d && v[where] < 0.0) ? -1.0 : 1.0;
    for (int i = lane; i < d; i += 64) evecs[(size_t)place * d + i] = sign * v[i];
    if (lane == 0) evals[place] = lj;
  }
  if (tid == 0) {
    double trace = 0.0;
    for (int i = 0; i < d; ++i) trace += cov[(size_t)i * d + i];
    info[0] = (double)sweeps;
    info[1] = (double)converged;
    info[2] = off;
    info[3] = trace;
  }
}

// ---------------------------------------------------------------- projection and its reverse
__global__ __launch_bounds__(kPcaThreads) void pca_project_kernel(const float* __restrict__ x, int N, int d,
                                                                  const double* __restrict__ mean, const double* __restrict__ W,
                                                                  int k, double scale, float* __restrict__ out) {
  __shared__ double xc[kRowsPerBlock * kPcaMaxD];
  const int tid = threadIdx.x, r0 = blockIdx.x * kRowsPerBlock, rows = min(kRowsPerBlock, N - r0);
  for (int e = tid; e < rows * d; e += kPcaThreads) xc[e] = (double)x[(size_t)r0 * d + e] - mean[e % d];
  __syncthreads();
  for (int item = tid; item < rows * k; item += kPcaThreads) {
    const int r = item / k, c = item % k;
    const double* xr = xc + r * d;
    const double* w = W + (size_t)c * d;
    double acc = 0.0;
    for (int j = 0; j < d; ++j) acc = fma(xr[j], w[j], acc);
    out[(size_t)r0 * k + item] = (float)(scale * acc);
  }
}

__global__ __launch_bounds__(kPcaThreads) void pca_reconstruct_kernel(const float* __restrict__ y, int N, int k,
                                                                      const double* __restrict__ mean,
                                                                      const double* __restrict__ W, int d, float* __restrict__ out) {
  __shared__ double yc[kRowsPerBlock * kPcaMaxD];
  const int tid = threadIdx.x, r0 = blockIdx.x * kRowsPerBlock, rows = min(kRowsPerBlock, N - r0);
  for (int e = tid; e < rows * k; e += kPcaThreads) yc[e] = (double)y[(size_t)r0 * k + e];
  __syncthreads();
  for (int item = tid; item < rows * d; item += kPcaThreads) {
    const int r = item / d, j = item % d;
    const double* yr = yc + r * k;
    double acc = 0.0;
    for (int c = 0; c < k; ++c) acc = fma(yr[c], W[(size_t)c * d + j], acc);
    out[(size_t)r0 * d + item] = (float)(mean[j] + acc);
  }
}

static int pca_chunks(int N) { return (N + kChunkRows - 1) / kChunkRows; }

}  // namespace evae

using namespace evae;

extern "C" int evae_pca_max_features(void) { return kPcaMaxD; }
extern "C" int evae_pca_max_points(void) { return kPcaMaxN; }
extern "C" int evae_pca_chunk_rows(void) { return kChunkRows; }
extern "C" int evae_pca_max_sweeps(void) { return kMaxSweeps; }

extern "C" size_t evae_pca_workspace_bytes(int N, int d) {
  if (N < 1 || d < 1) return 0;
  return (size_t)pca_chunks(N) * ((size_t)d + (size_t)d * d) * sizeof(double);
}

extern "C" size_t evae_pca_eigh_workspace_bytes(int d) {
  return d > kLdsMaxD ? 2 * (size_t)d * d * sizeof(double) : 0;
}

extern "C" int evae_pca_moments(const float* x, int N, int d, double* mean, double* cov, void* ws, size_t ws_bytes,
                                evae_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  static_assert(kTile * kTile == kPcaThreads && kPcaMaxD <= kPcaThreads, "one thread per tile entry and per column");
  EVAE_REQUIRE(d >= 1 && d <= kPcaMaxD, "pca_moments: d=%d outside [1, %d]", d, kPcaMaxD);
  EVAE_REQUIRE(N >= 2 && N <= kPcaMaxN, "pca_moments: N=%d outside [2, %d]", N, kPcaMaxN);
  EVAE_REQUIRE(x && mean && cov && ws, "pca_moments: null pointer");
  EVAE_REQUIRE(aligned8(ws) && aligned8(mean) && aligned8(cov), "pca_moments: misaligned workspace, mean or cov");
  EVAE_REQUIRE(ws_bytes >= evae_pca_workspace_bytes(N, d), "pca_moments: workspace of %zu bytes, %zu needed", ws_bytes,
               evae_pca_workspace_bytes(N, d));
  const int chunks = pca_chunks(N), T = (d + kTile - 1) / kTile;
  double* sums = static_cast<double*>(ws);
  double* gram = sums + (size_t)chunks * d;
  pca_colsum_kernel<<<chunks, kPcaThreads, 0, stream>>>(x, N, d, pow2_width(d, kPcaThreads), sums);
  int rc = check_launch("pca_colsum_kernel");
  if (rc) return rc;
  pca_mean_kernel<<<1, kPcaThreads, 0, stream>>>(sums, chunks, N, d, mean);
  rc = check_launch("pca_mean_kernel");
  if (rc) return rc;
  pca_gram_kernel<<<dim3(T * (T + 1) / 2, chunks), kPcaThreads, 0, stream>>>(x, N, d, mean, gram);
  rc = check_launch("pca_gram_kernel");
  if (rc) return rc;
  pca_cov_finish_kernel<<<(d * d + kPcaThreads - 1) / kPcaThreads, kPcaThreads, 0, stream>>>(gram, chunks, N, d, cov);
  return check_launch("pca_cov_finish_kernel");
}

extern "C" int evae_pca_eigh(const double* cov, int d, double* evals, double* evecs, double* info, void* ws, size_t ws_bytes,
                             evae_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  EVAE_REQUIRE(d >= 1 && d <= kPcaMaxD, "pca_eigh: d=%d outside [1, %d]", d, kPcaMaxD);
  EVAE_REQUIRE(cov && evals && evecs && info, "pca_eigh: null pointer");
  EVAE_REQUIRE(aligned8(cov) && aligned8(evals) && aligned8(evecs) && aligned8(info) && aligned8(ws),
               "pca_eigh: misaligned pointer");
  int waves = (d + 1) / 2;
  waves = waves < 1 ? 1 : (waves > kEighMaxWaves ? kEighMaxWaves : waves);
  if (d <= kLdsMaxD) {
    const int rc = set_max_lds((const void*)pca_eigh_kernel<true>, 2 * kLdsMaxD * kLdsMaxD * (int)sizeof(double), "pca_eigh");
    if (rc) return rc;
    pca_eigh_kernel<true><<<1, 64 * waves, 2 * (size_t)d * d * sizeof(double), stream>>>(cov, d, evals, evecs, info, nullptr);
  } else {
    EVAE_REQUIRE(ws && ws_bytes >= evae_pca_eigh_workspace_bytes(d), "pca_eigh: workspace of %zu bytes, %zu needed", ws_bytes,
                 evae_pca_eigh_workspace_bytes(d));
    pca_eigh_kernel<false><<<1, 64 * waves, 0, stream>>>(cov, d, evals, evecs, info, static_cast<double*>(ws));
  }
  return check_launch("pca_eigh_kernel");
}

extern "C" int evae_pca_project(const float* x, int N, int d, const double* mean, const double* W, int k, double scale, float* out,
                                evae_stream_t stream_) {
  EVAE_REQUIRE(d >= 1 && d <= kPcaMaxD, "pca_project: d=%d outside [1, %d]", d, kPcaMaxD);
  EVAE_REQUIRE(N >= 1 && N <= kPcaMaxN, "pca_project: N=%d outside [1, %d]", N, kPcaMaxN);
  EVAE_REQUIRE(k >= 1 && k <= d, "pca_project: k=%d outside [1, d = %d]", k, d);
  EVAE_REQUIRE(x && mean && W && out, "pca_project: null pointer");
  EVAE_REQUIRE(aligned8(mean) && aligned8(W), "pca_project: misaligned mean or W");
  pca_project_kernel<<<(N + kRowsPerBlock - 1) / kRowsPerBlock, kPcaThreads, 0, (hipStream_t)stream_>>>(x, N, d, mean, W, k,
                                                                                                       scale, out);
  return check_launch("pca_project_kernel");
}

extern "C" int evae_pca_reconstruct(const float* y, int N, int k, const double* mean, const double* W, int d, float* out,
                                    evae_stream_t stream_) {
  EVAE_REQUIRE(d >= 1 && d <= kPcaMaxD, "pca_reconstruct: d=%d outside [1, %d]", d, kPcaMaxD);
  EVAE_REQUIRE(N >= 1 && N <= kPcaMaxN, "pca_reconstruct: N=%d outside [1, %d]", N, kPcaMaxN);
  EVAE_REQUIRE(k >= 1 && k <= d, "pca_reconstruct: k=%d outside [1, d = %d]", k, d);
  EVAE_REQUIRE(y && mean && W && out, "pca_reconstruct: null pointer");
  EVAE_REQUIRE(aligned8(mean) && aligned8(W), "pca_reconstruct: misaligned mean or W");
  pca_reconstruct_kernel<<<(N + kRowsPerBlock - 1) / kRowsPerBlock, kPcaThreads, 0, (hipStream_t)stream_>>>(y, N, k, mean, W, d,
                                                                                                           out);
  return check_launch("pca_reconstruct_kernel");
}
