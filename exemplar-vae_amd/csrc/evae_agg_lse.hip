// Log-density of the aggregate posterior q(z) = 1/N sum_j N(z; mu_j, diag exp(lv_j)) on gfx950, jointly and per dimension, all
// arithmetic in fp64 on fp32 rows: what mutual information, total correlation and the per-dimension KL of the latent code are
// means of (evae/latent_info.py; DESIGN 3.7g has the definitions, the launch sequence and the measurements).  No [B x N] buffer
// exists at any point, there is no atomic and every sum has a fixed order, so equal inputs give bit-equal outputs, and a row's
// bits depend neither on B nor on where the row sits in the batch.
//
//   With w_jd = exp(-lv_jd), c_jd = -(lv_jd + log 2 pi) / 2 and t_ijd = c_jd - (z_id - mu_jd)^2 w_jd / 2 (the difference taken
//   directly, never expanded):
//     log_q[i]      = LSE_j (sum_d t_ijd) - log N          log_qd[i][d] = LSE_j t_ijd - log N
//     log_cond[i][d] = t_{rows[i], d}
//
//   prepare:  thread (j, d): mu, w, c as fp64 into the workspace, each [d x N] (dimension-major: a tile of one dimension is a
//             contiguous run).  The exponentials of the log-variances are taken here, once.
//   per_dim:  a block owns 64 queries x 4 dimensions, wave = dimension, lane = query: every LDS read of a component is a
//             broadcast.  The components pass through LDS in tiles of kAggTile; a thread keeps the tile's 32 terms in registers,
//             takes their maximum m, then s = sum exp(t - m) in index order.
//   joint:    a block owns 64 queries, one per lane; their rows sit in LDS transposed ([d][64]: conflict-free).  A tile's
//             components pass through LDS in chunks of kAggDims dimensions; the thread adds the tile's 32 sums over d in ascending
//             d in registers, then maximum and sum as above.
//   merge:    tiles in index order: (M, S) with (m, s) -> a = exp(-|M - m|); m > M ? (m, S a + s) : (M, S + s a): the
//             larger maximum's side is scaled by exactly 1.  The first tile is taken as it is.  The tile is a constant
//             (evae_agg_lse_tile), so no tuning argument exists that could change a bit.
//   cond:     thread (i, d): the one term of component rows[i]; an index outside [0, N) reads nothing and gives NaN.
//   Rows past B and dimensions past d are clamped for reading and not written; a tile's slots past N hold c = -inf, w = 0:
//   their terms are -inf, exp gives +0, the sums do not move.  Every thread reaches every barrier.
//   NaN:      finite inputs are the caller's contract.  fmax drops a NaN, exp(NaN - m) does not: a NaN term makes the sum NaN.
//             A NaN in z_i reaches row i's outputs and no other row; a NaN in a component reaches every row, as every row's
//             value depends on it.
#include <float.h>

#include "evae_latent.h"

namespace evae {

constexpr int kAggMaxD = 256;
constexpr int kAggMaxN = 1 << 20;
constexpr int kAggTile = 32;                                  // components of one (max, sum) pair
constexpr int kAggRows = 64;                                  // queries of a block: one wave
constexpr int kAggDimsPerBlock = 4;                           // per_dim: waves of a block, one dimension each
constexpr int kAggDims = 32;                                  // joint: dimensions of one staged chunk
constexpr int kAggPrepThreads = 256;
constexpr double kAggLog2Pi = 1.8378770664093454835606594728112;

__global__ __launch_bounds__(kAggPrepThreads) void agg_prepare_kernel(const float* __restrict__ mean,
                                                                       const float* __restrict__ log_var, int N, int d,
                                                                       double* __restrict__ mu, double* __restrict__ w,
                                                                       double* __restrict__ c) {
  const size_t e = (size_t)blockIdx.x * kAggPrepThreads + threadIdx.x;
  if (e >= (size_t)N * d) return;
  const int j = (int)(e / d), k = (int)(e % d);
  const double lv = (double)log_var[e];
  const size_t o = (size_t)k * N + j;
  mu[o] = (double)mean[e];
  w[o] = exp(-lv);
  c[o] = -0.5 * (lv + kAggLog2Pi);
}

// the tile's (m, s) into the running (M, S); `first` is the same in every thread
__device__ __forceinline__ void agg_merge(double& M, double& S, double m, double s, bool first) {
  if (first) {
    M = m;
    S = s;
    return;
  }
  const double a = exp(-fabs(M - m));
  if (m > M) {
    S = S * a + s;
    M = m;
  } else {
    S = S + s * a;
  }
}

// maximum of the tile's terms, then their exponentials added in index order
__device__ __forceinline__ void agg_tile_lse(const double (&t)[kAggTile], double& m, double& s) {
  m = t[0];
#pragma unroll
  for (int u = 1; u < kAggTile; ++u) m = fmax(m, t[u]);
  s = 0.0;
#pragma unroll
  for (int u = 0; u < kAggTile; ++u) s += exp(t[u] - m);
}

// tile slot `u` of dimension k (clamped by the caller): past N a component of weight zero
__device__ __forceinline__ void agg_stage(const double* __restrict__ mu, const double* __restrict__ w,
                                          const double* __restrict__ c, int N, int k, int j, double* smu, double* sw, double* sc) {
  const bool live = j < N;
  const size_t o = (size_t)k * N + (live ? j : 0);
  *smu = live ? mu[o] : 0.0;
  *sw = live ? w[o] : 0.0;
  *sc = live ? c[o] : -HUGE_VAL;
}

__global__ __launch_bounds__(kAggRows* kAggDimsPerBlock) void agg_per_dim_kernel(const float* __restrict__ z, int B, int N, int d,
                                                                                 const double* __restrict__ mu,
                                                                                 const double* __restrict__ w,
                                                                                 const double* __restrict__ c, double log_n,
                                                                                 double* __restrict__ log_qd) {
  __shared__ double smu[kAggDimsPerBlock][kAggTile], sw[kAggDimsPerBlock][kAggTile], sc[kAggDimsPerBlock][kAggTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = blockIdx.x * kAggRows + lane, k = blockIdx.y * kAggDimsPerBlock + wave;
  const int ir = min(i, B - 1), kr = min(k, d - 1);
  const double zv = (double)z[(size_t)ir * d + kr];
  double M = 0.0, S = 0.0;
  for (int j0 = 0; j0 < N; j0 += kAggTile) {
    __syncthreads();                                           // the tile before this one has been read
    if (tid < kAggDimsPerBlock * kAggTile) {
      const int sk = tid / kAggTile, u = tid % kAggTile;
      agg_stage(mu, w, c, N, min(blockIdx.y * kAggDimsPerBlock + sk, d - 1), j0 + u, &smu[sk][u], &sw[sk][u], &sc[sk][u]);
    }
    __syncthreads();
    double t[kAggTile];
#pragma unroll
    for (int u = 0; u < kAggTile; ++u) {
      const double df = zv - smu[wave][u];
      t[u] = sc[wave][u] - 0.5 * (df * df) * sw[wave][u];
    }
    double m, s;
    agg_tile_lse(t, m, s);
    agg_merge(M, S, m, s, j0 == 0);
  }
  if (i < B && k < d) log_qd[(size_t)i * d + k] = M + log(S) - log_n;
}

// dynamic LDS: the block's rows transposed, float [d][64], after the staged chunk
__global__ __launch_bounds__(kAggRows) void agg_joint_kernel(const float* __restrict__ z, int B, int N, int d,
                                                             const double* __restrict__ mu, const double* __restrict__ w,
                                                             const double* __restrict__ c, double log_n,
                                                             double* __restrict__ log_q) {
  __shared__ double smu[kAggDims][kAggTile], sw[kAggDims][kAggTile], sc[kAggDims][kAggTile];
  extern __shared__ float zs[];
  const int lane = threadIdx.x;
  const int i = blockIdx.x * kAggRows + lane;
  const int ir = min(i, B - 1);
  for (int k = 0; k < d; ++k) zs[k * kAggRows + lane] = z[(size_t)ir * d + k];
  double M = 0.0, S = 0.0;
  for (int j0 = 0; j0 < N; j0 += kAggTile) {
    double t[kAggTile];
#pragma unroll
    for (int u = 0; u < kAggTile; ++u) t[u] = 0.0;
    for (int k0 = 0; k0 < d; k0 += kAggDims) {
      const int kc = min(kAggDims, d - k0);
      __syncthreads();                                         // the chunk before this one has been read (and zs is written)
      for (int e = lane; e < kc * kAggTile; e += kAggRows) {
        const int sk = e / kAggTile, u = e % kAggTile;
        agg_stage(mu, w, c, N, k0 + sk, j0 + u, &smu[sk][u], &sw[sk][u], &sc[sk][u]);
      }
      __syncthreads();
      for (int sk = 0; sk < kc; ++sk) {
        const double zv = (double)zs[(k0 + sk) * kAggRows + lane];
#pragma unroll
        for (int u = 0; u < kAggTile; ++u) {
          const double df = zv - smu[sk][u];
          t[u] += sc[sk][u] - 0.5 * (df * df) * sw[sk][u];
        }
      }
    }
    double m, s;
    agg_tile_lse(t, m, s);
    agg_merge(M, S, m, s, j0 == 0);
  }
  if (i < B) log_q[i] = M + log(S) - log_n;
}

__global__ __launch_bounds__(kAggPrepThreads) void agg_cond_kernel(const float* __restrict__ z, int B, int N, int d,
                                                                    const int* __restrict__ rows, const double* __restrict__ mu,
                                                                    const double* __restrict__ w, const double* __restrict__ c,
                                                                    double* __restrict__ log_cond) {
  const size_t e = (size_t)blockIdx.x * kAggPrepThreads + threadIdx.x;
  if (e >= (size_t)B * d) return;
  const int i = (int)(e / d), k = (int)(e % d);
  const int r = rows[i];
  if (r < 0 || r >= N) {
    log_cond[e] = __longlong_as_double(0x7ff8000000000000ll);
    return;
  }
  const size_t o = (size_t)k * N + r;
  const double df = (double)z[e] - mu[o];
  log_cond[e] = c[o] - 0.5 * (df * df) * w[o];
}

struct AggWs {
  size_t mu, w, c, total;
};

static AggWs agg_ws(int N, int d) {
  WsCursor cur;
  AggWs a;
  const size_t bytes = (size_t)N * d * sizeof(double);
  a.mu = cur.take(bytes);
  a.w = cur.take(bytes);
  a.c = cur.take(bytes);
  a.total = cur.o;
  return a;
}

}  // namespace evae

using namespace evae;

extern "C" int evae_agg_lse_max_features(void) { return kAggMaxD; }
extern "C" int evae_agg_lse_max_points(void) { return kAggMaxN; }
extern "C" int evae_agg_lse_tile(void) { return kAggTile; }

extern "C" size_t evae_agg_lse_workspace_bytes(int B, int N, int d) {
  if (B < 1 || N < 1 || N > kAggMaxN || d < 1 || d > kAggMaxD) return 0;
  return agg_ws(N, d).total;
}

extern "C" int evae_agg_lse(const float* z, int B, const float* mean, const float* log_var, int N, int d, const int* rows,
                            double* log_q, double* log_qd, double* log_cond, void* ws, size_t ws_bytes, evae_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  EVAE_REQUIRE(d >= 1 && d <= kAggMaxD, "agg_lse: %d features outside [1, %d]", d, kAggMaxD);
  EVAE_REQUIRE(B >= 1 && B <= kAggMaxN, "agg_lse: B=%d outside [1, %d]", B, kAggMaxN);
  EVAE_REQUIRE(N >= 1 && N <= kAggMaxN, "agg_lse: N=%d outside [1, %d]", N, kAggMaxN);
  EVAE_REQUIRE(log_q || log_qd || log_cond, "agg_lse: no output asked for");
  EVAE_REQUIRE(!log_cond || rows, "agg_lse: log_cond asked for without rows");
  EVAE_REQUIRE(z && mean && log_var && ws, "agg_lse: null pointer");
  EVAE_REQUIRE(aligned8(ws) && aligned8(log_q) && aligned8(log_qd) && aligned8(log_cond), "agg_lse: misaligned fp64 buffer");
  const AggWs a = agg_ws(N, d);
  EVAE_REQUIRE(ws_bytes >= a.total, "agg_lse: workspace of %zu bytes, %zu needed", ws_bytes, a.total);
  char* base = static_cast<char*>(ws);
  double* mu = reinterpret_cast<double*>(base + a.mu);
  double* w = reinterpret_cast<double*>(base + a.w);
  double* c = reinterpret_cast<double*>(base + a.c);
  const double log_n = log((double)N);
  int rc;

  const size_t nd = (size_t)N * d, bd = (size_t)B * d;
  agg_prepare_kernel<<<(unsigned)((nd + kAggPrepThreads - 1) / kAggPrepThreads), kAggPrepThreads, 0, stream>>>(mean, log_var, N, d,
                                                                                                               mu, w, c);
  if ((rc = check_launch("agg_prepare_kernel"))) return rc;
  if (log_cond) {
    agg_cond_kernel<<<(unsigned)((bd + kAggPrepThreads - 1) / kAggPrepThreads), kAggPrepThreads, 0, stream>>>(z, B, N, d, rows, mu,
                                                                                                              w, c, log_cond);
    if ((rc = check_launch("agg_cond_kernel"))) return rc;
  }
  if (log_q) {
    const int zs_bytes = d * kAggRows * (int)sizeof(float);      // <= 64 KiB beside 24 KiB of static LDS
    // Only a wide input needs more LDS than a launch gets unasked: the latents' d = 40 (10 KiB) goes without this host call.
    if (zs_bytes > 32 * 1024 && (rc = set_max_lds((const void*)agg_joint_kernel, zs_bytes, "agg_joint_kernel"))) return rc;
    agg_joint_kernel<<<cdiv(B, kAggRows), kAggRows, zs_bytes, stream>>>(z, B, N, d, mu, w, c, log_n, log_q);
    if ((rc = check_launch("agg_joint_kernel"))) return rc;
  }
  if (log_qd) {
    const dim3 grid(cdiv(B, kAggRows), cdiv(d, kAggDimsPerBlock));
    agg_per_dim_kernel<<<grid, kAggRows * kAggDimsPerBlock, 0, stream>>>(z, B, N, d, mu, w, c, log_n, log_qd);
    if ((rc = check_launch("agg_per_dim_kernel"))) return rc;
  }
  return EVAE_OK;
}
