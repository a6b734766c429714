// Exact t-SNE of a latent space on gfx950 (van der Maaten & Hinton 2008; constructor and update rule of scikit-learn's
// sklearn.manifold.TSNE, method='exact').  DESIGN 3.7 has the formulas, the launch sequence and the byte / operation counts.
//
//   affinities: one workgroup (N > kWaveRowMax) or one wave per row.  The row of squared distances sits in LDS, its minimum over
//               j != i subtracted; a bracketing bisection of FIXED length finds the precision beta_i at which the conditional
//               p(j|i) ~ exp(-beta_i d_ij) has entropy log(perplexity).  The search runs in fp64 (one exp per pair per step, the
//               sums in a fixed order), so every lane of a row takes the same branch at every step and the result is the same on
//               every run.  The conditionals overwrite the distances row by row; a second launch forms
//               P_ij = (p(j|i) + p(i|j)) / 2N on pairs of 32 x 32 tiles, the SAME float sum a + b on both sides of the diagonal.
//   forces:     a workgroup owns kForceRows rows of P and streams them once, lane -> column (coalesced 256 B per wave and row);
//               y_j is loaded once per column and reused for the rows.  Per pair: one IEEE reciprocal, no exponential.  Every
//               per-row sum (attraction, repulsion, the row's share of Z, optionally of KL) is a fp64 accumulator per lane,
//               combined across lanes and waves in a fixed order -- no atomics.
//   update:     ONE workgroup: Z (and KL) as fixed-order fp64 sums over the rows, gradient, scikit-learn's gains / velocity
//               update, the re-centring of Y.  It needs Z of every row, hence the second launch of an iteration; there is no
//               grid-wide barrier anywhere in this file.  evae_tsne_nn.hip (sparse P, N above the cap below) ends its iteration
//               with this launch too.
#include "evae_common.h"

namespace evae {

constexpr int kTsneMaxPoints = 32768;   // a row of distances must fit one workgroup's LDS: 64 B + 4 N <= 160 KiB
constexpr int kWaveRowMax = 1024;       // N <= this: one wave per row (a 256-thread block would idle three waves in four)
constexpr int kForceRows = 8;
constexpr int kForceThreads = 256;
constexpr int kUpdateThreads = 1024;
constexpr int kPartStride = 8;          // evae_tsne_forces' row record, in doubles (include/evae_hip.h)

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}

// sum over the NTB threads of a block, the same value (same order of additions) in every thread; red: NTB / 64 doubles
template <int NTB>
__device__ __forceinline__ double block_sum(double v, double* red) {
  v = wave_sum(v);
  if (NTB == 64) return v;
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[wave] = v;
  __syncthreads();
  double t = red[0];
#pragma unroll
  for (int w = 1; w < NTB / 64; ++w) t += red[w];
  __syncthreads();
  return t;
}

// d2 and cond may be the same buffer: a block reads its whole row into LDS before it writes the row back.
template <int NTB>
__global__ __launch_bounds__(NTB) void tsne_beta_kernel(const float* d2, int N, double log_perp, int steps,
                                                         float* __restrict__ beta_out, float* cond) {
  extern __shared__ __attribute__((aligned(16))) double tsne_smem[];
  double* red = tsne_smem;                                  // 8 doubles
  float* row = reinterpret_cast<float*>(tsne_smem + 8);     // [N]
  const int i = blockIdx.x;
  const int tid = threadIdx.x;
  const float* src = d2 + (size_t)i * N;

  float m = INFINITY;
  for (int j = tid; j < N; j += NTB) {
    const float v = src[j];
    row[j] = v;
    if (j != i) m = fminf(m, v);
  }
  m = wave_min(m);
  if (NTB > 64) {
    float* redf = reinterpret_cast<float*>(red);
    if ((tid & 63) == 0) redf[tid >> 6] = m;
    __syncthreads();
    m = redf[0];
#pragma unroll
    for (int w = 1; w < NTB / 64; ++w) m = fminf(m, redf[w]);
  }
  __syncthreads();                                          // row[] complete; redf read before red is reused
  const double dmin = (double)m;

  double beta = 1.0, lo = 0.0, hi = 0.0;
  bool has_lo = false, has_hi = false;
  for (int s = 0; s < steps; ++s) {
    double S = 0.0, SD = 0.0;
    for (int j = tid; j < N; j += NTB) {
      if (j == i) continue;
      const double dd = (double)row[j] - dmin;
      const double e = exp(-beta * dd);
      S += e;
      SD = fma(dd, e, SD);
    }
    S = block_sum<NTB>(S, red);
    SD = block_sum<NTB>(SD, red);
    const double H = log(S) + beta * SD / S;                // S >= 1: the nearest neighbour contributes exp(0)
    if (H > log_perp) {                                     // too flat: raise the precision
      lo = beta; has_lo = true;
      beta = has_hi ? 0.5 * (beta + hi) : 2.0 * beta;
    } else {
      hi = beta; has_hi = true;
      beta = has_lo ? 0.5 * (beta + lo) : 0.5 * beta;
    }
  }
  double S = 0.0;
  for (int j = tid; j < N; j += NTB) {
    if (j == i) continue;
    S += exp(-beta * ((double)row[j] - dmin));
  }
  S = block_sum<NTB>(S, red);
  float* dst = cond + (size_t)i * N;
  for (int j = tid; j < N; j += NTB)
    dst[j] = (j == i) ? 0.0f : (float)(exp(-beta * ((double)row[j] - dmin)) / S);
  if (tid == 0) beta_out[i] = (float)beta;
}

// in place: P_ij = P_ji = (c_ij + c_ji) / 2N.  Block (bx, by), bx >= by, owns the tile pair (by, bx) / (bx, by).
__global__ __launch_bounds__(256) void tsne_symmetrise_kernel(float* P, int N, float two_n) {
  if (blockIdx.x < blockIdx.y) return;
  __shared__ float A[32][33];
  __shared__ float B[32][33];
  const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const bool diag = blockIdx.x == blockIdx.y;
  for (int r = ty; r < 32; r += 8) {
    const int ra = r0 + r, ca = c0 + tx;                    // A = tile (r0, c0)
    A[r][tx] = (ra < N && ca < N) ? P[(size_t)ra * N + ca] : 0.0f;
    const int rb = c0 + r, cb = r0 + tx;                    // B = tile (c0, r0)
    B[r][tx] = (rb < N && cb < N) ? P[(size_t)rb * N + cb] : 0.0f;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int ra = r0 + r, ca = c0 + tx;
    if (ra < N && ca < N) P[(size_t)ra * N + ca] = (A[r][tx] + B[tx][r]) / two_n;
    if (!diag) {
      const int rb = c0 + r, cb = r0 + tx;
      if (rb < N && cb < N) P[(size_t)rb * N + cb] = (A[tx][r] + B[r][tx]) / two_n;     // the same a + b as above
    }
  }
}

template <bool KL>
__global__ __launch_bounds__(kForceThreads) void tsne_forces_kernel(const float* __restrict__ P, const float* __restrict__ Y,
                                                                   int N, double exag, double* __restrict__ part) {
  constexpr int NV = KL ? 7 : 5;
  __shared__ double red[kForceThreads / 64][kForceRows * 7];
  const int i0 = blockIdx.x * kForceRows;
  const int tid = threadIdx.x;
  float yix[kForceRows], yiy[kForceRows];
  const float* prow[kForceRows];
  int irow[kForceRows];
#pragma unroll
  for (int r = 0; r < kForceRows; ++r) {
    const int ii = min(i0 + r, N - 1);                      // rows past the end repeat the last one and are not written
    irow[r] = ii;
    yix[r] = Y[2 * ii];
    yiy[r] = Y[2 * ii + 1];
    prow[r] = P + (size_t)ii * N;
  }
  double acc[kForceRows][NV];
#pragma unroll
  for (int r = 0; r < kForceRows; ++r)
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[r][v] = 0.0;

  for (int j = tid; j < N; j += kForceThreads) {
    const float2 yj = reinterpret_cast<const float2*>(Y)[j];
    float p[kForceRows];
#pragma unroll
    for (int r = 0; r < kForceRows; ++r) p[r] = prow[r][j];
#pragma unroll
    for (int r = 0; r < kForceRows; ++r) {
      const float dx = yix[r] - yj.x, dy = yiy[r] - yj.y;
      const float q = 1.0f + (dx * dx + dy * dy);
      const float w = 1.0f / q;
      const float pw = p[r] * w;
      const float w2 = w * w;
      acc[r][0] += (double)(pw * dx);
      acc[r][1] += (double)(pw * dy);
      acc[r][2] += (double)(w2 * dx);
      acc[r][3] += (double)(w2 * dy);
      acc[r][4] += (j != irow[r]) ? (double)w : 0.0;
      if (KL) {
        if (p[r] > 0.0f) acc[r][5] = fma((double)p[r], log((double)p[r] * (double)q), acc[r][5]);
        acc[r][6] += (double)p[r];
      }
    }
  }
  const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int r = 0; r < kForceRows; ++r)
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const double t = wave_sum(acc[r][v]);
      if (lane == 0) red[wave][r * 7 + v] = t;
    }
  __syncthreads();
  if (tid < kForceRows * 7) {
    const int r = tid / 7, v = tid - r * 7;
    const int i = i0 + r;
    if (i < N) {
      double t = 0.0;
      if (v < NV) {
        t = red[0][tid];
#pragma unroll
        for (int w = 1; w < kForceThreads / 64; ++w) t += red[w][tid];
        if (v < 2) t *= exag;
      }
      part[(size_t)i * kPartStride + v] = t;
    }
  }
}

// one block.  Y == nullptr: Z and KL only.
__global__ __launch_bounds__(kUpdateThreads) void tsne_update_kernel(const double* __restrict__ part, int N, int want_kl,
                                                                    double momentum, double lr, float* __restrict__ Y,
                                                                    float* __restrict__ vel, float* __restrict__ gains,
                                                                    float* __restrict__ grad, double* __restrict__ stats) {
  __shared__ double red[kUpdateThreads / 64];
  const int tid = threadIdx.x;
  double z = 0.0, kl = 0.0, sp = 0.0;
  for (int i = tid; i < N; i += kUpdateThreads) {
    z += part[(size_t)i * kPartStride + 4];
    if (want_kl) {
      kl += part[(size_t)i * kPartStride + 5];
      sp += part[(size_t)i * kPartStride + 6];
    }
  }
  const double Z = block_sum<kUpdateThreads>(z, red);
  double KLv = 0.0;
  if (want_kl) {                                            // sum p log(p / (w / Z)) = sum p log(p / w) + log Z sum p
    const double a = block_sum<kUpdateThreads>(kl, red);
    const double b = block_sum<kUpdateThreads>(sp, red);
    KLv = a + log(Z) * b;
  }
  if (tid == 0 && stats) {
    stats[0] = Z;
    stats[1] = KLv;
  }
  if (Y == nullptr) return;

  double mx = 0.0, my = 0.0;
  for (int i = tid; i < N; i += kUpdateThreads) {
    const double* pr = part + (size_t)i * kPartStride;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int e = 2 * i + c;
      const double g = 4.0 * (pr[c] - pr[2 + c] / Z);
      if (grad) grad[e] = (float)g;
      const double v = (double)vel[e];
      double ga = (double)gains[e];
      ga = (v * g < 0.0) ? ga + 0.2 : ga * 0.8;
      ga = fmax(ga, 0.01);
      const double vn = momentum * v - lr * ga * g;
      const double yn = (double)Y[e] + vn;
      gains[e] = (float)ga;
      vel[e] = (float)vn;
      Y[e] = (float)yn;
      if (c == 0) mx += yn; else my += yn;
    }
  }
  mx = block_sum<kUpdateThreads>(mx, red) / (double)N;
  my = block_sum<kUpdateThreads>(my, red) / (double)N;
  for (int i = tid; i < N; i += kUpdateThreads) {           // a thread re-reads only what it wrote itself
    Y[2 * i] = (float)((double)Y[2 * i] - mx);
    Y[2 * i + 1] = (float)((double)Y[2 * i + 1] - my);
  }
}

}  // namespace evae

using namespace evae;

extern "C" int evae_tsne_max_points(void) { return kTsneMaxPoints; }

extern "C" int evae_tsne_affinities(const float* d2, int N, double perplexity, int steps, float* beta, float* P,
                                    evae_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  EVAE_REQUIRE(N >= 2 && N <= kTsneMaxPoints, "tsne_affinities: N=%d outside [2, %d]", N, kTsneMaxPoints);
  EVAE_REQUIRE(perplexity > 0.0 && perplexity < (double)N, "tsne_affinities: perplexity %g outside (0, N=%d)", perplexity, N);
  EVAE_REQUIRE(steps >= 1 && steps <= 1000, "tsne_affinities: steps=%d outside [1, 1000]", steps);
  EVAE_REQUIRE(d2 && beta && P, "tsne_affinities: null pointer");
  const size_t lds = 8 * sizeof(double) + (size_t)N * sizeof(float);
  const double log_perp = log(perplexity);
  if (N <= kWaveRowMax) {
    tsne_beta_kernel<64><<<N, 64, lds, stream>>>(d2, N, log_perp, steps, beta, P);
  } else {
    static bool attr = false;
    if (!attr) {
      (void)hipFuncSetAttribute((const void*)tsne_beta_kernel<256>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      attr = true;
    }
    tsne_beta_kernel<256><<<N, 256, lds, stream>>>(d2, N, log_perp, steps, beta, P);
  }
  int rc = check_launch("tsne_beta_kernel");
  if (rc) return rc;
  const int nt = cdiv(N, 32);
  tsne_symmetrise_kernel<<<dim3(nt, nt), 256, 0, stream>>>(P, N, 2.0f * (float)N);
  return check_launch("tsne_symmetrise_kernel");
}

extern "C" int evae_tsne_forces(const float* P, const float* Y, int N, double exaggeration, int want_kl, double* part,
                                evae_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  EVAE_REQUIRE(N >= 2 && N <= kTsneMaxPoints, "tsne_forces: N=%d outside [2, %d]", N, kTsneMaxPoints);
  EVAE_REQUIRE(P && Y && part, "tsne_forces: null pointer");
  EVAE_REQUIRE(((uintptr_t)Y & 7) == 0, "tsne_forces: Y must be 8-byte aligned");
  const int nb = cdiv(N, kForceRows);
  if (want_kl) tsne_forces_kernel<true><<<nb, kForceThreads, 0, stream>>>(P, Y, N, exaggeration, part);
  else tsne_forces_kernel<false><<<nb, kForceThreads, 0, stream>>>(P, Y, N, exaggeration, part);
  return check_launch("tsne_forces_kernel");
}

// update and stats serve the sparse path too (evae_tsne_nn.hip): one workgroup strides over any N, so their bound is that path's
extern "C" int evae_tsne_update(const double* part, int N, int want_kl, double momentum, double lr, float* Y, float* velocity,
                                float* gains, float* grad, double* stats, evae_stream_t stream_) {
  EVAE_REQUIRE(N >= 2 && N <= evae_tsne_nn_max_points(), "tsne_update: N=%d outside [2, %d]", N, evae_tsne_nn_max_points());
  EVAE_REQUIRE(part && Y && velocity && gains, "tsne_update: null pointer");
  tsne_update_kernel<<<1, kUpdateThreads, 0, (hipStream_t)stream_>>>(part, N, want_kl, momentum, lr, Y, velocity, gains, grad,
                                                                    stats);
  return check_launch("tsne_update_kernel");
}

extern "C" int evae_tsne_stats(const double* part, int N, int want_kl, double* stats, evae_stream_t stream_) {
  EVAE_REQUIRE(N >= 2 && N <= evae_tsne_nn_max_points(), "tsne_stats: N=%d outside [2, %d]", N, evae_tsne_nn_max_points());
  EVAE_REQUIRE(part && stats, "tsne_stats: null pointer");
  tsne_update_kernel<<<1, kUpdateThreads, 0, (hipStream_t)stream_>>>(part, N, want_kl, 0.0, 0.0, nullptr, nullptr, nullptr,
                                                                    nullptr, stats);
  return check_launch("tsne_update_kernel");
}
