// Gaussian mixture of the latent space on gfx950: EM, densities and sampling, all arithmetic in fp64 on fp32 rows
// (evae/mixture.py; DESIGN 3.7e has the formulas, the order of every sum and the measurements).  The only atomic is an integer
// minimum (the first component whose covariance is not positive definite): every floating-point sum has a fixed order, so equal
// inputs give bit-equal outputs.  Plain fp64 fma throughout, no matrix instruction.
//
//   params:   one fp64 buffer, K-major blocks: weights [K] | n_k [K] | log_det [K] | means [K x d] | b [K x d] | cov [K x cs] |
//             prec [K x cs], cs = d*d ('full'), d ('diag') or 1 ('spherical').  prec is P_k, upper triangular with
//             P_k P_k^T = Sigma_k^-1 (scikit-learn's precisions_cholesky_), b_k = mu_k P_k, log_det_k = sum_j log P_k[j,j].
//   estep:    a block owns kGmStrip rows, staged in LDS as fp32 with an odd row stride; the factors pass through LDS in tiles of
//             T <= 4 components (the upper triangle packed by columns, with b_k).  Thread (row, group g) owns component t0 + g of
//             the tile: y_j = (sum_{i<=j} x_i P[i,j], i ascending, by fma) - b_j; m = sum_j y_j^2, j ascending, by fma;
//             log N + log pi_k goes to log_resp.  Then one lane per row: the maximum over k, sum_k exp(. - max) in ascending k,
//             log p(x_i) = max + log(sum), log_resp -= log p(x_i).  The strip's sum of log p(x_i) in row order by one thread.
//   wsum:     a block per (chunk of kGmChunk rows, component): r_i = exp(log_resp[i, k]) (or labels[i] == k) once into LDS;
//             columns across threads, rows g, g + G, .. per thread and the G partial sums in order of g.  Mode 0: sum r x and, as
//             column d, sum r.  Mode 1 ('diag', 'spherical'): sum r (x - mu_k)^2 about the NEW means.
//   means:    thread (k, c): the chunks in index order; n_k = sum r + 10 eps; mu_k = sum r x / n_k.
//   scatter:  'full': a block per (chunk, component); sub-tiles of kGmSub centred rows in LDS as fp64; a thread owns up to
//             kGmPerThread entries (a <= b) of the upper triangle and adds r (x_a - mu_a)(x_b - mu_b) over the chunk's rows in
//             index order.  A row of r == 0 adds exactly nothing and is skipped.
//   finish:   a block per component: the chunks in index order, / n_k, + reg_covar on the diagonal; 'full': Cholesky in LDS
//             (left-looking, every inner product in ascending index), the inverse of L column by column into the upper
//             triangle (= P), b and log_det.  A pivot or a variance that is not > 0 stops the component before any square
//             root or division: its index goes to `fail` by atomicMin, its P, b and log_det stay as they were.
//   record:   ONE workgroup: pi_k = n_k / sum n (k ascending), the lower bound = (strip sums in strip order) / N, the record.
//   Every kernel of a step starts with `if (state[1] != 0) return` -- the same value in every thread of the grid, written by an
//   EARLIER launch of the stream: nothing polls, nothing waits on another workgroup.  A step is six launches.
#include <float.h>

#include "evae_latent.h"

namespace evae {

constexpr int kGmMaxK = 256;
constexpr int kGmMaxDFull = 96;
constexpr int kGmMaxD = 256;
constexpr int kGmMaxN = 1 << 20;
constexpr int kGmChunk = 512;
constexpr int kGmStrip = 64;                                 // one wave of rows
constexpr int kGmThreads = 256;
constexpr int kGmGroups = kGmThreads / kGmStrip;             // 4: the most components of a tile
constexpr int kGmSub = 64;                                   // centred rows of a scatter sub-tile
constexpr int kGmMaxTri = kGmMaxDFull * (kGmMaxDFull + 1) / 2;
constexpr int kGmPerThread = (kGmMaxTri + kGmThreads - 1) / kGmThreads;   // 19
constexpr int kGmOneThreads = 1024;
constexpr size_t kGmMaxBytes = (size_t)1 << 30;
constexpr int kGmLdsBudget = 150 * 1024;
constexpr double kGmLog2Pi = 1.8378770664093454835606594728112;
enum { kGmFull = 0, kGmDiag = 1, kGmSph = 2 };

struct GmParams {
  double *w, *nk, *ld, *mu, *b, *cov, *prec;
  int cs;
};

__host__ __device__ inline int gm_cov_size(int d, int type) { return type == kGmFull ? d * d : (type == kGmDiag ? d : 1); }
__host__ __device__ inline size_t gm_params_doubles(int d, int K, int type) {
  return (size_t)K * (3 + 2 * (size_t)d + 2 * (size_t)gm_cov_size(d, type));
}
__host__ __device__ inline GmParams gm_params(double* p, int d, int K, int type) {
  GmParams q;
  q.cs = gm_cov_size(d, type);
  q.w = p;
  q.nk = p + K;
  q.ld = p + 2 * (size_t)K;
  q.mu = p + 3 * (size_t)K;
  q.b = q.mu + (size_t)K * d;
  q.cov = q.b + (size_t)K * d;
  q.prec = q.cov + (size_t)K * q.cs;
  return q;
}

// ---------------------------------------------------------------- E-step
static int gm_factor_doubles(int d, int type) { return type == kGmFull ? d * (d + 1) / 2 : (type == kGmDiag ? d : 1); }
static size_t gm_estep_rows_bytes(int d) { return (size_t)kGmStrip * (d | 1) * sizeof(float) + kGmStrip * sizeof(double); }
static int gm_estep_tile(int d, int type) {
  const size_t per = (size_t)(gm_factor_doubles(d, type) + d) * sizeof(double);
  const size_t fit = (kGmLdsBudget - gm_estep_rows_bytes(d)) / per;
  return fit >= (size_t)kGmGroups ? kGmGroups : (int)fit;
}
static size_t gm_estep_lds(int d, int type) {
  return (size_t)gm_estep_tile(d, type) * (gm_factor_doubles(d, type) + d) * sizeof(double) + gm_estep_rows_bytes(d);
}

template <int TYPE>
__global__ __launch_bounds__(kGmThreads) void gmm_estep_kernel(const float* __restrict__ x, int N, int d, int K, double* params,
                                                               int T, double* log_resp, double* __restrict__ logp,
                                                               double* __restrict__ strip_sum, const double* state) {
  if (step_done(state)) return;
  extern __shared__ __attribute__((aligned(16))) double gm_smem[];
  const GmParams q = gm_params(params, d, K, TYPE);
  const int ps = TYPE == kGmFull ? d * (d + 1) / 2 : (TYPE == kGmDiag ? d : 1);
  double* pf = gm_smem;                                            // [T x ps]
  double* bt = pf + (size_t)T * ps;                                // [T x d]
  double* red = bt + (size_t)T * d;                                // [kGmStrip]
  float* xr = reinterpret_cast<float*>(red + kGmStrip);            // [kGmStrip x ldx]
  const int tid = threadIdx.x, r = tid & (kGmStrip - 1), g = tid / kGmStrip;
  const int r0 = blockIdx.x * kGmStrip, rows = min(kGmStrip, N - r0), ldx = d | 1;
  for (int e = tid; e < kGmStrip * d; e += kGmThreads) {
    const int rr = e / d, c = e - rr * d;
    xr[rr * ldx + c] = rr < rows ? x[(size_t)r0 * d + e] : 0.f;
  }
  const float* xrow = xr + r * ldx;
  const double dlog = (double)d * kGmLog2Pi;
  for (int t0 = 0; t0 < K; t0 += T) {
    __syncthreads();                                               // the rows are staged; the last tile has been read
    const int tn = min(T, K - t0);
    if (TYPE == kGmFull) {
      for (int e = tid; e < tn * d * d; e += kGmThreads) {
        const int t = e / (d * d), ij = e - t * d * d, i = ij / d, j = ij - i * d;
        if (i <= j) pf[(size_t)t * ps + j * (j + 1) / 2 + i] = q.prec[(size_t)(t0 + t) * d * d + ij];
      }
    } else {
      for (int e = tid; e < tn * ps; e += kGmThreads) pf[e] = q.prec[(size_t)t0 * ps + e];
    }
    for (int e = tid; e < tn * d; e += kGmThreads) bt[e] = q.b[(size_t)t0 * d + e];
    __syncthreads();
    const int k = t0 + g;
    if (g < tn && r < rows) {
      const double* bk = bt + g * d;
      double m = 0.0;
      if (TYPE == kGmFull) {
        const double* col = pf + (size_t)g * ps;
        for (int j = 0; j < d; ++j) {
          double acc = 0.0;
          for (int i = 0; i <= j; ++i) acc = fma((double)xrow[i], col[i], acc);
          col += j + 1;
          const double y = acc - bk[j];
          m = fma(y, y, m);
        }
      } else {
        const double* pk = pf + (size_t)g * ps;
        for (int j = 0; j < d; ++j) {
          const double y = (double)xrow[j] * (TYPE == kGmDiag ? pk[j] : pk[0]) - bk[j];
          m = fma(y, y, m);
        }
      }
      log_resp[(size_t)(r0 + r) * K + k] = (-0.5 * (dlog + m) + q.ld[k]) + log(q.w[k]);
    }
  }
  __syncthreads();                                                 // the block's own writes to log_resp
  if (g == 0) {                                                    // wave 0: one lane per row
    double lse = 0.0;
    if (r < rows) {
      double* lr = log_resp + (size_t)(r0 + r) * K;
      double mx = -INFINITY;
      for (int k = 0; k < K; ++k) mx = fmax(mx, lr[k]);
      double s = 0.0;
      for (int k = 0; k < K; ++k) s += exp(lr[k] - mx);
      lse = mx + log(s);
      for (int k = 0; k < K; ++k) lr[k] -= lse;
      logp[r0 + r] = lse;
    }
    red[r] = lse;
  }
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int e = 0; e < rows; ++e) s += red[e];
    strip_sum[blockIdx.x] = s;
  }
}

// ---------------------------------------------------------------- weighted column sums (pass 1; pass 2 of 'diag' / 'spherical')
template <int MODE>
__global__ __launch_bounds__(kGmThreads) void gmm_wsum_kernel(const float* __restrict__ x, int N, int d, int K, int W,
                                                              const double* __restrict__ log_resp, const int* __restrict__ labels,
                                                              const double* __restrict__ mu, double* __restrict__ partial,
                                                              int* fail, const double* state) {
  if (step_done(state)) return;
  __shared__ double rr[kGmChunk];
  __shared__ double part[kGmThreads];
  const int tid = threadIdx.x, k = blockIdx.y, c0 = blockIdx.x * kGmChunk, n = min(kGmChunk, N - c0);
  const int cols = MODE == 0 ? d + 1 : d;
  if (MODE == 0 && fail && tid == 0 && blockIdx.x == 0 && k == 0) *fail = kNoIndex;   // read by the finish of this same pass
  for (int e = tid; e < kGmChunk; e += kGmThreads) {
    double v = 0.0;
    if (e < n) v = log_resp ? exp(log_resp[(size_t)(c0 + e) * K + k]) : (labels[c0 + e] == k ? 1.0 : 0.0);
    rr[e] = v;
  }
  __syncthreads();
  const int c = tid & (W - 1), g = tid / W, G = kGmThreads / W;
  for (int cb = 0; cb < cols; cb += W) {
    const int cc = cb + c;
    double s = 0.0;
    if (cc < cols) {
      if (MODE == 0) {
        if (cc < d) {
          for (int p = g; p < n; p += G) s = fma(rr[p], (double)x[(size_t)(c0 + p) * d + cc], s);
        } else {
          for (int p = g; p < n; p += G) s += rr[p];
        }
      } else {
        const double m = mu[(size_t)k * d + cc];
        for (int p = g; p < n; p += G) {
          const double df = (double)x[(size_t)(c0 + p) * d + cc] - m;
          s = fma(rr[p], df * df, s);
        }
      }
    }
    part[tid] = s;
    __syncthreads();
    if (g == 0 && cc < cols) {
      double t = 0.0;
      for (int h = 0; h < G; ++h) t += part[h * W + c];
      partial[((size_t)blockIdx.x * K + k) * cols + cc] = t;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kGmThreads) void gmm_means_kernel(const double* __restrict__ partial, int chunks, int d, int K,
                                                               double* params, int type, const double* state) {
  if (step_done(state)) return;
  const int idx = blockIdx.x * kGmThreads + threadIdx.x, cols = d + 1;
  if (idx >= K * cols) return;
  const int k = idx / cols, c = idx - k * cols;
  const GmParams q = gm_params(params, d, K, type);
  double sn = 0.0, sx = 0.0;
  for (int ch = 0; ch < chunks; ++ch) {
    const double* p = partial + ((size_t)ch * K + k) * cols;
    sn += p[d];
    sx += p[c];
  }
  const double nk = sn + 10.0 * DBL_EPSILON;
  if (c == d) q.nk[k] = nk;
  else q.mu[(size_t)k * d + c] = sx / nk;
}

// ---------------------------------------------------------------- weighted scatter about the new means ('full')
__device__ __forceinline__ void gm_tri_entry(int e, int d, int& a, int& b) {   // e-th entry (a <= b) of the upper triangle by rows
  a = 0;
  int rem = e;
  while (rem >= d - a) {
    rem -= d - a;
    ++a;
  }
  b = a + rem;
}

static size_t gm_scatter_lds(int d) { return ((size_t)kGmSub * (d | 1) + kGmSub) * sizeof(double); }

__global__ __launch_bounds__(kGmThreads) void gmm_scatter_kernel(const float* __restrict__ x, int N, int d, int K,
                                                                 const double* __restrict__ log_resp,
                                                                 const int* __restrict__ labels, const double* __restrict__ mu,
                                                                 double* __restrict__ partial, const double* state) {
  if (step_done(state)) return;
  extern __shared__ __attribute__((aligned(16))) double gm_smem[];
  const int ldc = d | 1, E = d * (d + 1) / 2;
  double* xc = gm_smem;                                            // [kGmSub x ldc]
  double* rs = xc + (size_t)kGmSub * ldc;                          // [kGmSub]
  const int tid = threadIdx.x, k = blockIdx.y, c0 = blockIdx.x * kGmChunk, n = min(kGmChunk, N - c0);
  const int nu = (E + kGmThreads - 1) / kGmThreads;               // entries per thread at this d: the same in every thread
  int ia[kGmPerThread], ib[kGmPerThread];
  double acc[kGmPerThread];
#pragma unroll
  for (int u = 0; u < kGmPerThread; ++u) {
    const int e = tid + u * kGmThreads;
    ia[u] = ib[u] = 0;
    if (e < E) gm_tri_entry(e, d, ia[u], ib[u]);
    acc[u] = 0.0;
  }
  for (int s0 = 0; s0 < n; s0 += kGmSub) {
    const int sn = min(kGmSub, n - s0);
    __syncthreads();                                               // the last sub-tile has been read
    for (int e = tid; e < kGmSub * d; e += kGmThreads) {
      const int rr = e / d, c = e - rr * d;
      xc[rr * ldc + c] = rr < sn ? (double)x[(size_t)(c0 + s0) * d + e] - mu[(size_t)k * d + c] : 0.0;
    }
    if (tid < kGmSub) {
      double v = 0.0;
      if (tid < sn) {
        const int i = c0 + s0 + tid;
        v = log_resp ? exp(log_resp[(size_t)i * K + k]) : (labels[i] == k ? 1.0 : 0.0);
      }
      rs[tid] = v;
    }
    __syncthreads();
    for (int row = 0; row < sn; ++row) {
      const double w = rs[row];                                    // a broadcast: the same in every thread
      if (w == 0.0) continue;
      const double* xw = xc + row * ldc;
#pragma unroll
      for (int u = 0; u < kGmPerThread; ++u)
        if (u < nu) acc[u] = fma(w * xw[ia[u]], xw[ib[u]], acc[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < kGmPerThread; ++u) {
    const int e = tid + u * kGmThreads;
    if (e < E) partial[((size_t)blockIdx.x * K + k) * E + e] = acc[u];
  }
}

// ---------------------------------------------------------------- finish: covariance -> precision factor, b, log_det
static size_t gm_finish_lds(int d, int type) {
  return type == kGmFull ? ((size_t)d * (d | 1) + d + 2) * sizeof(double) : ((size_t)d + 2) * sizeof(double);
}

template <int TYPE>
__global__ __launch_bounds__(kGmThreads) void gmm_finish_kernel(const double* __restrict__ partial, int chunks, int d, int K,
                                                                double reg, double* params, int* fail, const double* state) {
  if (step_done(state)) return;
  extern __shared__ __attribute__((aligned(16))) double gm_smem[];
  const int tid = threadIdx.x, k = blockIdx.x;
  const GmParams q = gm_params(params, d, K, TYPE);
  const double nk = q.nk[k];
  if (TYPE == kGmFull) {
    const int ld = d | 1, E = d * (d + 1) / 2;
    double* A = gm_smem;                                           // [d x ld]
    double* tmp = A + (size_t)d * ld;                              // [d]
    for (int e = tid; e < E; e += kGmThreads) {
      int a, b;
      gm_tri_entry(e, d, a, b);
      double s = 0.0;
      for (int ch = 0; ch < chunks; ++ch) s += partial[((size_t)ch * K + k) * E + e];
      double v = s / nk;
      if (a == b) v += reg;
      A[a * ld + b] = v;
      A[b * ld + a] = v;
      q.cov[(size_t)k * d * d + a * d + b] = v;
      q.cov[(size_t)k * d * d + b * d + a] = v;
    }
    __syncthreads();
    // left-looking Cholesky: L in the lower triangle.  s_i = A[i,j] - sum_{m<j} L[i,m] L[j,m], m ascending.
    for (int j = 0; j < d; ++j) {
      double s = 0.0;
      if (tid >= j && tid < d) {
        s = A[tid * ld + j];
        for (int m = 0; m < j; ++m) s = fma(-A[tid * ld + m], A[j * ld + m], s);
        tmp[tid] = s;
      }
      __syncthreads();
      const double piv = tmp[j];                                   // the same in every thread
      if (!(piv > 0.0) || !(piv < INFINITY)) {                     // not positive definite: no square root, no division
        if (tid == 0) atomicMin(fail, k);
        return;
      }
      const double root = sqrt(piv);
      if (tid == j) A[j * ld + j] = root;
      else if (tid > j && tid < d) A[tid * ld + j] = s / root;
      __syncthreads();
    }
    // column c of L^-1 into row c of the upper triangle: z_c = 1 / L[c,c], z_i = -(sum_{m=c}^{i-1} L[i,m] z_m) / L[i,i]
    if (tid < d) {
      const int c = tid;
      const double zc = 1.0 / A[c * ld + c];
      for (int i = 1; i < d; ++i) {
        double s = 0.0;
        for (int m = 0; m < i; ++m) {
          const double l = A[i * ld + m];                          // a broadcast
          const double z = m == c ? zc : A[c * ld + m];
          if (m >= c) s = fma(l, z, s);
        }
        if (c < i) A[c * ld + i] = -s / A[i * ld + i];
      }
    }
    __syncthreads();
    double* P = q.prec + (size_t)k * d * d;
    for (int e = tid; e < d * d; e += kGmThreads) {
      const int i = e / d, j = e - i * d;
      P[e] = j > i ? A[i * ld + j] : (j == i ? 1.0 / A[i * ld + i] : 0.0);
    }
    if (tid < d) {
      double s = 0.0;
      for (int i = 0; i <= tid; ++i) s = fma(q.mu[(size_t)k * d + i], i == tid ? 1.0 / A[i * ld + i] : A[i * ld + tid], s);
      q.b[(size_t)k * d + tid] = s;
    }
    if (tid == 0) {
      double s = 0.0;
      for (int j = 0; j < d; ++j) s += log(1.0 / A[j * ld + j]);
      q.ld[k] = s;
    }
  } else {
    double* v = gm_smem;                                           // [d], then the mean and the flag
    for (int c = tid; c < d; c += kGmThreads) {
      double s = 0.0;
      for (int ch = 0; ch < chunks; ++ch) s += partial[((size_t)ch * K + k) * d + c];
      v[c] = s / nk + reg;
    }
    __syncthreads();
    if (tid == 0) {
      double bad = 0.0, mean = 0.0;
      for (int c = 0; c < d; ++c) mean += v[c];
      mean /= (double)d;
      if (TYPE == kGmSph) {
        if (!(mean > 0.0) || !(mean < INFINITY)) bad = 1.0;
      } else {
        for (int c = 0; c < d; ++c)
          if (!(v[c] > 0.0) || !(v[c] < INFINITY)) bad = 1.0;
      }
      v[d] = mean;
      v[d + 1] = bad;
    }
    __syncthreads();
    if (v[d + 1] != 0.0) {
      if (tid == 0) atomicMin(fail, k);
      return;
    }
    if (TYPE == kGmSph) {
      const double p = 1.0 / sqrt(v[d]);
      for (int c = tid; c < d; c += kGmThreads) q.b[(size_t)k * d + c] = q.mu[(size_t)k * d + c] * p;
      if (tid == 0) {
        q.cov[k] = v[d];
        q.prec[k] = p;
        q.ld[k] = (double)d * log(p);
      }
    } else {
      for (int c = tid; c < d; c += kGmThreads) {
        const double p = 1.0 / sqrt(v[c]);
        q.cov[(size_t)k * d + c] = v[c];
        q.prec[(size_t)k * d + c] = p;
        q.b[(size_t)k * d + c] = q.mu[(size_t)k * d + c] * p;
      }
      if (tid == 0) {
        double s = 0.0;
        for (int c = 0; c < d; ++c) s += log(1.0 / sqrt(v[c]));
        q.ld[k] = s;
      }
    }
  }
}

// b and log_det of given means and factors (an initialisation that brings its own): a block per component
__global__ __launch_bounds__(kGmThreads) void gmm_prepare_kernel(int d, int K, int type, double* params) {
  const int tid = threadIdx.x, k = blockIdx.x;
  const GmParams q = gm_params(params, d, K, type);
  const double* P = q.prec + (size_t)k * q.cs;
  for (int j = tid; j < d; j += kGmThreads) {
    double s;
    if (type == kGmFull) {
      s = 0.0;
      for (int i = 0; i <= j; ++i) s = fma(q.mu[(size_t)k * d + i], P[i * d + j], s);
    } else {
      s = q.mu[(size_t)k * d + j] * (type == kGmDiag ? P[j] : P[0]);
    }
    q.b[(size_t)k * d + j] = s;
  }
  if (tid == 0) {
    double s = 0.0;
    if (type == kGmSph) s = (double)d * log(P[0]);
    else
      for (int j = 0; j < d; ++j) s += log(type == kGmFull ? P[j * d + j] : P[j]);
    q.ld[k] = s;
  }
}

// ---------------------------------------------------------------- record
// Not ordered_total: contiguous slices per thread, then the 1024 partial sums in thread order -- another association, other bits.
__device__ __forceinline__ double gm_strip_total(const double* __restrict__ strip_sum, int strips, double* buf) {
  const int tid = threadIdx.x, S = (strips + kGmOneThreads - 1) / kGmOneThreads;
  double s = 0.0;
  for (int e = tid * S; e < min(strips, (tid + 1) * S); ++e) s += strip_sum[e];
  buf[tid] = s;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int e = 0; e < kGmOneThreads; ++e) t += buf[e];
    buf[0] = t;
  }
  __syncthreads();
  const double t = buf[0];
  __syncthreads();
  return t;
}

__device__ __forceinline__ void gm_weights(const GmParams& q, int K, double* buf) {
  const int tid = threadIdx.x;
  if (tid < K) buf[tid] = q.nk[tid];
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int k = 0; k < K; ++k) t += buf[k];
    buf[kGmMaxK] = t;
  }
  __syncthreads();
  if (tid < K) q.w[tid] = buf[tid] / buf[kGmMaxK];
  __syncthreads();
}

// advance != 0: the close of a step.  advance == 0: the close of an M-step alone (weights and the failure only).
__global__ __launch_bounds__(kGmOneThreads) void gmm_record_kernel(double* params, int d, int K, int type,
                                                                   const double* __restrict__ strip_sum, int strips, int N,
                                                                   double tol, const int* fail, int advance, double* state) {
  if (advance && step_done(state)) return;
  __shared__ double buf[kGmOneThreads];
  const GmParams q = gm_params(params, d, K, type);
  gm_weights(q, K, buf);
  const int f = *fail;
  const double failed = f == kNoIndex ? -1.0 : (double)f;
  if (!advance) {
    if (threadIdx.x == 0) {
      state[5] = failed;
      if (failed >= 0.0) state[1] = 1.0;
    }
    return;
  }
  const double lb = gm_strip_total(strip_sum, strips, buf) / (double)N;
  if (threadIdx.x == 0) {
    const double prev = state[0] == 0.0 ? -INFINITY : state[3];
    const bool conv = failed < 0.0 && fabs(lb - prev) < tol;
    state[0] += 1.0;
    state[1] = (conv || failed >= 0.0) ? 1.0 : 0.0;
    state[2] = conv ? 1.0 : 0.0;
    state[3] = lb;
    state[4] = prev;
    state[5] = failed;
    state[6] = 0.0;
    state[7] = 0.0;
  }
}

__global__ __launch_bounds__(kGmOneThreads) void gmm_mean_logp_kernel(const double* __restrict__ strip_sum, int strips, int N,
                                                                      double* __restrict__ out) {
  __shared__ double buf[kGmOneThreads];
  const double t = gm_strip_total(strip_sum, strips, buf);
  if (threadIdx.x == 0) out[0] = t / (double)N;
}

// ---------------------------------------------------------------- predict, sample
__global__ __launch_bounds__(kGmThreads) void gmm_argmax_kernel(const double* __restrict__ log_resp, int N, int K,
                                                                int* __restrict__ labels) {
  const int i = blockIdx.x * kGmThreads + threadIdx.x;
  if (i >= N) return;
  const double* lr = log_resp + (size_t)i * K;
  double bv = lr[0];
  int bk = 0;
  for (int k = 1; k < K; ++k)
    if (lr[k] > bv) {                                              // ascending k, ">": ties go to the lowest component
      bv = lr[k];
      bk = k;
    }
  labels[i] = bk;
}

// z_i = mu_c + L_c eps_i with L = (P^T)^-1, i.e. P^T v = eps by forward substitution: v_j = (eps_j - sum_{i<j} P[i,j] v_i) /
// P[j,j], i ascending (column j's running value takes -P[i,j] v_i as soon as v_i is known).  One wave per sample.
__global__ __launch_bounds__(64) void gmm_sample_kernel(double* params, int d, int K, int type, const int* __restrict__ comp,
                                                        const double* __restrict__ eps, int n, float* __restrict__ z) {
  __shared__ double vj;
  const int i = blockIdx.x, lane = threadIdx.x, c = comp[i];
  if ((unsigned)c >= (unsigned)K) {                                // the same in every thread
    for (int m = lane; m < d; m += 64) z[(size_t)i * d + m] = 0.f;
    return;
  }
  const GmParams q = gm_params(params, d, K, type);
  const double* mu = q.mu + (size_t)c * d;
  if (type != kGmFull) {
    const double* P = q.prec + (size_t)c * q.cs;
    for (int m = lane; m < d; m += 64)
      z[(size_t)i * d + m] = (float)(mu[m] + eps[(size_t)i * d + m] / (type == kGmDiag ? P[m] : P[0]));
    return;
  }
  const double* P = q.prec + (size_t)c * d * d;
  double acc0 = lane < d ? eps[(size_t)i * d + lane] : 0.0;
  double acc1 = lane + 64 < d ? eps[(size_t)i * d + lane + 64] : 0.0;
  for (int j = 0; j < d; ++j) {
    if (lane == (j & 63)) {
      const double v = (j < 64 ? acc0 : acc1) / P[(size_t)j * d + j];
      if (j < 64) acc0 = v; else acc1 = v;
      vj = v;
    }
    __syncthreads();
    const double v = vj;
    if (lane > j && lane < d) acc0 = fma(-P[(size_t)j * d + lane], v, acc0);
    if (lane + 64 > j && lane + 64 < d) acc1 = fma(-P[(size_t)j * d + lane + 64], v, acc1);
    __syncthreads();
  }
  if (lane < d) z[(size_t)i * d + lane] = (float)(mu[lane] + acc0);
  if (lane + 64 < d) z[(size_t)i * d + lane + 64] = (float)(mu[lane + 64] + acc1);
}

static_assert(kGmMaxDFull <= 128, "gmm_sample_kernel holds two columns per lane");

// ---------------------------------------------------------------- host side
struct GmLayout {
  size_t part1, part2, strip, fail, bytes;
};

static int gm_chunks(int N) { return (N + kGmChunk - 1) / kGmChunk; }
static int gm_strips(int N) { return (N + kGmStrip - 1) / kGmStrip; }
static int gm_entries(int d, int type) { return type == kGmFull ? d * (d + 1) / 2 : d; }

static GmLayout gm_layout(int N, int d, int K, int type) {
  GmLayout w;
  WsCursor ws;
  const size_t chunks = (size_t)gm_chunks(N);
  w.part1 = ws.take(chunks * K * (d + 1) * sizeof(double));
  w.part2 = ws.take(chunks * K * gm_entries(d, type) * sizeof(double));
  w.strip = ws.take((size_t)gm_strips(N) * sizeof(double));
  w.fail = ws.take(sizeof(int));
  w.bytes = ws.o;
  return w;
}

// Only a wide input needs more LDS than a launch gets unasked; then the most a workgroup may have, less what is static.
static int gm_lds_attr(const void* fn, size_t bytes, const char* what) {
  return bytes <= 32 * 1024 ? EVAE_OK : set_max_lds(fn, 160 * 1024 - 2048, what);
}

static int gm_estep_launch(const float* x, int N, int d, int K, int type, double* params, double* log_resp, double* logp,
                           char* ws, const GmLayout& w, const double* state, hipStream_t stream) {
  const int T = gm_estep_tile(d, type);
  const size_t lds = gm_estep_lds(d, type);
  double* strip = reinterpret_cast<double*>(ws + w.strip);
  const auto estep = type == kGmFull ? gmm_estep_kernel<kGmFull>
                                     : (type == kGmDiag ? gmm_estep_kernel<kGmDiag> : gmm_estep_kernel<kGmSph>);
  int rc = gm_lds_attr((const void*)estep, lds, "gmm_estep");
  if (rc) return rc;
  estep<<<gm_strips(N), kGmThreads, lds, stream>>>(x, N, d, K, params, T, log_resp, logp, strip, state);
  return check_launch("gmm_estep_kernel");
}

// pass 1, means, pass 2, finish: everything of the M-step but the weights
static int gm_mstep_launch(const float* x, int N, int d, int K, int type, const double* log_resp, const int* labels, double reg,
                           double* params, char* ws, const GmLayout& w, const double* state, hipStream_t stream) {
  const int chunks = gm_chunks(N);
  const GmParams q = gm_params(params, d, K, type);
  double* part1 = reinterpret_cast<double*>(ws + w.part1);
  double* part2 = reinterpret_cast<double*>(ws + w.part2);
  int* fail = reinterpret_cast<int*>(ws + w.fail);
  const dim3 grid(chunks, K);
  const auto finish = type == kGmFull ? gmm_finish_kernel<kGmFull>
                                      : (type == kGmDiag ? gmm_finish_kernel<kGmDiag> : gmm_finish_kernel<kGmSph>);
  gmm_wsum_kernel<0><<<grid, kGmThreads, 0, stream>>>(x, N, d, K, pow2_width(d + 1, kGmThreads), log_resp, labels, nullptr, part1, fail,
                                                      state);
  int rc = check_launch("gmm_wsum_kernel<0>");
  if (rc) return rc;
  gmm_means_kernel<<<(K * (d + 1) + kGmThreads - 1) / kGmThreads, kGmThreads, 0, stream>>>(part1, chunks, d, K, params, type, state);
  if ((rc = check_launch("gmm_means_kernel"))) return rc;
  if (type == kGmFull) {
    if ((rc = gm_lds_attr((const void*)gmm_scatter_kernel, gm_scatter_lds(d), "gmm_scatter"))) return rc;
    gmm_scatter_kernel<<<grid, kGmThreads, gm_scatter_lds(d), stream>>>(x, N, d, K, log_resp, labels, q.mu, part2, state);
    if ((rc = check_launch("gmm_scatter_kernel"))) return rc;
  } else {
    gmm_wsum_kernel<1><<<grid, kGmThreads, 0, stream>>>(x, N, d, K, pow2_width(d, kGmThreads), log_resp, labels, q.mu, part2, nullptr,
                                                        state);
    if ((rc = check_launch("gmm_wsum_kernel<1>"))) return rc;
  }
  // (only 'full' can be wide enough to ask for more LDS here: the others hold d + 2 doubles)
  if ((rc = gm_lds_attr((const void*)finish, gm_finish_lds(d, type), "gmm_finish"))) return rc;
  finish<<<K, kGmThreads, gm_finish_lds(d, type), stream>>>(part2, chunks, d, K, reg, params, fail, state);
  return check_launch("gmm_finish_kernel");
}

}  // namespace evae

using namespace evae;

extern "C" int evae_gmm_max_components(void) { return kGmMaxK; }
extern "C" int evae_gmm_max_features(int type) { return type == kGmFull ? kGmMaxDFull : kGmMaxD; }
extern "C" int evae_gmm_max_points(void) { return kGmMaxN; }
extern "C" int evae_gmm_chunk_rows(void) { return kGmChunk; }
extern "C" int evae_gmm_strip_rows(void) { return kGmStrip; }
extern "C" size_t evae_gmm_max_bytes(void) { return kGmMaxBytes; }

extern "C" size_t evae_gmm_params_doubles(int d, int K, int type) {
  if (d < 1 || K < 1 || type < kGmFull || type > kGmSph) return 0;
  return gm_params_doubles(d, K, type);
}

extern "C" size_t evae_gmm_workspace_bytes(int N, int d, int K, int type) {
  if (N < 1 || d < 1 || K < 1 || type < kGmFull || type > kGmSph) return 0;
  return gm_layout(N, d, K, type).bytes;
}

#define GM_SHAPE(who)                                                                                                  \
  EVAE_REQUIRE(type >= kGmFull && type <= kGmSph, who ": covariance type %d outside 0 (full), 1 (diag), 2 (spherical)", type); \
  EVAE_REQUIRE(d >= 1 && d <= evae_gmm_max_features(type), who ": d=%d outside [1, %d] for this covariance type", d,   \
               evae_gmm_max_features(type));                                                                           \
  EVAE_REQUIRE(K >= 1 && K <= kGmMaxK, who ": K=%d outside [1, %d]", K, kGmMaxK)

#define GM_SIZES(who)                                                                                                  \
  GM_SHAPE(who);                                                                                                       \
  EVAE_REQUIRE(N >= 1 && N <= kGmMaxN, who ": N=%d outside [1, %d]", N, kGmMaxN);                                      \
  EVAE_REQUIRE((size_t)N * K * sizeof(double) + evae_gmm_workspace_bytes(N, d, K, type) <= kGmMaxBytes,                \
               who ": log_resp of %zu bytes plus a workspace of %zu bytes for N=%d, d=%d, K=%d exceed %zu bytes",      \
               (size_t)N * K * sizeof(double), evae_gmm_workspace_bytes(N, d, K, type), N, d, K, kGmMaxBytes);         \
  EVAE_REQUIRE(ws && ((uintptr_t)ws & 255) == 0, who ": null or misaligned workspace");                                \
  EVAE_REQUIRE(ws_bytes >= evae_gmm_workspace_bytes(N, d, K, type), who ": workspace of %zu bytes, %zu needed", ws_bytes, \
               evae_gmm_workspace_bytes(N, d, K, type))

extern "C" int evae_gmm_estep(const float* x, int N, int d, int K, int type, const double* params, double* log_resp, double* logp,
                              double* mean_logp, void* ws, size_t ws_bytes, evae_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GM_SIZES("gmm_estep");
  EVAE_REQUIRE(x && params && log_resp && logp && mean_logp, "gmm_estep: null pointer");
  EVAE_REQUIRE(aligned8(params) && aligned8(log_resp) && aligned8(logp) && aligned8(mean_logp),
               "gmm_estep: misaligned pointer");
  const GmLayout w = gm_layout(N, d, K, type);
  char* base = static_cast<char*>(ws);
  int rc = gm_estep_launch(x, N, d, K, type, const_cast<double*>(params), log_resp, logp, base, w, nullptr, stream);
  if (rc) return rc;
  gmm_mean_logp_kernel<<<1, kGmOneThreads, 0, stream>>>(reinterpret_cast<const double*>(base + w.strip), gm_strips(N), N, mean_logp);
  return check_launch("gmm_mean_logp_kernel");
}

extern "C" int evae_gmm_mstep(const float* x, int N, int d, int K, int type, const double* log_resp, const int* labels,
                              double reg_covar, double* params, double* state, void* ws, size_t ws_bytes, evae_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GM_SIZES("gmm_mstep");
  EVAE_REQUIRE(x && params && state, "gmm_mstep: null pointer");
  EVAE_REQUIRE((log_resp != nullptr) != (labels != nullptr), "gmm_mstep: exactly one of log_resp and labels expected");
  EVAE_REQUIRE(aligned8(params) && aligned8(log_resp) && aligned8(state), "gmm_mstep: misaligned pointer");
  EVAE_REQUIRE(reg_covar >= 0.0, "gmm_mstep: reg_covar=%g", reg_covar);
  const GmLayout w = gm_layout(N, d, K, type);
  char* base = static_cast<char*>(ws);
  int rc = gm_mstep_launch(x, N, d, K, type, log_resp, labels, reg_covar, params, base, w, nullptr, stream);
  if (rc) return rc;
  gmm_record_kernel<<<1, kGmOneThreads, 0, stream>>>(params, d, K, type, nullptr, 0, N, 0.0, reinterpret_cast<const int*>(base + w.fail),
                                                     0, state);
  return check_launch("gmm_record_kernel");
}

extern "C" int evae_gmm_step(const float* x, int N, int d, int K, int type, double* params, double* log_resp, double* logp,
                             double reg_covar, double tol, double* state, void* ws, size_t ws_bytes, evae_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GM_SIZES("gmm_step");
  EVAE_REQUIRE(x && params && log_resp && logp && state, "gmm_step: null pointer");
  EVAE_REQUIRE(aligned8(params) && aligned8(log_resp) && aligned8(logp) && aligned8(state), "gmm_step: misaligned pointer");
  EVAE_REQUIRE(reg_covar >= 0.0 && tol >= 0.0, "gmm_step: reg_covar=%g, tol=%g", reg_covar, tol);
  const GmLayout w = gm_layout(N, d, K, type);
  char* base = static_cast<char*>(ws);
  int rc = gm_estep_launch(x, N, d, K, type, params, log_resp, logp, base, w, state, stream);
  if (rc) return rc;
  if ((rc = gm_mstep_launch(x, N, d, K, type, log_resp, nullptr, reg_covar, params, base, w, state, stream))) return rc;
  gmm_record_kernel<<<1, kGmOneThreads, 0, stream>>>(params, d, K, type, reinterpret_cast<const double*>(base + w.strip), gm_strips(N),
                                                     N, tol, reinterpret_cast<const int*>(base + w.fail), 1, state);
  return check_launch("gmm_record_kernel");
}

extern "C" int evae_gmm_prepare(double* params, int d, int K, int type, evae_stream_t stream_) {
  GM_SHAPE("gmm_prepare");
  EVAE_REQUIRE(params && aligned8(params), "gmm_prepare: null or misaligned params");
  gmm_prepare_kernel<<<K, kGmThreads, 0, (hipStream_t)stream_>>>(d, K, type, params);
  return check_launch("gmm_prepare_kernel");
}

extern "C" int evae_gmm_argmax(const double* log_resp, int N, int K, int* labels, evae_stream_t stream_) {
  EVAE_REQUIRE(N >= 1 && N <= kGmMaxN, "gmm_argmax: N=%d outside [1, %d]", N, kGmMaxN);
  EVAE_REQUIRE(K >= 1 && K <= kGmMaxK, "gmm_argmax: K=%d outside [1, %d]", K, kGmMaxK);
  EVAE_REQUIRE(log_resp && labels && aligned8(log_resp), "gmm_argmax: null or misaligned pointer");
  gmm_argmax_kernel<<<(N + kGmThreads - 1) / kGmThreads, kGmThreads, 0, (hipStream_t)stream_>>>(log_resp, N, K, labels);
  return check_launch("gmm_argmax_kernel");
}

extern "C" int evae_gmm_sample(const double* params, int d, int K, int type, const int* comp, const double* eps, int n, float* z,
                               evae_stream_t stream_) {
  GM_SHAPE("gmm_sample");
  EVAE_REQUIRE(n >= 1 && n <= kGmMaxN, "gmm_sample: n=%d outside [1, %d]", n, kGmMaxN);
  EVAE_REQUIRE(params && comp && eps && z, "gmm_sample: null pointer");
  EVAE_REQUIRE(aligned8(params) && aligned8(eps), "gmm_sample: misaligned params or eps");
  gmm_sample_kernel<<<n, 64, 0, (hipStream_t)stream_>>>(const_cast<double*>(params), d, K, type, comp, eps, n, z);
  return check_launch("gmm_sample_kernel");
}
