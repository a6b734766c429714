// Linear probe of the latent space on gfx950: multinomial (softmax) regression with an L2 penalty by L-BFGS, all arithmetic in
// fp64 on fp32 rows (evae/linear.py; DESIGN 3.7i has the formulas, the order of every sum and the measurements).  No
// floating-point atomic; the one atomic is the integer ticket by which the last workgroup of the line launch learns that it is
// the last.  Every floating-point sum has a fixed order, so equal inputs give bit-equal outputs.  Plain fp64 fma throughout, no
// matrix instruction.
//
//   a_n = (x_n, 1), p = d + 1 (p = d without an intercept), L = K p, lambda = 1 / C:
//   f(W) = sum_n [ lse_k(a_n . w_k) - a_n . w_{y_n} ] + (lambda / 2) sum_k sum_{c<d} W_kc^2
//
//   solver:  one fp64 buffer: G [L] | Q [L] | D [L] | S [m x L] | Y [m x L] | sy [m] | yy [m] | alpha [m] | scal [8]
//            (scal: pairs held, next slot, max|G| / N, ww).  Q is the work vector of the finish.
//   record:  [8] = iterations, done, converged, f, t, j, line search failed, G.D
//   logits:  a block owns kLrStrip rows, staged in LDS as fp32 with an odd row stride; W passes through LDS in tiles of kLrTile
//            rows.  Thread (row, group g) owns the classes t0 + g, t0 + g + 4, ..: fma over the features in index order, the
//            intercept last.  A row's bits depend on the row and on W alone.
//   line:    block (chunk of kLrChunk rows, trial j).  Thread tid adds the losses of the rows tid, tid + 256, .. of the chunk in
//            that order; the 256 thread sums by chunk_sum_store (the waves' butterflies, then the four waves); [chunks x T].  The
//            workgroup that draws the last ticket adds the chunks in chunk order, the penalty (lambda / 2)(ww + 2 t wd + t^2 dd)
//            from three ordered dots, takes the first j with f_j <= f + c1 t_j G.D, writes the record and the ring and applies
//            W += t D.  No j: the record's line-search flag and done; W stays.
//   grad:    a block of 1024 per chunk, the only one to touch the chunk's rows of Z and Z_D.  Phase 1, a thread per row: Z += t
//            Z_D (t of the record; 0: nothing is read from Z_D), m = max_k, s = sum_k exp(z_k - m) in class order, R = exp / s
//            - onehot INTO Z_D, the row's loss (m + log s) - z_y; the chunk's loss (the waves' butterflies, the 16 waves in
//            order).  Phase 2: sub-tiles of up to 128 rows (what fits 96 KiB), R and the rows as fp64 in LDS; thread (column c,
//            group g) owns the classes k0 + g, k0 + g + G, .. (up to 4) of column c and adds R_nk a_nc over the chunk's rows in
//            index order; [chunks x K x p].
//   finish:  ONE workgroup: the chunks in chunk order + lambda W on the penalised columns = the new G; the pair (s, y) = (t D,
//            G_new - G) with s.y and y.y (kept when s.y > 0); f; max|G| / N against tol; the two-loop recursion for the next D
//            and G.D.  The vectors stay in global memory: a thread keeps to the entries tid, tid + 256, .. from start to end.
//   Every launch of a step starts with `if (state[1] != 0) return` -- the same value in every thread of the grid, written by an
//   EARLIER launch of the stream (the line launch writes it after every other workgroup has drawn its ticket, so after every
//   read).  Nothing polls, nothing waits on another workgroup.  A step is four launches.
#include <float.h>

#include "evae_latent.h"

namespace evae {

constexpr int kLrMaxK = 256;
constexpr int kLrMaxD = 256;
constexpr int kLrMaxN = 1 << 20;
constexpr int kLrMaxHistory = 64;
constexpr int kLrMaxLine = 32;
constexpr int kLrChunk = 1024;
constexpr int kLrStrip = 64;                                 // rows of a logits block: one wave of rows
constexpr int kLrTile = 16;                                  // rows of W in LDS at a time
constexpr int kLrThreads = 256;
constexpr int kLrGroups = kLrThreads / kLrStrip;             // 4
constexpr int kLrPer = kLrTile / kLrGroups;                  // 4 classes per thread and tile
constexpr int kLrGradThreads = 1024;                         // the gradient's block: a thread per row of a chunk
constexpr int kLrMaxSub = 128;                               // rows of a gradient sub-tile at most
constexpr size_t kLrGradLds = 96 * 1024;                     // what a sub-tile may take of a CU's 160 KiB
constexpr int kLrAcc = 4;                                    // classes per thread in the gradient
constexpr int kLrTotalTile = 64;                             // chunks whose trial sums the line launch's last block stages at once
static_assert(kLrGradThreads == kLrChunk, "logreg_grad_kernel: a thread per row of a chunk");
constexpr size_t kLrMaxBytes = (size_t)1 << 30;
constexpr double kLrC1 = 1e-4;
enum { kLrIter = 0, kLrDone = 1, kLrConv = 2, kLrLoss = 3, kLrT = 4, kLrJ = 5, kLrLineFail = 6, kLrGD = 7 };
enum { kLrCount = 0, kLrHead = 1, kLrGnorm = 2, kLrWW = 3 };

struct LrSolver {
  double *G, *Q, *D, *S, *Y, *sy, *yy, *alpha, *scal;
};

__host__ __device__ inline size_t lr_solver_doubles(int L, int m) { return (size_t)L * (3 + 2 * (size_t)m) + 3 * (size_t)m + 8; }
__host__ __device__ inline LrSolver lr_solver(double* s, int L, int m) {
  LrSolver q;
  q.G = s;
  q.Q = s + L;
  q.D = s + 2 * (size_t)L;
  q.S = s + 3 * (size_t)L;
  q.Y = q.S + (size_t)m * L;
  q.sy = q.Y + (size_t)m * L;
  q.yy = q.sy + m;
  q.alpha = q.yy + m;
  q.scal = q.alpha + m;
  return q;
}

// ---------------------------------------------------------------- block reductions of the one-workgroup parts (256 threads)
// Thread tid brings s, its sum over the entries tid, tid + 256, .. in that order: the 64 lane sums by the wave's butterfly, the
// four waves as ((w0 + w1) + w2) + w3; every thread gets the total.  red: [5].  Closes with a barrier.
__device__ __forceinline__ double lr_block_sum(double s, double* red) {
  const int tid = threadIdx.x;
  s = wave_sum(s);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) red[4] = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  const double t = red[4];
  __syncthreads();
  return t;
}

__device__ __forceinline__ double lr_dot(const double* a, const double* b, int L, double* red) {
  double s = 0.0;
  for (int e = threadIdx.x; e < L; e += kLrThreads) s = fma(a[e], b[e], s);
  return lr_block_sum(s, red);
}

// the same over the penalised columns (c < d) of two [K x p] arrays
__device__ __forceinline__ double lr_pen_dot(const double* a, const double* b, int L, int p, int d, double* red) {
  double s = 0.0;
  for (int e = threadIdx.x; e < L; e += kLrThreads)
    if (e % p < d) s = fma(a[e], b[e], s);
  return lr_block_sum(s, red);
}

// ---------------------------------------------------------------- logits
static size_t lr_logits_lds(int d, int p) { return (size_t)kLrTile * p * sizeof(double) + (size_t)kLrStrip * (d | 1) * sizeof(float); }

__global__ __launch_bounds__(kLrThreads) void logreg_logits_kernel(const float* __restrict__ x, int N, int d,
                                                                   const double* __restrict__ W, int K, int p,
                                                                   double* __restrict__ out, const double* state) {
  if (step_done(state)) return;
  extern __shared__ __attribute__((aligned(16))) double lr_smem[];
  double* wt = lr_smem;                                            // [kLrTile x p]
  float* xr = reinterpret_cast<float*>(wt + (size_t)kLrTile * p);  // [kLrStrip x ldx]
  const int tid = threadIdx.x, r = tid & (kLrStrip - 1), g = tid / kLrStrip;
  const int r0 = blockIdx.x * kLrStrip, rows = min(kLrStrip, N - r0), ldx = d | 1;
  for (int e = tid; e < kLrStrip * d; e += kLrThreads) {
    const int rr = e / d, c = e - rr * d;
    xr[rr * ldx + c] = rr < rows ? x[(size_t)r0 * d + e] : 0.f;
  }
  const float* xrow = xr + r * ldx;
  for (int t0 = 0; t0 < K; t0 += kLrTile) {
    __syncthreads();                                               // the rows are staged; the last tile has been read
    const int tn = min(kLrTile, K - t0);
    for (int e = tid; e < tn * p; e += kLrThreads) wt[e] = W[(size_t)t0 * p + e];
    __syncthreads();
    double acc[kLrPer];
    const double* wk[kLrPer];
#pragma unroll
    for (int u = 0; u < kLrPer; ++u) {
      acc[u] = 0.0;
      wk[u] = wt + (size_t)min(g + u * kLrGroups, tn - 1) * p;     // a slot past the tile reads a live row and is not stored
    }
    for (int c = 0; c < d; ++c) {
      const double xv = (double)xrow[c];
#pragma unroll
      for (int u = 0; u < kLrPer; ++u) acc[u] = fma(xv, wk[u][c], acc[u]);
    }
    if (p > d) {
#pragma unroll
      for (int u = 0; u < kLrPer; ++u) acc[u] += wk[u][d];
    }
    if (r < rows) {
#pragma unroll
      for (int u = 0; u < kLrPer; ++u)
        if (g + u * kLrGroups < tn) out[(size_t)(r0 + r) * K + t0 + g + u * kLrGroups] = acc[u];
    }
  }
}

// ---------------------------------------------------------------- line search
__global__ __launch_bounds__(kLrThreads) void logreg_line_kernel(const double* __restrict__ Z, const double* __restrict__ ZD,
                                                                 const int* __restrict__ y, int N, int K, int p, int d,
                                                                 double* W, const double* D, double lambda, int T,
                                                                 double* __restrict__ part, unsigned* ticket, double* state,
                                                                 int* __restrict__ ring, int ring_len) {
  if (step_done(state)) return;
  __shared__ double tile[kLrTotalTile * kLrMaxLine];               // the last block's: chunk sums on their way to the totals
  __shared__ double buf[kLrMaxLine];                               // the trial losses
  __shared__ double red[5];
  const int tid = threadIdx.x;
  const int chunks = gridDim.x, c0 = blockIdx.x * kLrChunk, n = min(kLrChunk, N - c0);
  {
    const int j = blockIdx.y;                                      // < T: the grid is (chunks, T)
    const double t = ldexp(1.0, -j);
    double s = 0.0;
    for (int r = tid; r < n; r += kLrThreads) {
      const int row = c0 + r, yr = y[row];
      const double* __restrict__ z = Z + (size_t)row * K;
      const double* __restrict__ zd = ZD + (size_t)row * K;
      double mx = -INFINITY;
      for (int k = 0; k < K; ++k) mx = fmax(mx, fma(t, zd[k], z[k]));
      double se = 0.0;
      for (int k = 0; k < K; ++k) se += exp(fma(t, zd[k], z[k]) - mx);
      const double zy = (unsigned)yr < (unsigned)K ? fma(t, zd[yr], z[yr]) : 0.0;
      s += (mx + log(se)) - zy;
    }
    chunk_sum_store(s, red, part + (size_t)blockIdx.x * T + j);
  }
  // the ticket: every wave's stores have left, the block's release at agent scope, then one relaxed add
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned old = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = old == gridDim.x * gridDim.y - 1;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the next line launch of the stream
    }
    red[0] = last ? 1.0 : 0.0;
  }
  __syncthreads();
  const bool last = red[0] != 0.0;
  __syncthreads();
  if (!last) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");               // every wave of the reader reads the others' sums afresh

  double mine = 0.0;                                               // thread jj < T: the total of trial jj, the chunks in chunk order
  for (int h0 = 0; h0 < chunks; h0 += kLrTotalTile) {              // (kLrTotalTile chunks of sums through LDS at a time)
    const int m = min(kLrTotalTile, chunks - h0);
    for (int e = tid; e < m * T; e += kLrThreads) tile[e] = part[(size_t)h0 * T + e];
    __syncthreads();
    if (tid < T)
      for (int e = 0; e < m; ++e) mine += tile[e * T + tid];
    __syncthreads();
  }
  const int L = K * p;
  const double ww = lr_pen_dot(W, W, L, p, d, red);
  const double wd = lr_pen_dot(W, D, L, p, d, red);
  const double dd = lr_pen_dot(D, D, L, p, d, red);
  if (tid < T) {
    const double t = ldexp(1.0, -tid);
    buf[tid] = mine + (0.5 * lambda) * ((ww + (2.0 * t) * wd) + (t * t) * dd);
  }
  __syncthreads();
  if (tid == 0) {
    const double f = state[kLrLoss], gd = state[kLrGD];
    int pick = -1;
    for (int jj = 0; jj < T && pick < 0; ++jj) {
      const double t = ldexp(1.0, -jj);
      if (buf[jj] <= f + (kLrC1 * t) * gd) pick = jj;
    }
    red[1] = (double)pick;
    const int it = (int)state[kLrIter];
    if (pick >= 0) {
      state[kLrT] = ldexp(1.0, -pick);
      state[kLrJ] = (double)pick;
      if (ring && it >= 0 && it < ring_len) ring[it] = pick;
    } else {
      state[kLrT] = 0.0;
      state[kLrJ] = -1.0;
      state[kLrLineFail] = 1.0;
      state[kLrConv] = 0.0;
      state[kLrDone] = 1.0;
    }
  }
  __syncthreads();
  const int pick = (int)red[1];
  if (pick < 0) return;
  const double t = ldexp(1.0, -pick);
  for (int e = tid; e < L; e += kLrThreads) W[e] = fma(t, D[e], W[e]);
}

// ---------------------------------------------------------------- gradient
static int lr_grad_width(int p) { return pow2_width(p, 256); }
static int lr_grad_tile(int p, int K) {                           // classes of a tile
  const int t = kLrAcc * (kLrGradThreads / lr_grad_width(p));
  return t < K ? t : K;
}
static int lr_grad_sub(int p, int K) {                            // rows of a sub-tile: a power of two, what fits kLrGradLds
  const size_t row = ((size_t)lr_grad_width(p) + lr_grad_tile(p, K)) * sizeof(double);
  int s = kLrMaxSub;
  while (s > 8 && (size_t)s * row > kLrGradLds) s >>= 1;
  return s;
}
static size_t lr_grad_lds(int p, int K) {
  return (size_t)lr_grad_sub(p, K) * ((size_t)lr_grad_width(p) + lr_grad_tile(p, K)) * sizeof(double);
}

__global__ __launch_bounds__(kLrGradThreads) void logreg_grad_kernel(const float* __restrict__ x, const int* __restrict__ y, int N,
                                                                     int d, int K, int p, int Wd, int TK, int SUB, double* Z,
                                                                     double* ZD, double* __restrict__ partial,
                                                                     double* __restrict__ chunk_loss, const double* state) {
  if (step_done(state)) return;
  extern __shared__ __attribute__((aligned(16))) double lr_smem[];
  __shared__ double wpart[kLrGradThreads / 64];
  double* at = lr_smem;                                            // [SUB x Wd]
  double* rt = at + (size_t)SUB * Wd;                              // [SUB x TK]
  const int tid = threadIdx.x, c0 = blockIdx.x * kLrChunk, n = min(kLrChunk, N - c0);
  const double t = state[kLrT];
  // phase 1: a thread per row (kLrGradThreads == kLrChunk)
  double ls = 0.0;
  if (tid < n) {
    const int row = c0 + tid, yr = y[row];
    double* __restrict__ z = Z + (size_t)row * K;
    double* __restrict__ zd = ZD + (size_t)row * K;
    double mx = -INFINITY;
    if (t != 0.0) {
#pragma unroll 4
      for (int k = 0; k < K; ++k) {
        const double v = fma(t, zd[k], z[k]);
        z[k] = v;
        mx = fmax(mx, v);
      }
    } else {
#pragma unroll 4
      for (int k = 0; k < K; ++k) mx = fmax(mx, z[k]);
    }
    double se = 0.0;
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
      const double e = exp(z[k] - mx);
      zd[k] = e;
      se += e;
    }
    for (int k = 0; k < K; ++k) zd[k] = zd[k] / se - (k == yr ? 1.0 : 0.0);
    ls = (mx + log(se)) - ((unsigned)yr < (unsigned)K ? z[yr] : 0.0);
  }
  ls = wave_sum(ls);                                               // the chunk's loss: the waves' butterflies, then the 16 waves in order
  if ((tid & 63) == 0) wpart[tid >> 6] = ls;
  __syncthreads();                                                 // also: the block's own R, read back below
  if (tid == 0) {
    double s = 0.0;
    for (int h = 0; h < kLrGradThreads / 64; ++h) s += wpart[h];
    chunk_loss[blockIdx.x] = s;
  }
  // phase 2: thread (column c, group g)
  const int wshift = __ffs(Wd) - 1;                                // Wd is a power of two
  const int c = tid & (Wd - 1), g = tid >> wshift, G = kLrGradThreads >> wshift;
  // p = 257 > Wd (d = 256 with an intercept): the column of ones does not go through the tiles a second time; its sum is
  // sum_n R_nk, added in the same row order by the first wave of every group (fma(r, 1, acc) == acc + r: the same bits)
  const bool ones_apart = p > Wd;
  const int pc = ones_apart ? d : p;
  const bool ones_wave = ones_apart && c < 64;
  // a thread's entries tid, tid + threads, .. of the [SUB x TK] tile of R as (row, class): stepped, not divided, in the loop
  const int rstep = kLrGradThreads / TK, kstep = kLrGradThreads - rstep * TK;
  const int rr0 = tid / TK, kk0 = tid - rr0 * TK;
  for (int k0 = 0; k0 < K; k0 += TK) {
    const int tn = min(TK, K - k0);
    for (int cb = 0; cb < pc; cb += Wd) {
      const int cc = cb + c;
      double acc[kLrAcc], one[kLrAcc];
#pragma unroll
      for (int u = 0; u < kLrAcc; ++u) acc[u] = one[u] = 0.0;
      for (int s0 = 0; s0 < n; s0 += SUB) {
        const int sn = min(SUB, n - s0);
        __syncthreads();                                           // the last sub-tile has been read
        // every load goes to a clamped, live address and is chosen or dropped afterwards: no load waits behind a branch
#pragma unroll 4
        for (int e = tid; e < SUB * Wd; e += kLrGradThreads) {
          const int rr = e >> wshift, col = cb + (e & (Wd - 1));
          const float xv = x[(size_t)(c0 + s0 + min(rr, sn - 1)) * d + min(col, d - 1)];
          at[e] = (rr < sn && col < pc) ? (col < d ? (double)xv : 1.0) : 0.0;
        }
        int er = rr0, ek = kk0;                                    // e == er * TK + ek
#pragma unroll 4
        for (int e = tid; e < SUB * TK; e += kLrGradThreads) {
          const double rv = ZD[(size_t)(c0 + s0 + min(er, sn - 1)) * K + k0 + min(ek, tn - 1)];
          rt[e] = (er < sn && ek < tn) ? rv : 0.0;
          er += rstep;
          ek += kstep;
          if (ek >= TK) {
            ek -= TK;
            ++er;
          }
        }
        __syncthreads();
        if (cc < pc) {
          for (int rr = 0; rr < sn; ++rr) {
            const double a = at[rr * Wd + c];
            const double* rrow = rt + rr * TK;
#pragma unroll
            for (int u = 0; u < kLrAcc; ++u) {
              const int kk = g + u * G;
              if (kk < TK) acc[u] = fma(rrow[kk], a, acc[u]);
            }
          }
        }
        if (ones_wave) {
          for (int rr = 0; rr < sn; ++rr) {
            const double* rrow = rt + rr * TK;
#pragma unroll
            for (int u = 0; u < kLrAcc; ++u) {
              const int kk = g + u * G;
              if (kk < TK) one[u] += rrow[kk];
            }
          }
        }
      }
#pragma unroll
      for (int u = 0; u < kLrAcc; ++u) {
        const int kk = g + u * G;
        if (kk < tn) {
          double* out = partial + ((size_t)blockIdx.x * K + k0 + kk) * p;
          if (cc < pc) out[cc] = acc[u];
          if (ones_apart && c == 0) out[d] = one[u];
        }
      }
    }
  }
}

// ---------------------------------------------------------------- finish: G, the pair, the stop, the next direction
// The two-loop recursion on Q (= G on entry) -> D = -H G and G.D into the record.  Thread tid keeps to the entries tid, tid +
// 256, .. of every vector; each dot is lr_dot's fixed order.
__device__ __forceinline__ void lr_direction(const LrSolver& q, int L, int m, double gmax, double* state, double* red) {
  const int tid = threadIdx.x;
  const int count = (int)q.scal[kLrCount], head = (int)q.scal[kLrHead];
  for (int i = 0; i < count; ++i) {                                // newest first
    const int slot = (head - 1 - i + 2 * m) % m;
    const double a = lr_dot(q.S + (size_t)slot * L, q.Q, L, red) / q.sy[slot];
    if (tid == 0) q.alpha[slot] = a;
    const double* yv = q.Y + (size_t)slot * L;
    for (int e = tid; e < L; e += kLrThreads) q.Q[e] = fma(-a, yv[e], q.Q[e]);
  }
  __syncthreads();                                                 // alpha, written by thread 0
  double gamma = 1.0 / gmax;
  if (count > 0) {
    const int slot = (head - 1 + m) % m;
    gamma = q.sy[slot] / q.yy[slot];
  }
  for (int e = tid; e < L; e += kLrThreads) q.Q[e] *= gamma;
  for (int i = count - 1; i >= 0; --i) {                           // oldest first
    const int slot = (head - 1 - i + 2 * m) % m;
    const double b = lr_dot(q.Y + (size_t)slot * L, q.Q, L, red) / q.sy[slot];
    const double ab = q.alpha[slot] - b;
    const double* sv = q.S + (size_t)slot * L;
    for (int e = tid; e < L; e += kLrThreads) q.Q[e] = fma(ab, sv[e], q.Q[e]);
  }
  for (int e = tid; e < L; e += kLrThreads) q.D[e] = -q.Q[e];
  const double gd = lr_dot(q.G, q.D, L, red);
  if (tid == 0) state[kLrGD] = gd;
}

__device__ __forceinline__ double lr_abs_max(const double* g, int L, double* red) {
  const int tid = threadIdx.x;
  double mx = 0.0;
  for (int e = tid; e < L; e += kLrThreads) {
    const double a = fabs(g[e]);
    mx = (a > mx || a != a) ? a : mx;                              // a NaN stays
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double other = __shfl_xor(mx, o, 64);
    mx = (other > mx || other != other) ? other : mx;
  }
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  if (tid == 0) {
    double t = red[0];
    for (int h = 1; h < 4; ++h) t = (red[h] > t || red[h] != red[h]) ? red[h] : t;
    red[4] = t;
  }
  __syncthreads();
  const double t = red[4];
  __syncthreads();
  return t;
}

__global__ __launch_bounds__(kLrThreads) void logreg_finish_kernel(const double* __restrict__ partial,
                                                                   const double* __restrict__ chunk_loss, int chunks, int N, int K,
                                                                   int p, int d, const double* W, double* solver, int m,
                                                                   double lambda, double tol, double* state) {
  if (step_done(state)) return;
  __shared__ double buf[kLrThreads];
  __shared__ double red[5];
  const int tid = threadIdx.x, L = K * p;
  const LrSolver q = lr_solver(solver, L, m);
  const double t = state[kLrT];
  const bool stepped = t != 0.0;
  double sy = 0.0, yy = 0.0;
  for (int e = tid; e < L; e += kLrThreads) {
    double s = 0.0;
#pragma unroll 8
    for (int ch = 0; ch < chunks; ++ch) s += partial[(size_t)ch * L + e];
    const double g = (e % p < d) ? fma(lambda, W[e], s) : s;
    q.Q[e] = g;
    if (stepped) {
      const double yv = g - q.G[e];
      sy = fma(t * q.D[e], yv, sy);
      yy = fma(yv, yv, yy);
    }
  }
  if (stepped) {                                                   // the same in every thread
    sy = lr_block_sum(sy, red);
    yy = lr_block_sum(yy, red);
    if (sy > 0.0) {
      const int head = (int)q.scal[kLrHead], count = (int)q.scal[kLrCount];
      double* sv = q.S + (size_t)head * L;
      double* yv = q.Y + (size_t)head * L;
      for (int e = tid; e < L; e += kLrThreads) {
        sv[e] = t * q.D[e];
        yv[e] = q.Q[e] - q.G[e];
      }
      __syncthreads();                                             // scal has been read by everybody
      if (tid == 0) {
        q.sy[head] = sy;
        q.yy[head] = yy;
        q.scal[kLrHead] = (double)((head + 1) % m);
        q.scal[kLrCount] = (double)min(count + 1, m);
      }
    }
  }
  for (int e = tid; e < L; e += kLrThreads) q.G[e] = q.Q[e];
  __syncthreads();                                                 // sy, yy, scal of thread 0; G
  const double gmax = lr_abs_max(q.G, L, red);
  const double ww = lr_pen_dot(W, W, L, p, d, red);
  const double data = ordered_total<kLrThreads>(chunk_loss, chunks, buf);   // thread 0's alone
  const double gn = gmax / (double)N;
  const bool conv = gn <= tol;
  if (tid == 0) {
    state[kLrLoss] = data + (0.5 * lambda) * ww;
    if (stepped) state[kLrIter] += 1.0;
    state[kLrConv] = conv ? 1.0 : 0.0;
    q.scal[kLrGnorm] = gn;
    q.scal[kLrWW] = ww;
  }
  if (!(gn > tol)) {                                               // converged, or not a number: no direction from this G
    if (tid == 0) state[kLrDone] = 1.0;
    return;
  }
  lr_direction(q, L, m, gmax, state, red);
}

// the two-loop recursion alone: D and G.D from the G and the pairs already in the solver
__global__ __launch_bounds__(kLrThreads) void logreg_direction_kernel(double* solver, int L, int m, double* state) {
  __shared__ double red[5];
  const LrSolver q = lr_solver(solver, L, m);
  for (int e = threadIdx.x; e < L; e += kLrThreads) q.Q[e] = q.G[e];
  const double gmax = lr_abs_max(q.G, L, red);
  lr_direction(q, L, m, gmax, state, red);
}

// ---------------------------------------------------------------- log-probabilities and labels
__global__ __launch_bounds__(kLrThreads) void logreg_softmax_kernel(const double* __restrict__ Z, int N, int K,
                                                                    double* __restrict__ logp, int* __restrict__ labels) {
  const int i = blockIdx.x * kLrThreads + threadIdx.x;
  if (i >= N) return;
  const double* z = Z + (size_t)i * K;
  double bv = z[0];
  int bk = 0;
  for (int k = 1; k < K; ++k)
    if (z[k] > bv) {                                               // ascending k, ">": ties go to the lowest class
      bv = z[k];
      bk = k;
    }
  double se = 0.0;
  for (int k = 0; k < K; ++k) se += exp(z[k] - bv);
  const double ls = log(se);
  if (logp)
    for (int k = 0; k < K; ++k) logp[(size_t)i * K + k] = (z[k] - bv) - ls;
  if (labels) labels[i] = bk;
}

// ---------------------------------------------------------------- host side
struct LrLayout {
  size_t part, loss, line, ticket, bytes;
};

static int lr_chunks(int N) { return (N + kLrChunk - 1) / kLrChunk; }

static LrLayout lr_layout(int N, int L, int T) {
  LrLayout w;
  WsCursor ws;
  const size_t chunks = (size_t)lr_chunks(N);
  w.part = ws.take(chunks * L * sizeof(double));
  w.loss = ws.take(chunks * sizeof(double));
  w.line = ws.take(chunks * T * sizeof(double));
  w.ticket = ws.take(sizeof(unsigned));
  w.bytes = ws.o;
  return w;
}

static int lr_lds_attr(const void* fn, size_t bytes, const char* what) {
  return bytes <= 32 * 1024 ? EVAE_OK : set_max_lds(fn, 160 * 1024 - 2048, what);
}

static int lr_logits_launch(const float* x, int N, int d, const double* W, int K, int p, double* out, const double* state,
                            hipStream_t stream) {
  const size_t lds = lr_logits_lds(d, p);
  int rc = lr_lds_attr((const void*)logreg_logits_kernel, lds, "logreg_logits");
  if (rc) return rc;
  logreg_logits_kernel<<<(N + kLrStrip - 1) / kLrStrip, kLrThreads, lds, stream>>>(x, N, d, W, K, p, out, state);
  return check_launch("logreg_logits_kernel");
}

static int lr_line_launch(const double* Z, const double* ZD, const int* y, int N, int d, int K, int p, double* W, double* solver,
                          int m, double lambda, int T, double* state, int* ring, int ring_len, char* ws, const LrLayout& w,
                          hipStream_t stream) {
  const LrSolver q = lr_solver(solver, K * p, m);
  const dim3 grid(lr_chunks(N), T);
  logreg_line_kernel<<<grid, kLrThreads, 0, stream>>>(Z, ZD, y, N, K, p, d, W, q.D, lambda, T, reinterpret_cast<double*>(ws + w.line),
                                                      reinterpret_cast<unsigned*>(ws + w.ticket), state, ring, ring_len);
  return check_launch("logreg_line_kernel");
}

static int lr_grad_launch(const float* x, const int* y, int N, int d, int K, int p, double* Z, double* ZD, const double* state,
                          char* ws, const LrLayout& w, hipStream_t stream) {
  const size_t lds = lr_grad_lds(p, K);
  int rc = lr_lds_attr((const void*)logreg_grad_kernel, lds, "logreg_grad");
  if (rc) return rc;
  logreg_grad_kernel<<<lr_chunks(N), kLrGradThreads, lds, stream>>>(x, y, N, d, K, p, lr_grad_width(p), lr_grad_tile(p, K),
                                                                    lr_grad_sub(p, K), Z, ZD, reinterpret_cast<double*>(ws + w.part),
                                                                    reinterpret_cast<double*>(ws + w.loss), state);
  return check_launch("logreg_grad_kernel");
}

static int lr_finish_launch(int N, int d, int K, int p, const double* W, double* solver, int m, double lambda, double tol,
                            double* state, char* ws, const LrLayout& w, hipStream_t stream) {
  logreg_finish_kernel<<<1, kLrThreads, 0, stream>>>(reinterpret_cast<const double*>(ws + w.part),
                                                     reinterpret_cast<const double*>(ws + w.loss), lr_chunks(N), N, K, p, d, W, solver,
                                                     m, lambda, tol, state);
  return check_launch("logreg_finish_kernel");
}

}  // namespace evae

using namespace evae;

extern "C" int evae_logreg_max_classes(void) { return kLrMaxK; }
extern "C" int evae_logreg_max_features(void) { return kLrMaxD; }
extern "C" int evae_logreg_max_points(void) { return kLrMaxN; }
extern "C" int evae_logreg_max_history(void) { return kLrMaxHistory; }
extern "C" int evae_logreg_max_line_steps(void) { return kLrMaxLine; }
extern "C" int evae_logreg_chunk_rows(void) { return kLrChunk; }
extern "C" size_t evae_logreg_max_bytes(void) { return kLrMaxBytes; }

extern "C" size_t evae_logreg_solver_doubles(int d, int K, int fit_intercept, int history) {
  if (d < 1 || K < 1 || history < 1) return 0;
  return lr_solver_doubles(K * (d + (fit_intercept ? 1 : 0)), history);
}

extern "C" size_t evae_logreg_workspace_bytes(int N, int d, int K, int fit_intercept, int line_steps) {
  if (N < 1 || d < 1 || K < 1 || line_steps < 1) return 0;
  return lr_layout(N, K * (d + (fit_intercept ? 1 : 0)), line_steps).bytes;
}

#define LR_SHAPE(who)                                                                                                  \
  EVAE_REQUIRE(d >= 1 && d <= kLrMaxD, who ": d=%d outside [1, %d]", d, kLrMaxD);                                      \
  EVAE_REQUIRE(K >= 2 && K <= kLrMaxK, who ": K=%d outside [2, %d]", K, kLrMaxK);                                      \
  const int p = d + (fit_intercept ? 1 : 0)

#define LR_ROWS(who) EVAE_REQUIRE(N >= 1 && N <= kLrMaxN, who ": N=%d outside [1, %d]", N, kLrMaxN)

#define LR_SIZES(who)                                                                                                  \
  LR_SHAPE(who);                                                                                                       \
  LR_ROWS(who);                                                                                                        \
  EVAE_REQUIRE(line_steps >= 1 && line_steps <= kLrMaxLine, who ": line_steps=%d outside [1, %d]", line_steps, kLrMaxLine); \
  EVAE_REQUIRE(2 * (size_t)N * K * sizeof(double) + evae_logreg_workspace_bytes(N, d, K, fit_intercept, line_steps) <= kLrMaxBytes, \
               who ": Z and Z_D of %zu bytes each plus a workspace of %zu bytes for N=%d, d=%d, K=%d exceed %zu bytes", \
               (size_t)N * K * sizeof(double), evae_logreg_workspace_bytes(N, d, K, fit_intercept, line_steps), N, d, K, \
               kLrMaxBytes);                                                                                           \
  EVAE_REQUIRE(ws && ((uintptr_t)ws & 255) == 0, who ": null or misaligned workspace");                                \
  EVAE_REQUIRE(ws_bytes >= evae_logreg_workspace_bytes(N, d, K, fit_intercept, line_steps),                            \
               who ": workspace of %zu bytes, %zu needed", ws_bytes,                                                   \
               evae_logreg_workspace_bytes(N, d, K, fit_intercept, line_steps));                                       \
  const LrLayout w = lr_layout(N, K * p, line_steps);                                                                  \
  char* base = static_cast<char*>(ws)

#define LR_HISTORY(who) \
  EVAE_REQUIRE(history >= 1 && history <= kLrMaxHistory, who ": history=%d outside [1, %d]", history, kLrMaxHistory)

extern "C" int evae_logreg_logits(const float* x, int N, int d, const double* W, int K, int fit_intercept, double* out,
                                  evae_stream_t stream_) {
  LR_SHAPE("logreg_logits");
  LR_ROWS("logreg_logits");
  EVAE_REQUIRE(x && W && out, "logreg_logits: null pointer");
  EVAE_REQUIRE(aligned8(W) && aligned8(out), "logreg_logits: misaligned pointer");
  return lr_logits_launch(x, N, d, W, K, p, out, nullptr, (hipStream_t)stream_);
}

extern "C" int evae_logreg_line(const double* Z, const double* ZD, const int* y, int N, int d, int K, int fit_intercept, double* W,
                                double* solver, int history, double lambda, int line_steps, double* state, int* ring, int ring_len,
                                void* ws, size_t ws_bytes, evae_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  LR_SIZES("logreg_line");
  LR_HISTORY("logreg_line");
  EVAE_REQUIRE(Z && ZD && y && W && solver && state, "logreg_line: null pointer");
  EVAE_REQUIRE(aligned8(Z) && aligned8(ZD) && aligned8(W) && aligned8(solver) && aligned8(state), "logreg_line: misaligned pointer");
  EVAE_REQUIRE(lambda >= 0.0 && lambda < INFINITY, "logreg_line: lambda=%g", lambda);
  EVAE_REQUIRE(ring == nullptr || ring_len >= 1, "logreg_line: ring_len=%d", ring_len);
  if (hipMemsetAsync(base + w.ticket, 0, sizeof(unsigned), stream) != hipSuccess) return check_launch("logreg_line: ticket");
  return lr_line_launch(Z, ZD, y, N, d, K, p, W, solver, history, lambda, line_steps, state, ring, ring_len, base, w, stream);
}

extern "C" int evae_logreg_grad(const float* x, const int* y, int N, int d, int K, int fit_intercept, int line_steps, double* Z,
                                double* ZD, const double* state, void* ws, size_t ws_bytes, evae_stream_t stream_) {
  LR_SIZES("logreg_grad");
  EVAE_REQUIRE(x && y && Z && ZD && state, "logreg_grad: null pointer");
  EVAE_REQUIRE(aligned8(Z) && aligned8(ZD) && aligned8(state), "logreg_grad: misaligned pointer");
  return lr_grad_launch(x, y, N, d, K, p, Z, ZD, state, base, w, (hipStream_t)stream_);
}

extern "C" int evae_logreg_finish(int N, int d, int K, int fit_intercept, int line_steps, const double* W, double* solver,
                                  int history, double lambda, double tol, double* state, void* ws, size_t ws_bytes,
                                  evae_stream_t stream_) {
  LR_SIZES("logreg_finish");
  LR_HISTORY("logreg_finish");
  EVAE_REQUIRE(W && solver && state, "logreg_finish: null pointer");
  EVAE_REQUIRE(aligned8(W) && aligned8(solver) && aligned8(state), "logreg_finish: misaligned pointer");
  EVAE_REQUIRE(lambda >= 0.0 && lambda < INFINITY && tol >= 0.0, "logreg_finish: lambda=%g, tol=%g", lambda, tol);
  return lr_finish_launch(N, d, K, p, W, solver, history, lambda, tol, state, base, w, (hipStream_t)stream_);
}

extern "C" int evae_logreg_direction(double* solver, int d, int K, int fit_intercept, int history, double* state,
                                     evae_stream_t stream_) {
  LR_SHAPE("logreg_direction");
  LR_HISTORY("logreg_direction");
  EVAE_REQUIRE(solver && state && aligned8(solver) && aligned8(state), "logreg_direction: null or misaligned pointer");
  logreg_direction_kernel<<<1, kLrThreads, 0, (hipStream_t)stream_>>>(solver, K * p, history, state);
  return check_launch("logreg_direction_kernel");
}

#define LR_FIT_ARGS(who)                                                                                               \
  LR_SIZES(who);                                                                                                       \
  LR_HISTORY(who);                                                                                                     \
  EVAE_REQUIRE(x && y && W && Z && ZD && solver && state, who ": null pointer");                                       \
  EVAE_REQUIRE(aligned8(W) && aligned8(Z) && aligned8(ZD) && aligned8(solver) && aligned8(state), who ": misaligned pointer"); \
  EVAE_REQUIRE(lambda >= 0.0 && lambda < INFINITY && tol >= 0.0, who ": lambda=%g, tol=%g", lambda, tol)

extern "C" int evae_logreg_begin(const float* x, const int* y, int N, int d, int K, int fit_intercept, double* W, double* Z,
                                 double* ZD, double* solver, int history, double lambda, double tol, int line_steps, double* state,
                                 void* ws, size_t ws_bytes, evae_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  LR_FIT_ARGS("logreg_begin");
  if (hipMemsetAsync(state, 0, 8 * sizeof(double), stream) != hipSuccess ||
      hipMemsetAsync(solver, 0, lr_solver_doubles(K * p, history) * sizeof(double), stream) != hipSuccess ||
      hipMemsetAsync(base + w.ticket, 0, sizeof(unsigned), stream) != hipSuccess)
    return check_launch("logreg_begin: memset");
  int rc = lr_logits_launch(x, N, d, W, K, p, Z, nullptr, stream);
  if (rc) return rc;
  if ((rc = lr_grad_launch(x, y, N, d, K, p, Z, ZD, state, base, w, stream))) return rc;
  return lr_finish_launch(N, d, K, p, W, solver, history, lambda, tol, state, base, w, stream);
}

extern "C" int evae_logreg_step(const float* x, const int* y, int N, int d, int K, int fit_intercept, double* W, double* Z,
                                double* ZD, double* solver, int history, double lambda, double tol, int line_steps, double* state,
                                int* ring, int ring_len, void* ws, size_t ws_bytes, evae_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  LR_FIT_ARGS("logreg_step");
  EVAE_REQUIRE(ring == nullptr || ring_len >= 1, "logreg_step: ring_len=%d", ring_len);
  const LrSolver q = lr_solver(solver, K * p, history);
  int rc = lr_logits_launch(x, N, d, q.D, K, p, ZD, state, stream);
  if (rc) return rc;
  if ((rc = lr_line_launch(Z, ZD, y, N, d, K, p, W, solver, history, lambda, line_steps, state, ring, ring_len, base, w, stream)))
    return rc;
  if ((rc = lr_grad_launch(x, y, N, d, K, p, Z, ZD, state, base, w, stream))) return rc;
  return lr_finish_launch(N, d, K, p, W, solver, history, lambda, tol, state, base, w, stream);
}

extern "C" int evae_logreg_softmax(const double* Z, int N, int K, double* logp, int* labels, evae_stream_t stream_) {
  EVAE_REQUIRE(N >= 1 && N <= kLrMaxN, "logreg_softmax: N=%d outside [1, %d]", N, kLrMaxN);
  EVAE_REQUIRE(K >= 2 && K <= kLrMaxK, "logreg_softmax: K=%d outside [2, %d]", K, kLrMaxK);
  EVAE_REQUIRE(Z && (logp || labels), "logreg_softmax: null pointer");
  EVAE_REQUIRE(aligned8(Z) && aligned8(logp), "logreg_softmax: misaligned pointer");
  logreg_softmax_kernel<<<(N + kLrThreads - 1) / kLrThreads, kLrThreads, 0, (hipStream_t)stream_>>>(Z, N, K, logp, labels);
  return check_launch("logreg_softmax_kernel");
}
