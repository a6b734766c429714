// Kernel sums of one set of rows against another on gfx950, all arithmetic in fp64 on fp32 rows: what the unbiased kernel MMD^2
// (KID with the cubic kernel) is made of, the ordered grand total of such sums, and the small congruence product A S A^T of the
// Frechet distance's matrix square root (evae/sample_quality.py; DESIGN 3.7h has the formulae, the order of every sum and the
// measurements).  No [B x N] buffer exists at any point, there is no atomic and every sum has a fixed order, so equal inputs
// give bit-equal outputs, and a row's bits depend neither on B, nor on where the row sits in the batch, nor on the grid.
//
//   row_sum[i] = sum_j k(q_i, c_j), j ascending; with skip_self the term j == i is left out BY INDEX (the within-set form).
//     POLY: k = (gamma <q_i, c_j> + coef0)^degree   the dot product by fma in ascending feature order (a product of two fp32
//           values is exact in fp64: only the additions round), v = fma(gamma, dot, coef0), then degree - 1 multiplications by v.
//     RBF:  k = exp(-gamma |q_i - c_j|^2)           the difference taken directly in fp64, fma(df, df, acc), never expanded.
//
//   row_sums: a block is ONE wave of 64 queries, one per lane; their rows sit in LDS transposed (float [d][64]: conflict-free,
//             one read per kKsTile fp64 operations).  The columns pass through LDS as fp64 in tiles of kKsTile rows, a tile in
//             chunks of kKsDims features ([feature][column], so that a thread's read of a column entry is a broadcast and a
//             chunk row is one contiguous run); the thread keeps the tile's 32 accumulators in registers.  The chunks are double
//             buffered: the next chunk's fp32 entries are in flight from global memory (16 registers) while the current one is
//             consumed, one barrier per chunk.  A tile's 32 terms are added in index order into s, then total += s: tiles in
//             index order.  The tile is a constant (evae_kernel_sum_tile), so no tuning argument exists that could change a bit.
//             A one-wave block is what spreads B = 10^4 rows over 157 compute units; the price is that every wave stages its
//             own copy of the columns (L2 traffic, 1 / 64 of the arithmetic).
//   Rows past B are clamped for reading and not written; tile slots past N are never read from memory (the slot holds 0) and
//   their terms are left out by index, as the skipped diagonal is.  Every thread reaches every barrier.
//   Non-finite inputs: a NaN or inf in q_i stays in row i; one in c_j reaches every row (every row's sum has that term).
//
//   ordered_sum: one workgroup, ordered_total of evae_latent.h: x[0] + x[1] + .. left to right.
//   sym_congruence: T = A S into the workspace (thread per entry, m ascending), then out[i][j] = sum_k T[i][k] A[j][k] for
//             i <= j (k ascending), written to [i][j] and [j][i] from the one value.
#include "evae_latent.h"

namespace evae {

constexpr int kKsMaxD = 256;
constexpr int kKsMaxN = 1 << 20;
constexpr int kKsMaxDegree = 8;
constexpr int kKsTile = 32;                                   // columns of one tile: the accumulators of a thread
constexpr int kKsDims = 32;                                   // features of one staged chunk
constexpr int kKsRows = 64;                                   // queries of a block: one wave
constexpr int kKsLd = kKsTile + 2;                            // chunk row stride in doubles: 16-byte aligned, staging stores 4-way
constexpr int kKsPre = kKsTile * kKsDims / kKsRows;           // chunk entries a lane brings: 16
constexpr int kKsSumThreads = 256;
constexpr int kKsCongTile = 16;

enum { kKsPoly = EVAE_KERNEL_POLY, kKsRbf = EVAE_KERNEL_RBF };

// the fp32 entries of chunk (j0, k0) this lane brings: feature fastest (a column's run of features is one 128-byte line)
__device__ __forceinline__ void ks_fetch(const float* __restrict__ c, int N, int d, int j0, int k0, int lane, float (&pre)[kKsPre]) {
#pragma unroll
  for (int r = 0; r < kKsPre; ++r) {
    const int e = r * kKsRows + lane, u = e / kKsDims, sk = e % kKsDims;
    const int j = j0 + u, k = k0 + sk;
    pre[r] = (j < N && k < d) ? c[(size_t)j * d + k] : 0.0f;  // past the end: nothing is read
  }
}

__device__ __forceinline__ void ks_store(double (*sc)[kKsLd], int lane, const float (&pre)[kKsPre]) {
#pragma unroll
  for (int r = 0; r < kKsPre; ++r) {
    const int e = r * kKsRows + lane, u = e / kKsDims, sk = e % kKsDims;
    sc[sk][u] = (double)pre[r];
  }
}

// dynamic LDS: the block's rows transposed, float [d][64]
template <int KIND>
__global__ __launch_bounds__(kKsRows) void kernel_row_sums_kernel(const float* __restrict__ q, int B, const float* __restrict__ c,
                                                                  int N, int d, double gamma, double coef0, int degree,
                                                                  int skip_self, double* __restrict__ row_sum) {
  __shared__ __attribute__((aligned(16))) double sc[2][kKsDims][kKsLd];
  extern __shared__ float zs[];
  const int lane = threadIdx.x;
  const int i = blockIdx.x * kKsRows + lane;
  const int ir = min(i, B - 1);
  for (int k = 0; k < d; ++k) zs[k * kKsRows + lane] = q[(size_t)ir * d + k];
  const int chunks = (d + kKsDims - 1) / kKsDims;
  const int tiles = (N + kKsTile - 1) / kKsTile;
  const int steps = tiles * chunks;
  const int self = skip_self ? i : -1;

  float pre[kKsPre];
  ks_fetch(c, N, d, 0, 0, lane, pre);
  double acc[kKsTile];
  double total = 0.0;
  int tile = 0, chunk = 0;
  for (int step = 0; step < steps; ++step) {
    double(*buf)[kKsLd] = sc[step & 1];
    ks_store(buf, lane, pre);
    // One barrier per chunk: the buffer written here was last read two steps ago, and every thread finished that read before
    // it reached the barrier of the step in between.  (The first pass also publishes zs.)
    __syncthreads();
    const int j0 = tile * kKsTile, k0 = chunk * kKsDims;
    int ntile = tile, nchunk = chunk + 1;
    if (nchunk == chunks) {
      nchunk = 0;
      ++ntile;
    }
    if (step + 1 < steps) ks_fetch(c, N, d, ntile * kKsTile, nchunk * kKsDims, lane, pre);
    if (chunk == 0) {
#pragma unroll
      for (int u = 0; u < kKsTile; ++u) acc[u] = 0.0;
    }
    const int kc = min(kKsDims, d - k0);
    for (int sk = 0; sk < kc; ++sk) {
      const double zv = (double)zs[(k0 + sk) * kKsRows + lane];
#pragma unroll
      for (int u = 0; u < kKsTile; ++u) {
        if (KIND == kKsPoly) {
          acc[u] = fma(zv, buf[sk][u], acc[u]);
        } else {
          const double df = zv - buf[sk][u];
          acc[u] = fma(df, df, acc[u]);
        }
      }
    }
    if (nchunk == 0) {                                         // the tile is complete: its terms in index order
      double s = 0.0;
#pragma unroll
      for (int u = 0; u < kKsTile; ++u) {
        double v;
        if (KIND == kKsPoly) {
          const double b = fma(gamma, acc[u], coef0);
          v = b;
          for (int t = 1; t < degree; ++t) v *= b;
        } else {
          v = exp(-gamma * acc[u]);
        }
        const int j = j0 + u;
        if (j < N && j != self) s += v;
      }
      total += s;
    }
    tile = ntile;
    chunk = nchunk;
  }
  if (i < B) row_sum[i] = total;
}

__global__ __launch_bounds__(kKsSumThreads) void ordered_sum_kernel(const double* __restrict__ x, int n, double* __restrict__ out) {
  __shared__ double buf[kKsSumThreads];
  const double total = ordered_total<kKsSumThreads>(x, n, buf);
  if (threadIdx.x == 0) out[0] = total;
}

// T[i][k] = sum_m A[i][m] S[m][k], m ascending
__global__ __launch_bounds__(kKsCongTile* kKsCongTile) void cong_left_kernel(const double* __restrict__ A,
                                                                             const double* __restrict__ S, int d,
                                                                             double* __restrict__ T) {
  const int k = blockIdx.x * kKsCongTile + threadIdx.x, i = blockIdx.y * kKsCongTile + threadIdx.y;
  if (i >= d || k >= d) return;
  double acc = 0.0;
  for (int m = 0; m < d; ++m) acc = fma(A[(size_t)i * d + m], S[(size_t)m * d + k], acc);
  T[(size_t)i * d + k] = acc;
}

// out[i][j] = out[j][i] = sum_k T[i][k] A[j][k], k ascending, for i <= j
__global__ __launch_bounds__(kKsCongTile* kKsCongTile) void cong_right_kernel(const double* __restrict__ T,
                                                                              const double* __restrict__ A, int d,
                                                                              double* __restrict__ out) {
  const int j = blockIdx.x * kKsCongTile + threadIdx.x, i = blockIdx.y * kKsCongTile + threadIdx.y;
  if (i >= d || j >= d || i > j) return;
  double acc = 0.0;
  for (int k = 0; k < d; ++k) acc = fma(T[(size_t)i * d + k], A[(size_t)j * d + k], acc);
  out[(size_t)i * d + j] = acc;
  out[(size_t)j * d + i] = acc;
}

}  // namespace evae

using namespace evae;

extern "C" int evae_kernel_sum_max_features(void) { return kKsMaxD; }
extern "C" int evae_kernel_sum_max_points(void) { return kKsMaxN; }
extern "C" int evae_kernel_sum_max_degree(void) { return kKsMaxDegree; }
extern "C" int evae_kernel_sum_tile(void) { return kKsTile; }

extern "C" int evae_kernel_row_sums(const float* q, int B, const float* c, int N, int d, int kind, double gamma, double coef0,
                                    int degree, int skip_self, double* row_sum, evae_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  EVAE_REQUIRE(d >= 1 && d <= kKsMaxD, "kernel_row_sums: %d features outside [1, %d]", d, kKsMaxD);
  EVAE_REQUIRE(B >= 1 && B <= kKsMaxN, "kernel_row_sums: B=%d outside [1, %d]", B, kKsMaxN);
  EVAE_REQUIRE(N >= 1 && N <= kKsMaxN, "kernel_row_sums: N=%d outside [1, %d]", N, kKsMaxN);
  EVAE_REQUIRE(kind == kKsPoly || kind == kKsRbf, "kernel_row_sums: kind=%d (0 poly, 1 rbf)", kind);
  EVAE_REQUIRE(kind != kKsPoly || (degree >= 1 && degree <= kKsMaxDegree), "kernel_row_sums: degree=%d outside [1, %d]", degree,
               kKsMaxDegree);
  EVAE_REQUIRE(!skip_self || B == N, "kernel_row_sums: skip_self with B=%d, N=%d", B, N);
  EVAE_REQUIRE(q && c && row_sum, "kernel_row_sums: null pointer");
  EVAE_REQUIRE(aligned8(row_sum), "kernel_row_sums: misaligned fp64 buffer");
  const int zs_bytes = d * kKsRows * (int)sizeof(float);         // <= 64 KiB beside 17 KiB of static LDS
  int rc;
  if (kind == kKsPoly) {
    // Only a wide input needs more LDS than a launch gets unasked: the latents' d = 40 (10 KiB) goes without this host call.
    if (zs_bytes > 32 * 1024 &&
        (rc = set_max_lds((const void*)kernel_row_sums_kernel<kKsPoly>, zs_bytes, "kernel_row_sums_kernel")))
      return rc;
    kernel_row_sums_kernel<kKsPoly><<<cdiv(B, kKsRows), kKsRows, zs_bytes, stream>>>(q, B, c, N, d, gamma, coef0, degree,
                                                                                      skip_self, row_sum);
  } else {
    if (zs_bytes > 32 * 1024 &&
        (rc = set_max_lds((const void*)kernel_row_sums_kernel<kKsRbf>, zs_bytes, "kernel_row_sums_kernel")))
      return rc;
    kernel_row_sums_kernel<kKsRbf><<<cdiv(B, kKsRows), kKsRows, zs_bytes, stream>>>(q, B, c, N, d, gamma, coef0, degree,
                                                                                     skip_self, row_sum);
  }
  return check_launch("kernel_row_sums_kernel");
}

extern "C" int evae_ordered_sum(const double* x, int n, double* out, evae_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  EVAE_REQUIRE(n >= 1 && n <= kKsMaxN, "ordered_sum: n=%d outside [1, %d]", n, kKsMaxN);
  EVAE_REQUIRE(x && out, "ordered_sum: null pointer");
  EVAE_REQUIRE(aligned8(x) && aligned8(out), "ordered_sum: misaligned fp64 buffer");
  ordered_sum_kernel<<<1, kKsSumThreads, 0, stream>>>(x, n, out);
  return check_launch("ordered_sum_kernel");
}

extern "C" size_t evae_sym_congruence_workspace_bytes(int d) {
  if (d < 1 || d > kKsMaxD) return 0;
  return align_up((size_t)d * d * sizeof(double), 256);
}

extern "C" int evae_sym_congruence(const double* A, const double* S, double* out, int d, void* ws, size_t ws_bytes,
                                   evae_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  EVAE_REQUIRE(d >= 1 && d <= kKsMaxD, "sym_congruence: d=%d outside [1, %d]", d, kKsMaxD);
  EVAE_REQUIRE(A && S && out && ws, "sym_congruence: null pointer");
  EVAE_REQUIRE(aligned8(A) && aligned8(S) && aligned8(out) && aligned8(ws), "sym_congruence: misaligned fp64 buffer");
  const size_t need = evae_sym_congruence_workspace_bytes(d);
  EVAE_REQUIRE(ws_bytes >= need, "sym_congruence: workspace of %zu bytes, %zu needed", ws_bytes, need);
  double* T = static_cast<double*>(ws);
  const size_t n = (size_t)d * d;
  const auto apart = [n](const double* a, const double* b) { return a + n <= b || b + n <= a; };
  EVAE_REQUIRE(apart(out, A) && apart(out, S), "sym_congruence: out overlaps an input");
  EVAE_REQUIRE(apart(T, A) && apart(T, S) && apart(T, out), "sym_congruence: the workspace overlaps A, S or out");
  const dim3 block(kKsCongTile, kKsCongTile), grid(cdiv(d, kKsCongTile), cdiv(d, kKsCongTile));
  int rc;
  cong_left_kernel<<<grid, block, 0, stream>>>(A, S, d, T);
  if ((rc = check_launch("cong_left_kernel"))) return rc;
  cong_right_kernel<<<grid, block, 0, stream>>>(T, A, d, out);
  return check_launch("cong_right_kernel");
}
