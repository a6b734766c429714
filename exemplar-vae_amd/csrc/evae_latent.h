// The one copy of the blocks the latent-analysis kernels share: evae_tsne_nn.hip, evae_nn_rank.hip, evae_pca.hip,
// evae_kmeans.hip, evae_gmm.hip, evae_ball_count.hip, evae_agg_lse.hip, evae_kernel_sum.hip, evae_logreg.hip.  They all rest on one contract -- fp64
// arithmetic on fp32 rows, no floating-point atomics, every sum in a fixed order, equal inputs giving bit-equal outputs -- and this header
// carries it: nothing here changes the order of a sum, and a helper that would need to know which caller it serves does not
// belong here.
// tests/test_gpu_latent_bits.py holds the callers to the bits they gave before the blocks were shared.
#pragma once
#include "evae_common.h"

namespace evae {

constexpr int kNoIndex = 0x7fffffff;                             // "no row / no centre / no component yet": above every index

// ---------------------------------------------------------------- device side
// The record of an iterated step (kmeans_step, gmm_step, logreg_step): state[1] != 0 once it is done.  Every kernel of a step starts with
// this test -- the same value in every thread of the grid, written by an EARLIER launch of the stream.
__device__ __forceinline__ bool step_done(const double* state) { return state != nullptr && state[1] != 0.0; }

// Thread (g, c) of a block of G groups of W columns brings s, its partial sum of column c; the owner (group 0 of a live
// column) gets the G partial sums added in order of g, everybody else 0.  One barrier, after the store: a caller that loops
// closes its round with a barrier of its own.
__device__ __forceinline__ double group_fold(double s, double* part, int c, int W, int G, bool owner) {
  part[threadIdx.x] = s;
  __syncthreads();
  double t = 0.0;
  if (owner)
    for (int h = 0; h < G; ++h) t += part[h * W + c];
  return t;
}

// A 256-thread block's sum of s: the four waves' sums through wpart[4], ((w0 + w1) + w2) + w3 by thread 0 into *out
__device__ __forceinline__ void chunk_sum_store(double s, double* wpart, double* out) {
  const int tid = threadIdx.x;
  s = wave_sum(s);
  if ((tid & 63) == 0) wpart[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) *out = ((wpart[0] + wpart[1]) + wpart[2]) + wpart[3];
}

// The chunk sums through LDS (buf[THREADS]), added by thread 0 in chunk order; the total is thread 0's alone
template <int THREADS>
__device__ __forceinline__ double ordered_total(const double* __restrict__ chunk_sum, int chunks, double* buf) {
  const int tid = threadIdx.x;
  double total = 0.0;
  for (int c0 = 0; c0 < chunks; c0 += THREADS) {
    if (c0 + tid < chunks) buf[tid] = chunk_sum[c0 + tid];
    __syncthreads();
    if (tid == 0) {
      const int n = min(THREADS, chunks - c0);
      for (int e = 0; e < n; ++e) total += buf[e];
    }
    __syncthreads();
  }
  return total;
}

// ---------------------------------------------------------------- host side
// the smallest power of two >= cols, capped at the block (no cap in effect for PCA and k-means: d <= 256 = their threads)
static inline int pow2_width(int cols, int threads) {
  int W = 1;
  while (W < cols && W < threads) W <<= 1;
  return W;
}

// offsets of a workspace's parts, each on a 256-byte boundary; `o` ends as the size of the whole
struct WsCursor {
  size_t o = 0;
  size_t take(size_t bytes) {
    const size_t at = o;
    o += align_up(bytes, 256);
    return at;
  }
};

static inline bool aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }

// More dynamic LDS for `fn` than a launch gets unasked.  Where it is needed, at every call, not once per process: the
// attribute belongs to the function on the CURRENT device.  When it is needed, and how much, is the caller's to say.
static inline int set_max_lds(const void* fn, int bytes, const char* what) {
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e != hipSuccess) {
    set_error("%s: %d bytes of LDS refused: %s", what, bytes, hipGetErrorString(e));
    return EVAE_ELAUNCH;
  }
  return EVAE_OK;
}

// Query rows R per strip of [R x N] fp32 distances: the caller's strip_rows, or (0) what fits kStripBytes in whole tiles of
// the distance kernel.  evae_tsne_knn_workspace_bytes is the exported form of the same rule.
constexpr size_t kStripBytes = (size_t)256 << 20;
static inline int strip_rows_of(int N, int strip_rows) {
  if (strip_rows > 0) return strip_rows > N ? N : strip_rows;
  size_t r = kStripBytes / ((size_t)N * sizeof(float));
  if (r >= 64) r &= ~(size_t)63;
  if (r < 1) r = 1;
  return r > (size_t)N ? N : (int)r;
}

// The squared distances of x's rows r0 .. r0 + rows to all N rows, R rows at a time into `strip`; reader(r0, rows) launches
// what consumes the strip and returns its status.
template <typename Reader>
static inline int for_each_strip(const float* x, int N, int d, int R, float* strip, evae_stream_t stream, Reader reader) {
  for (int r0 = 0; r0 < N; r0 += R) {
    const int rows = N - r0 < R ? N - r0 : R;
    int rc = evae_pairwise_distance(x + (size_t)r0 * d, rows, x, N, d, strip, stream);
    if (rc) return rc;
    if ((rc = reader(r0, rows))) return rc;
  }
  return EVAE_OK;
}

// The cross-set siblings: B query rows from one array, N columns from another.  The same byte rule on the column count; the
// strip is never longer than the queries.
static inline int cross_strip_rows_of(int B, int N, int strip_rows) {
  size_t r = strip_rows > 0 ? (size_t)strip_rows : kStripBytes / ((size_t)N * sizeof(float));
  if (strip_rows <= 0 && r >= 64) r &= ~(size_t)63;
  if (r < 1) r = 1;
  return r > (size_t)B ? B : (int)r;
}

// The squared distances of q's rows r0 .. r0 + rows to all N rows of c, R rows at a time into `strip`
template <typename Reader>
static inline int for_each_cross_strip(const float* q, int B, const float* c, int N, int d, int R, float* strip,
                                       evae_stream_t stream, Reader reader) {
  for (int r0 = 0; r0 < B; r0 += R) {
    const int rows = B - r0 < R ? B - r0 : R;
    int rc = evae_pairwise_distance(q + (size_t)r0 * d, rows, c, N, d, strip, stream);
    if (rc) return rc;
    if ((rc = reader(r0, rows))) return rc;
  }
  return EVAE_OK;
}

}  // namespace evae
