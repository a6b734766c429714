// t-SNE with sparse affinities and exact repulsion on gfx950: scikit-learn's large-N formulation (P on each point's
// k = min(N - 1, floor(3 perplexity) + 1) nearest neighbours, symmetrised) without its tree -- the repulsive sum and Z run over all
// N^2 pairs, as Barnes-Hut would give at angle 0.  No [N x N] buffer exists at any point.  DESIGN 3.7a has the formulas, the
// launch sequence and the byte / operation counts; evae_tsne.hip is the dense path, whose update launch this one reuses.
//
//   neighbours:   the queries go in strips of R rows; the strip's [R x N] distances come from evae_pairwise_distance (fp64
//                 accumulated, rounded once) into a workspace.  One workgroup per row then radix-selects the k-th smallest key
//                 (distances are >= 0: their bit patterns order as unsigned integers) with four 8-bit LDS histograms, gathers
//                 everything below it plus the lowest-indexed ties, and rank-sorts the k by (value, index) in LDS.  The row is
//                 read five times and never has to fit LDS.  Integer LDS atomics only: counts do not depend on order.
//   conditionals: one wave per row over its k distances (4 per lane at most), the search of tsne_beta_kernel restated: shift by
//                 the row minimum, fp64, fixed length, the same doubling / halving rule; every lane takes the same branch.
//   joint:        val_e = (a + b) / 2N from the two conditionals the host-side index plumbing pairs up; (i, j) forms a + b and
//                 (j, i) forms b + a, the same float.
//   forces:       launch 1, repulsion: block (rb, cs) owns 256 rows (one per thread, y_i in registers) and a range of 256-column
//                 tiles of Y staged through LDS (every lane reads the same y_j: a broadcast); R_i and Z_i partial sums in fp64 go
//                 to rep[cs][i][3].  Launch 2, attraction: a wave per CSR row loops over its non-zeros, then adds the row's
//                 column-split partials in split order and writes the [8] record of evae_tsne_forces.  Fixed order throughout,
//                 no floating-point atomics, no grid-wide barrier.  Launch 3 is evae_tsne_update.
#include "evae_latent.h"

namespace evae {

constexpr int kNnMaxPoints = 131072;      // see include/evae_hip.h for what sets it
constexpr int kNnMaxNeighbours = 256;     // one wave holds a row of the search in registers, 4 values per lane
constexpr int kSelThreads = 256;
constexpr int kHistCopies = 16;           // the top byte of a float puts most of a row into a few bins: 16 copies, one per lane & 15
constexpr int kRepRows = 256;             // rows of a repulsion block = its threads
constexpr int kRepTile = 256;             // columns of Y per LDS tile
constexpr int kRepBlocksWanted = 1024;    // 256 CUs x 4 SIMDs: one wave per SIMD from this launch alone needs 256 blocks; x 4 to hide latency
constexpr int kPartStride = 8;

// ------------------------------------------------------------------------------------------------ neighbours
// row: the distances of query `self` to all N points.  out_idx / out_val: the k nearest, self left out BY INDEX.
__global__ __launch_bounds__(kSelThreads) void tsne_knn_select_kernel(const float* __restrict__ strip, int N, int row0, int k,
                                                                       int* __restrict__ out_idx, float* __restrict__ out_val) {
  __shared__ unsigned hist[256 * kHistCopies];
  __shared__ unsigned long long cand[kNnMaxNeighbours];
  __shared__ unsigned sel[2];                                 // the chosen bin, the rank that remains inside it
  __shared__ unsigned counter[2];                             // gathered below the threshold, gathered at it
  __shared__ unsigned wcnt[kSelThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int self = row0 + blockIdx.x;
  const unsigned* keys = reinterpret_cast<const unsigned*>(strip + (size_t)blockIdx.x * N);

  unsigned prefix = 0, rank = (unsigned)k, in_bin = 0;        // rank: 1-based, among the keys that share `prefix`
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    for (int b = tid; b < 256 * kHistCopies; b += kSelThreads) hist[b] = 0;
    __syncthreads();
    for (int j = tid; j < N; j += kSelThreads) {
      if (j == self) continue;
      const unsigned key = keys[j];
      if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[((key >> shift) & 255u) * kHistCopies + (lane & (kHistCopies - 1))], 1u);
    }
    __syncthreads();
    unsigned c = 0;
#pragma unroll
    for (int r = 0; r < kHistCopies; ++r) c += hist[tid * kHistCopies + r];
    __syncthreads();
    hist[tid] = c;                                            // bin tid's count, copies folded
    __syncthreads();
    if (wave == 0) {                                          // lane l: bins 4l .. 4l + 3
      const unsigned c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
      const unsigned s = c0 + c1 + c2 + c3;
      unsigned incl = s;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
      }
      const unsigned excl = incl - s;
      if (excl < rank && rank <= incl) {                      // exactly one lane
        unsigned r = rank - excl, b = 4 * lane, cnt = c0;
        if (r > c0) { r -= c0; ++b; cnt = c1;
          if (r > c1) { r -= c1; ++b; cnt = c2;
            if (r > c2) { r -= c2; ++b; cnt = c3; } } }
        sel[0] = b;
        sel[1] = r;
        counter[0] = cnt;                                     // borrowed until the gather: the chosen bin's population
      }
    }
    __syncthreads();
    prefix = (prefix << 8) | sel[0];
    rank = sel[1];
    in_bin = counter[0];
    __syncthreads();
  }
  // prefix: the k-th smallest key; `rank` of the in_bin keys equal to it are wanted, the lowest-indexed ones
  const unsigned thr = prefix, ties = rank, below = (unsigned)k - ties;
  if (tid < 2) counter[tid] = 0;
  __syncthreads();
  const bool all_ties = ties == in_bin;                       // then their order of arrival does not matter: the sort fixes it
  for (int j = tid; j < N; j += kSelThreads) {
    if (j == self) continue;
    const unsigned key = keys[j];
    if (key < thr) {
      const unsigned p = atomicAdd(&counter[0], 1u);
      if (p < below) cand[p] = ((unsigned long long)key << 32) | (unsigned)j;
    } else if (all_ties && key == thr) {
      const unsigned p = atomicAdd(&counter[1], 1u);
      if (p < ties) cand[below + p] = ((unsigned long long)key << 32) | (unsigned)j;
    }
  }
  if (!all_ties) {                                            // in index order, chunk by chunk, until `ties` are taken
    unsigned taken = 0;
    for (int base = 0; base < N && taken < ties; base += kSelThreads) {
      const int j = base + tid;
      const bool f = j < N && j != self && keys[j] == thr;
      const unsigned long long m = __ballot(f);
      if (lane == 0) wcnt[wave] = (unsigned)__popcll(m);
      __syncthreads();
      unsigned off = taken, total = 0;
#pragma unroll
      for (int w = 0; w < kSelThreads / 64; ++w) {
        if (w < wave) off += wcnt[w];
        total += wcnt[w];
      }
      off += (unsigned)__popcll(m & ((1ull << lane) - 1ull));
      if (f && off < ties) cand[below + off] = ((unsigned long long)thr << 32) | (unsigned)j;
      taken += total;
      __syncthreads();
    }
  }
  __syncthreads();
  if (tid < k) {                                              // rank sort: the composite keys are distinct
    const unsigned long long mine = cand[tid];
    int pos = 0;
    for (int t = 0; t < k; ++t) pos += cand[t] < mine;
    out_idx[(size_t)blockIdx.x * k + pos] = (int)(unsigned)(mine & 0xffffffffull);
    out_val[(size_t)blockIdx.x * k + pos] = __uint_as_float((unsigned)(mine >> 32));
  }
}

// ------------------------------------------------------------------------------------------------ conditionals
// one wave per row; the search of tsne_beta_kernel<64> over the k values of the row (no self among them)
__global__ __launch_bounds__(256) void tsne_nn_beta_kernel(const float* __restrict__ d2, int N, int k, double log_perp, int steps,
                                                            float* __restrict__ beta_out, float* __restrict__ cond) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N) return;                                         // whole waves leave; there is no barrier below
  const float* src = d2 + (size_t)i * k;
  float v[4];
  float m = INFINITY;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int j = lane + 64 * r;
    v[r] = j < k ? src[j] : INFINITY;
    m = fminf(m, v[r]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fminf(m, __shfl_xor(m, o, 64));
  const double dmin = (double)m;
  double dd[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) dd[r] = (double)v[r] - dmin;

  double beta = 1.0, lo = 0.0, hi = 0.0;
  bool has_lo = false, has_hi = false;
  for (int s = 0; s < steps; ++s) {
    double S = 0.0, SD = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (lane + 64 * r < k) {
        const double e = exp(-beta * dd[r]);
        S += e;
        SD = fma(dd[r], e, SD);
      }
    }
    S = wave_sum(S);
    SD = wave_sum(SD);
    const double H = log(S) + beta * SD / S;                  // S >= 1: the nearest neighbour contributes exp(0)
    if (H > log_perp) {                                       // too flat: raise the precision
      lo = beta; has_lo = true;
      beta = has_hi ? 0.5 * (beta + hi) : 2.0 * beta;
    } else {
      hi = beta; has_hi = true;
      beta = has_lo ? 0.5 * (beta + lo) : 0.5 * beta;
    }
  }
  double e[4], S = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    e[r] = (lane + 64 * r < k) ? exp(-beta * dd[r]) : 0.0;
    S += e[r];
  }
  S = wave_sum(S);
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (lane + 64 * r < k) cond[(size_t)i * k + lane + 64 * r] = (float)(e[r] / S);
  if (lane == 0) beta_out[i] = (float)beta;
}

// ------------------------------------------------------------------------------------------------ joint
// ia / ib: where in cond the entry's own conditional p(j|i) and its transpose's p(i|j) stand, -1 = outside that row's neighbours
__global__ __launch_bounds__(256) void tsne_nn_joint_kernel(const float* __restrict__ cond, const int* __restrict__ ia,
                                                             const int* __restrict__ ib, int nnz, float two_n,
                                                             float* __restrict__ val) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= nnz) return;
  const int a_at = ia[e], b_at = ib[e];
  const float a = a_at >= 0 ? cond[a_at] : 0.0f;
  const float b = b_at >= 0 ? cond[b_at] : 0.0f;
  val[e] = (a + b) / two_n;                                   // the transposed entry forms b + a: the same float
}

// ------------------------------------------------------------------------------------------------ forces
// rep [CS x N x 3] doubles: block (rb, cs) writes rows rb * 256 .. of split cs = (R_x, R_y, Z_i) over its columns
__global__ __launch_bounds__(kRepRows) void tsne_nn_repulsion_kernel(const float* __restrict__ Y, int N, int tiles_per_split,
                                                                      double* __restrict__ rep) {
  __shared__ float2 tile[kRepTile];
  const int tid = threadIdx.x;
  const int i = blockIdx.x * kRepRows + tid;
  const int ii = min(i, N - 1);                               // rows past the end repeat the last one and are not written
  const float2 yi = reinterpret_cast<const float2*>(Y)[ii];
  const int j_begin = blockIdx.y * tiles_per_split * kRepTile;
  const int j_end = min(N, j_begin + tiles_per_split * kRepTile);
  double rx = 0.0, ry = 0.0, z = 0.0;
  for (int j0 = j_begin; j0 < j_end; j0 += kRepTile) {
    const int len = min(kRepTile, j_end - j0);
    __syncthreads();
    if (tid < len) tile[tid] = reinterpret_cast<const float2*>(Y)[j0 + tid];
    __syncthreads();
#pragma unroll 4
    for (int t = 0; t < len; ++t) {
      const float2 yj = tile[t];
      const float dx = yi.x - yj.x, dy = yi.y - yj.y;
      const float w = 1.0f / (1.0f + (dx * dx + dy * dy));
      const float w2 = w * w;
      rx += (double)(w2 * dx);
      ry += (double)(w2 * dy);
      z += (j0 + t != ii) ? (double)w : 0.0;
    }
  }
  if (i < N) {
    double* o = rep + ((size_t)blockIdx.y * N + i) * 3;
    o[0] = rx;
    o[1] = ry;
    o[2] = z;
  }
}

template <bool KL>
__global__ __launch_bounds__(256) void tsne_nn_attraction_kernel(const int* __restrict__ row_ptr, const int* __restrict__ col,
                                                                  const float* __restrict__ val, const float* __restrict__ Y, int N,
                                                                  double exag, const double* __restrict__ rep, int splits,
                                                                  double* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N) return;                                         // whole waves leave; there is no barrier below
  const float2 yi = reinterpret_cast<const float2*>(Y)[i];
  const int e_end = row_ptr[i + 1];
  double ax = 0.0, ay = 0.0, kl = 0.0, sp = 0.0;
  for (int e = row_ptr[i] + lane; e < e_end; e += 64) {
    const float p = val[e];
    const float2 yj = reinterpret_cast<const float2*>(Y)[col[e]];
    const float dx = yi.x - yj.x, dy = yi.y - yj.y;
    const float q = 1.0f + (dx * dx + dy * dy);
    const float w = 1.0f / q;
    const float pw = p * w;
    ax += (double)(pw * dx);
    ay += (double)(pw * dy);
    if (KL) {
      if (p > 0.0f) kl = fma((double)p, log((double)p * (double)q), kl);
      sp += (double)p;
    }
  }
  ax = wave_sum(ax);
  ay = wave_sum(ay);
  if (KL) {
    kl = wave_sum(kl);
    sp = wave_sum(sp);
  }
  if (lane == 0) {
    double rx = 0.0, ry = 0.0, z = 0.0;
    for (int s = 0; s < splits; ++s) {                        // in split order
      const double* r = rep + ((size_t)s * N + i) * 3;
      rx += r[0];
      ry += r[1];
      z += r[2];
    }
    double* o = part + (size_t)i * kPartStride;
    o[0] = ax * exag;
    o[1] = ay * exag;
    o[2] = rx;
    o[3] = ry;
    o[4] = z;
    o[5] = kl;
    o[6] = sp;
    o[7] = 0.0;
  }
}

// how the repulsion's columns are split: enough blocks to fill the device, a whole number of tiles per split, no empty split
static void rep_split(int N, int* splits, int* tiles_per_split) {
  const int row_blocks = cdiv(N, kRepRows), tiles = cdiv(N, kRepTile);
  int cs = cdiv(kRepBlocksWanted, row_blocks);
  if (cs > tiles) cs = tiles;
  if (cs < 1) cs = 1;
  *tiles_per_split = cdiv(tiles, cs);
  *splits = cdiv(tiles, *tiles_per_split);
}

}  // namespace evae

using namespace evae;

extern "C" int evae_tsne_nn_max_points(void) { return kNnMaxPoints; }
extern "C" int evae_tsne_nn_max_neighbours(void) { return kNnMaxNeighbours; }

extern "C" size_t evae_tsne_knn_workspace_bytes(int N, int strip_rows) {
  if (N < 1) return 0;
  return (size_t)strip_rows_of(N, strip_rows) * (size_t)N * sizeof(float);
}

extern "C" int evae_tsne_knn(const float* z, int N, int zdim, int k, int strip_rows, int* idx, float* d2, void* ws, size_t ws_bytes,
                             evae_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  EVAE_REQUIRE(N >= 2 && N <= kNnMaxPoints, "tsne_knn: N=%d outside [2, %d]", N, kNnMaxPoints);
  EVAE_REQUIRE(zdim > 0, "tsne_knn: zdim=%d", zdim);
  EVAE_REQUIRE(k >= 1 && k <= kNnMaxNeighbours, "tsne_knn: k=%d outside [1, %d] (perplexity up to 85)", k, kNnMaxNeighbours);
  EVAE_REQUIRE(k <= N - 1, "tsne_knn: k=%d but a point has only N - 1 = %d neighbours", k, N - 1);
  EVAE_REQUIRE(strip_rows >= 0, "tsne_knn: strip_rows=%d (0 = automatic)", strip_rows);
  EVAE_REQUIRE(z && idx && d2 && ws, "tsne_knn: null pointer");
  const int R = strip_rows_of(N, strip_rows);
  EVAE_REQUIRE(ws_bytes >= (size_t)R * (size_t)N * sizeof(float), "tsne_knn: workspace of %zu bytes, %zu needed", ws_bytes,
               (size_t)R * (size_t)N * sizeof(float));
  float* strip = static_cast<float*>(ws);
  return for_each_strip(z, N, zdim, R, strip, stream_, [&](int r0, int rows) {
    tsne_knn_select_kernel<<<rows, kSelThreads, 0, stream>>>(strip, N, r0, k, idx + (size_t)r0 * k, d2 + (size_t)r0 * k);
    return check_launch("tsne_knn_select_kernel");
  });
}

extern "C" int evae_tsne_nn_conditionals(const float* d2, int N, int k, double perplexity, int steps, float* beta, float* cond,
                                         evae_stream_t stream_) {
  EVAE_REQUIRE(N >= 2 && N <= kNnMaxPoints, "tsne_nn_conditionals: N=%d outside [2, %d]", N, kNnMaxPoints);
  EVAE_REQUIRE(k >= 1 && k <= kNnMaxNeighbours && k <= N - 1, "tsne_nn_conditionals: k=%d outside [1, min(%d, N - 1)]", k,
               kNnMaxNeighbours);
  EVAE_REQUIRE(perplexity > 0.0 && perplexity < (double)N, "tsne_nn_conditionals: perplexity %g outside (0, N=%d)", perplexity, N);
  EVAE_REQUIRE(steps >= 1 && steps <= 1000, "tsne_nn_conditionals: steps=%d outside [1, 1000]", steps);
  EVAE_REQUIRE(d2 && beta && cond, "tsne_nn_conditionals: null pointer");
  tsne_nn_beta_kernel<<<cdiv(N, 4), 256, 0, (hipStream_t)stream_>>>(d2, N, k, log(perplexity), steps, beta, cond);
  return check_launch("tsne_nn_beta_kernel");
}

extern "C" int evae_tsne_nn_joint(const float* cond, int64_t n_cond, const int* ia, const int* ib, int nnz, int N, float* val,
                                  evae_stream_t stream_) {
  EVAE_REQUIRE(N >= 2 && N <= kNnMaxPoints, "tsne_nn_joint: N=%d outside [2, %d]", N, kNnMaxPoints);
  EVAE_REQUIRE(n_cond >= 1 && n_cond <= (int64_t)N * kNnMaxNeighbours, "tsne_nn_joint: %lld conditionals for N=%d",
               (long long)n_cond, N);
  EVAE_REQUIRE(nnz >= 1 && (int64_t)nnz <= 2 * n_cond, "tsne_nn_joint: nnz=%d outside [1, 2 x %lld]", nnz, (long long)n_cond);
  EVAE_REQUIRE(cond && ia && ib && val, "tsne_nn_joint: null pointer");
  tsne_nn_joint_kernel<<<cdiv(nnz, 256), 256, 0, (hipStream_t)stream_>>>(cond, ia, ib, nnz, 2.0f * (float)N, val);
  return check_launch("tsne_nn_joint_kernel");
}

extern "C" size_t evae_tsne_nn_forces_workspace_bytes(int N) {
  if (N < 1) return 0;
  int splits, tps;
  rep_split(N, &splits, &tps);
  return (size_t)splits * (size_t)N * 3 * sizeof(double);
}

extern "C" int evae_tsne_nn_forces(const int* row_ptr, const int* col, const float* val, const float* Y, int N, double exaggeration,
                                   int want_kl, double* part, void* ws, size_t ws_bytes, evae_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  EVAE_REQUIRE(N >= 2 && N <= kNnMaxPoints, "tsne_nn_forces: N=%d outside [2, %d]", N, kNnMaxPoints);
  EVAE_REQUIRE(row_ptr && col && val && Y && part && ws, "tsne_nn_forces: null pointer");
  EVAE_REQUIRE(((uintptr_t)Y & 7) == 0 && ((uintptr_t)ws & 7) == 0, "tsne_nn_forces: Y and the workspace must be 8-byte aligned");
  int splits, tps;
  rep_split(N, &splits, &tps);
  EVAE_REQUIRE(ws_bytes >= (size_t)splits * (size_t)N * 3 * sizeof(double), "tsne_nn_forces: workspace of %zu bytes, %zu needed",
               ws_bytes, (size_t)splits * (size_t)N * 3 * sizeof(double));
  double* rep = static_cast<double*>(ws);
  tsne_nn_repulsion_kernel<<<dim3(cdiv(N, kRepRows), splits), kRepRows, 0, stream>>>(Y, N, tps, rep);
  int rc = check_launch("tsne_nn_repulsion_kernel");
  if (rc) return rc;
  if (want_kl)
    tsne_nn_attraction_kernel<true><<<cdiv(N, 4), 256, 0, stream>>>(row_ptr, col, val, Y, N, exaggeration, rep, splits, part);
  else
    tsne_nn_attraction_kernel<false><<<cdiv(N, 4), 256, 0, stream>>>(row_ptr, col, val, Y, N, exaggeration, rep, splits, part);
  return check_launch("tsne_nn_attraction_kernel");
}
