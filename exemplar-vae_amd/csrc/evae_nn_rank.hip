// Ranks of chosen neighbours on gfx950: for every point i and each of k chosen columns j = nbr[i][m], the place of j among all
// other points ordered by (squared distance to i ascending, index ascending) -- the integer that trustworthiness, continuity and
// neighbourhood preservation of an embedding are sums of (evae/tsne.py; DESIGN 3.7b has the definition, the launch sequence and
// the traffic).  No [N x N] buffer and no sort of a row exist at any point.
//
//   distances: the queries go in strips of R rows, as in evae_tsne_knn; the strip's [R x N] distances come from
//              evae_pairwise_distance (fp64 accumulated, rounded once) into a workspace, so ranks agree with the neighbour
//              search bit for bit.
//   counting:  one workgroup per row.  The row's k thresholds (d2(i, j), j) are gathered and rank-sorted in LDS as 64-bit
//              composite keys (distances are >= 0: their bit patterns order as unsigned integers; the index in the low word breaks
//              ties).  The N distances then stream through once in 16-byte loads; each (d, l) is placed among the sorted
//              thresholds by binary search and bumps one of k LDS bins (16 copies of each, one per lane & 15: the top of a skewed
//              row lands in a few bins); an element not below the largest threshold -- most of a row when the chosen columns are
//              near neighbours -- leaves after one comparison.  An inclusive prefix sum of the bins gives, for the t-th sorted
//              threshold, the number of elements below it; the sort permutation is undone on the way out.  Integer LDS atomics
//              only: counts do not depend on order.  An entry j == i or outside [0, N) is never dereferenced and gets rank 0.
#include "evae_latent.h"

namespace evae {

constexpr int kRankThreads = 256;
constexpr int kRankMaxK = 256;            // = evae_tsne_nn_max_neighbours(): one lane of wave 0 scans 4 bins
constexpr int kBinCopies = 16;
constexpr unsigned long long kNoThreshold = ~0ull;

// sorted[0 .. kv): ascending, distinct or equal only between repeated columns; top = sorted[kv - 1] (0 when kv == 0).
// (key, l) is counted for every threshold above it: bin p = the number of thresholds <= (key, l), nothing to do at p == kv.
__device__ __forceinline__ void rank_place(unsigned key, int l, int self, const unsigned long long* sorted, int kv,
                                           unsigned long long top, unsigned* bins, int copy) {
  const unsigned long long e = ((unsigned long long)key << 32) | (unsigned)l;
  if (l == self || e >= top) return;
  int lo = 0, hi = kv - 1;                                    // sorted[kv - 1] > e is known
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (sorted[mid] <= e) lo = mid + 1; else hi = mid;
  }
  atomicAdd(&bins[lo * kBinCopies + copy], 1u);
}

// strip: rows row0 .. of the distance matrix, [rows x N].  nbr, rank: rows row0 .. of the [N x k] arrays; sums: of [N x 2].
__global__ __launch_bounds__(kRankThreads) void nn_rank_count_kernel(const float* __restrict__ strip, int N, int row0, int k,
                                                                      const int* __restrict__ nbr, int* __restrict__ rank,
                                                                      long long* __restrict__ sums) {
  __shared__ unsigned bins[kRankMaxK * kBinCopies];
  __shared__ unsigned long long raw[kRankMaxK];               // thresholds in the order of nbr
  __shared__ unsigned long long sorted[kRankMaxK];
  __shared__ int origin[kRankMaxK];                           // sorted place -> entry m
  __shared__ unsigned below[kRankMaxK];                       // elements below the t-th sorted threshold
  __shared__ int wsum[2 * (kRankThreads / 64)];
  __shared__ int nvalid;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int self = row0 + blockIdx.x;
  const float* row = strip + (size_t)blockIdx.x * N;
  const unsigned* keys = reinterpret_cast<const unsigned*>(row);

  for (int b = tid; b < k * kBinCopies; b += kRankThreads) bins[b] = 0;
  if (tid == 0) nvalid = 0;
  __syncthreads();
  if (tid < k) {
    const int j = nbr[(size_t)blockIdx.x * k + tid];
    const bool ok = j >= 0 && j < N && j != self;             // the guard: nothing is read for the other entries
    raw[tid] = ok ? (((unsigned long long)keys[j] << 32) | (unsigned)j) : kNoThreshold;
    if (ok) atomicAdd(&nvalid, 1);
  }
  __syncthreads();
  const int kv = nvalid;
  if (tid < k) {                                              // rank sort; equal keys (a column named twice, the guarded ones) by m
    const unsigned long long mine = raw[tid];
    int pos = 0;
    for (int t = 0; t < k; ++t) {
      const unsigned long long o = raw[t];
      pos += (o < mine) || (o == mine && t < tid);
    }
    sorted[pos] = mine;                                       // a real threshold is below kNoThreshold: its index is < N
    origin[pos] = tid;
  }
  __syncthreads();
  const unsigned long long top = kv > 0 ? sorted[kv - 1] : 0ull;
  const int copy = lane & (kBinCopies - 1);

  // the row: a head up to the first 16-byte boundary, 16-byte loads, a tail
  int head = (int)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) >> 2);
  if (head > N) head = N;
  const int nvec = (N - head) >> 2;
  if (tid < head) rank_place(keys[tid], tid, self, sorted, kv, top, bins, copy);
  const uint4* body = reinterpret_cast<const uint4*>(keys + head);
  for (int v = tid; v < nvec; v += kRankThreads) {
    const uint4 q = body[v];
    const int l = head + 4 * v;
    rank_place(q.x, l, self, sorted, kv, top, bins, copy);
    rank_place(q.y, l + 1, self, sorted, kv, top, bins, copy);
    rank_place(q.z, l + 2, self, sorted, kv, top, bins, copy);
    rank_place(q.w, l + 3, self, sorted, kv, top, bins, copy);
  }
  {
    const int l = head + 4 * nvec + tid;
    if (l < N) rank_place(keys[l], l, self, sorted, kv, top, bins, copy);
  }
  __syncthreads();

  unsigned c = 0;                                             // bin tid's count, copies folded
  if (tid < k) {
#pragma unroll
    for (int r = 0; r < kBinCopies; ++r) c += bins[tid * kBinCopies + r];
  }
  __syncthreads();
  bins[tid] = c;                                              // zero from k on
  __syncthreads();
  if (wave == 0) {                                            // lane l: bins 4l .. 4l + 3, inclusive prefix sums
    const unsigned c0 = bins[4 * lane], c1 = bins[4 * lane + 1], c2 = bins[4 * lane + 2], c3 = bins[4 * lane + 3];
    const unsigned s = c0 + c1 + c2 + c3;
    unsigned incl = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    const unsigned excl = incl - s;
    below[4 * lane] = excl + c0;
    below[4 * lane + 1] = excl + c0 + c1;
    below[4 * lane + 2] = excl + c0 + c1 + c2;
    below[4 * lane + 3] = incl;
  }
  __syncthreads();

  int penalty = 0, hit = 0;                                   // at most k (N - 1) <= 2^25: int is wide enough inside the row
  if (tid < k) {
    const int r = tid < kv ? 1 + (int)below[tid] : 0;
    rank[(size_t)blockIdx.x * k + origin[tid]] = r;
    penalty = r > k ? r - k : 0;
    hit = r >= 1 && r <= k;
  }
  penalty = wave_sum(penalty);
  hit = wave_sum(hit);
  if (lane == 0) {
    wsum[2 * wave] = penalty;
    wsum[2 * wave + 1] = hit;
  }
  __syncthreads();
  if (tid < 2) {
    long long s = 0;
#pragma unroll
    for (int w = 0; w < kRankThreads / 64; ++w) s += wsum[2 * w + tid];
    sums[(size_t)blockIdx.x * 2 + tid] = s;
  }
}

}  // namespace evae

using namespace evae;

extern "C" size_t evae_nn_rank_workspace_bytes(int N, int strip_rows) {
  return evae_tsne_knn_workspace_bytes(N, strip_rows);
}

extern "C" int evae_nn_rank(const float* z, int N, int zdim, const int* nbr, int k, int strip_rows, int* rank, long long* row_sums,
                            void* ws, size_t ws_bytes, evae_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int max_points = evae_tsne_nn_max_points(), max_k = evae_tsne_nn_max_neighbours();
  static_assert(kRankThreads == kRankMaxK && kRankMaxK == 4 * 64, "one thread per threshold, 4 bins per lane of the scan");
  EVAE_REQUIRE(max_k <= kRankMaxK, "nn_rank: built for up to %d neighbours, the neighbour search gives %d", kRankMaxK, max_k);
  EVAE_REQUIRE(N >= 2 && N <= max_points, "nn_rank: N=%d outside [2, %d]", N, max_points);
  EVAE_REQUIRE(zdim > 0, "nn_rank: zdim=%d", zdim);
  EVAE_REQUIRE(k >= 1 && k <= max_k, "nn_rank: k=%d outside [1, %d]", k, max_k);
  EVAE_REQUIRE(k <= N - 1, "nn_rank: k=%d but a point has only N - 1 = %d neighbours", k, N - 1);
  EVAE_REQUIRE(strip_rows >= 0, "nn_rank: strip_rows=%d (0 = automatic)", strip_rows);
  EVAE_REQUIRE(z && nbr && rank && row_sums && ws, "nn_rank: null pointer");
  EVAE_REQUIRE(((uintptr_t)ws & 3) == 0 && ((uintptr_t)row_sums & 7) == 0, "nn_rank: misaligned workspace or row_sums");
  const int R = strip_rows_of(N, strip_rows);               // the strip of the neighbour search, by its own rule
  EVAE_REQUIRE(ws_bytes >= (size_t)R * (size_t)N * sizeof(float), "nn_rank: workspace of %zu bytes, %zu needed", ws_bytes,
               (size_t)R * (size_t)N * sizeof(float));
  float* strip = static_cast<float*>(ws);
  return for_each_strip(z, N, zdim, R, strip, stream_, [&](int r0, int rows) {
    nn_rank_count_kernel<<<rows, kRankThreads, 0, stream>>>(strip, N, r0, k, nbr + (size_t)r0 * k, rank + (size_t)r0 * k,
                                                            row_sums + (size_t)r0 * 2);
    return check_launch("nn_rank_count_kernel");
  });
}
