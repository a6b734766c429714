// Ball counts and nearest columns between two sets of rows on gfx950: for every query q_i and all columns c_j, how many
// distances D(q_i, c_j) lie strictly below the column's radius, how many strictly below the row's radius, and the column that
// minimises (D(q_i, c_j), j) -- the integers that precision, recall, density, coverage and authenticity of generated samples
// are sums of (evae/sample_quality.py; DESIGN 3.7f has the definitions, the launch sequence and the traffic).  No [B x N]
// buffer exists at any point.
//
//   distances: the queries go in strips of R rows, as in evae_nn_rank; the strip's [R x N] distances come from
//              evae_pairwise_distance (fp64 accumulated, rounded once) into a workspace, so every comparison is on the values the
//              neighbour search made the radii from.
//   counting:  one workgroup per row.  The N distances stream through once: a head of scalars up to the row's first 16-byte
//              boundary (a row starts at i * N floats), 16-byte loads, a tail of scalars; the ragged ends are predicated, every
//              thread reaches every barrier.  Column j's radius sits at another phase of a 16-byte boundary than its distance, so
//              the radii are read as scalars (consecutive lanes, consecutive addresses; the [N] vector is shared by all rows and
//              stays in cache).  A thread keeps two integer counts and the unsigned minimum of (distance bits << 32) | j --
//              distances are >= 0, their bit patterns order as unsigned integers, the index in the low word breaks ties towards
//              the lower column.  Integer add and min only, over the wave by shuffles and over the four waves through LDS: the
//              result does not depend on which thread saw which column.
//   NaN:       finite inputs are the caller's contract.  A NaN distance or radius fails every `<`, so it is in no ball; a NaN's
//              bit pattern lies above +inf's, so it is the minimum only of a row whose distances are all NaN.
#include "evae_latent.h"

namespace evae {

constexpr int kBallThreads = 256;
constexpr unsigned long long kNoColumn = ~0ull;

struct BallAcc {
  int col = 0, row = 0;
  unsigned long long best = kNoColumn;
};

template <bool COL, bool NN>
__device__ __forceinline__ void ball_see(BallAcc& a, float v, int j, const float* __restrict__ col_radius, float rr) {
  if (COL) a.col += v < col_radius[j];
  a.row += v < rr;                                             // rr is NaN when the row count is off: never true
  if (NN) {
    const unsigned long long e = ((unsigned long long)__float_as_uint(v) << 32) | (unsigned)j;
    a.best = e < a.best ? e : a.best;
  }
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned hi = __shfl_xor((unsigned)(v >> 32), o, 64), lo = __shfl_xor((unsigned)v, o, 64);
    const unsigned long long t = ((unsigned long long)hi << 32) | lo;
    v = t < v ? t : v;
  }
  return v;
}

// strip: [rows x N] distances of the query rows row0 .. ; the outputs and row_radius are already offset to row0
template <bool COL, bool NN>
__global__ __launch_bounds__(kBallThreads) void ball_count_kernel(const float* __restrict__ strip, int N,
                                                                   const float* __restrict__ col_radius,
                                                                   const float* __restrict__ row_radius, int* __restrict__ col_hits,
                                                                   int* __restrict__ row_hits, int* __restrict__ nn_idx,
                                                                   float* __restrict__ nn_d2) {
  __shared__ int wcol[kBallThreads / 64], wrow[kBallThreads / 64];
  __shared__ unsigned long long wbest[kBallThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* row = strip + (size_t)blockIdx.x * N;
  const float rr = row_radius ? row_radius[blockIdx.x] : __uint_as_float(0x7fc00000u);
  BallAcc a;

  int head = (int)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) >> 2);
  if (head > N) head = N;
  const int nvec = (N - head) >> 2;
  if (tid < head) ball_see<COL, NN>(a, row[tid], tid, col_radius, rr);
  const float4* body = reinterpret_cast<const float4*>(row + head);
#pragma unroll 4
  for (int v = tid; v < nvec; v += kBallThreads) {
    const float4 q = body[v];
    const int j = head + 4 * v;
    ball_see<COL, NN>(a, q.x, j, col_radius, rr);
    ball_see<COL, NN>(a, q.y, j + 1, col_radius, rr);
    ball_see<COL, NN>(a, q.z, j + 2, col_radius, rr);
    ball_see<COL, NN>(a, q.w, j + 3, col_radius, rr);
  }
  {
    const int j = head + 4 * nvec + tid;                       // fewer than 4 of them
    if (j < N) ball_see<COL, NN>(a, row[j], j, col_radius, rr);
  }

  a.col = wave_sum(a.col);
  a.row = wave_sum(a.row);
  if (NN) a.best = wave_min_u64(a.best);
  if (lane == 0) {
    wcol[wave] = a.col;
    wrow[wave] = a.row;
    wbest[wave] = a.best;
  }
  __syncthreads();
  if (tid == 0) {
    int c = 0, r = 0;
    unsigned long long b = kNoColumn;
#pragma unroll
    for (int w = 0; w < kBallThreads / 64; ++w) {
      c += wcol[w];
      r += wrow[w];
      b = wbest[w] < b ? wbest[w] : b;
    }
    if (COL) col_hits[blockIdx.x] = c;
    if (row_hits) row_hits[blockIdx.x] = r;
    if (NN) {
      if (nn_idx) nn_idx[blockIdx.x] = (int)(unsigned)b;       // N >= 1: some column was seen
      if (nn_d2) nn_d2[blockIdx.x] = __uint_as_float((unsigned)(b >> 32));
    }
  }
}

}  // namespace evae

using namespace evae;

extern "C" int evae_ball_count_max_points(void) { return evae_tsne_nn_max_points(); }

extern "C" size_t evae_ball_count_workspace_bytes(int B, int N, int strip_rows) {
  if (B < 1 || N < 1) return 0;
  return (size_t)cross_strip_rows_of(B, N, strip_rows) * (size_t)N * sizeof(float);
}

extern "C" int evae_ball_count(const float* q, int B, const float* c, int N, int d, const float* col_radius,
                               const float* row_radius, int strip_rows, int* col_hits, int* row_hits, int* nn_idx, float* nn_d2,
                               void* ws, size_t ws_bytes, evae_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int max_points = evae_ball_count_max_points();
  EVAE_REQUIRE(B >= 1 && B <= max_points, "ball_count: B=%d outside [1, %d]", B, max_points);
  EVAE_REQUIRE(N >= 1 && N <= max_points, "ball_count: N=%d outside [1, %d]", N, max_points);
  EVAE_REQUIRE(d >= 1, "ball_count: d=%d", d);
  EVAE_REQUIRE(strip_rows >= 0, "ball_count: strip_rows=%d (0 = automatic)", strip_rows);
  EVAE_REQUIRE((col_radius != nullptr) == (col_hits != nullptr), "ball_count: col_hits and col_radius go together (%s given alone)",
               col_radius ? "col_radius" : "col_hits");
  EVAE_REQUIRE((row_radius != nullptr) == (row_hits != nullptr), "ball_count: row_hits and row_radius go together (%s given alone)",
               row_radius ? "row_radius" : "row_hits");
  EVAE_REQUIRE(col_hits || row_hits || nn_idx || nn_d2, "ball_count: no output asked for");
  EVAE_REQUIRE(q && c && ws, "ball_count: null pointer");
  EVAE_REQUIRE(((uintptr_t)ws & 3) == 0, "ball_count: misaligned workspace");
  const int R = cross_strip_rows_of(B, N, strip_rows);
  EVAE_REQUIRE(ws_bytes >= (size_t)R * (size_t)N * sizeof(float), "ball_count: workspace of %zu bytes, %zu needed", ws_bytes,
               (size_t)R * (size_t)N * sizeof(float));
  float* strip = static_cast<float*>(ws);
  const bool col = col_radius != nullptr, nn = nn_idx || nn_d2;
  return for_each_cross_strip(q, B, c, N, d, R, strip, stream_, [&](int r0, int rows) {
    const float* rrad = row_radius ? row_radius + r0 : nullptr;
    int* ch = col_hits ? col_hits + r0 : nullptr;
    int* rh = row_hits ? row_hits + r0 : nullptr;
    int* ni = nn_idx ? nn_idx + r0 : nullptr;
    float* nd = nn_d2 ? nn_d2 + r0 : nullptr;
#define EVAE_BALL_LAUNCH(COL_, NN_) \
  ball_count_kernel<COL_, NN_><<<rows, kBallThreads, 0, stream>>>(strip, N, col_radius, rrad, ch, rh, ni, nd)
    if (col && nn) EVAE_BALL_LAUNCH(true, true);
    else if (col) EVAE_BALL_LAUNCH(true, false);
    else if (nn) EVAE_BALL_LAUNCH(false, true);
    else EVAE_BALL_LAUNCH(false, false);
#undef EVAE_BALL_LAUNCH
    return check_launch("ball_count_kernel");
  });
}
