// k-means of the latent space and clustering scores on gfx950, all arithmetic in fp64 (evae/cluster.py; DESIGN 3.7d has the
// formulas, the order of every sum and the measurements).  The only atomics are integer ones (counts, an index minimum): every
// floating-point sum has a fixed order, so equal inputs give bit-equal outputs.
//
//   assign:   a block owns kAssignRows rows, staged in LDS as fp32 with an odd row stride; the centres pass through LDS in tiles
//             of kKmTile rows as fp64.  Thread (row, group g) holds kPerThread running sums -- the centres g, g + 4, .. of the
//             tile -- so a row's value is read once for eight differences and a centre's value is a wave-wide broadcast.
//             sum_k (x_ik - c_jk)^2 by fma, k ascending; strict "<" in ascending j, then the four groups of a row merged on
//             (value, index): ties go to the lowest centre.  No atomics.  transform is the same kernel writing
//             sqrt of every sum, rounded once to fp32, instead of the winner.
//   update:   hist (a block per chunk of kKmChunk rows, integer LDS atomics; the chunk's sum of d2 on the way) -> scan (one
//             workgroup: thread c totals cluster c over the chunks, a block scan over c, then the chunk offsets of c in place)
//             -> place (a block per chunk: a row's place is the number of earlier rows of the chunk with its label, counted
//             against the chunk's labels in LDS) -> segsum (a block per segment of kKmChunk positions of the order: every run
//             of one cluster in it, columns across threads, rows g, g + G, .. per thread and the G partial sums in order of g,
//             to slot segment + cluster) -> sums (cluster c's slots in segment order).
//   finish:   ONE workgroup: counts, the empty-cluster rule (a pass over d2 per empty cluster; a taken point's d2 is parked at
//             -1 and restored), centres = sum / count, the shift, the inertia (chunk sums added in chunk order), the record.
//   Every kernel of a step starts with `if (state[1] != 0) return` -- the same value in every thread of the grid, written by
//   an EARLIER launch of the stream: nothing polls, nothing waits on another workgroup.
//   seed:     dist (a block per chunk: distance to the last pick, d2min, the chunk's running sums added by one thread in index
//             order) -> pick (one workgroup: chunk bases in order, the first chunk and then the first row above u_t total).
//   scores:   contingency by int64 atomics; scores in one workgroup (row and column sums, pair counts and the purity as exact
//             integers; entropies and MI per thread in entry order, then a fixed tree through LDS).
//   silhouette: x[order] gathered once; per strip evae_pairwise_distance and one wave per row over the clusters' segments.
#include "evae_latent.h"

namespace evae {

constexpr int kKmMaxK = 1024;
constexpr int kKmMaxD = 256;
constexpr int kKmMaxN = 1 << 20;
constexpr int kKmChunk = 512;
constexpr int kKmTile = 32;
constexpr int kKmThreads = 256;
constexpr int kAssignRows = 64;                             // one wave of rows
constexpr int kAssignGroups = kKmThreads / kAssignRows;     // 4
constexpr int kPerThread = kKmTile / kAssignGroups;         // 8 centres of a tile per thread
constexpr int kOneThreads = 1024;                           // the one-workgroup kernels
constexpr int kMaxChunks = kKmMaxN / kKmChunk;              // 2048
constexpr int kStateDoubles = 8;

static_assert(kOneThreads >= kKmMaxK, "one thread per cluster in the one-workgroup kernels");
static_assert(kKmMaxD <= kKmThreads, "pow2_width(d, kKmThreads) is never capped");

// a fixed tree through LDS over the kOneThreads threads of a one-workgroup kernel (double or long long); the buffer is free
// again on return
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* buf) {
  const int tid = threadIdx.x;
  buf[tid] = v;
  __syncthreads();
  for (int s = kOneThreads / 2; s > 0; s >>= 1) {
    if (tid < s) buf[tid] += buf[tid + s];
    __syncthreads();
  }
  const T r = buf[0];
  __syncthreads();
  return r;
}

// ---------------------------------------------------------------- assign
static size_t assign_lds_bytes(int d) { return (size_t)kKmTile * d * sizeof(double) + (size_t)kAssignRows * (d | 1) * sizeof(float); }

__global__ __launch_bounds__(kKmThreads) void kmeans_assign_kernel(const float* __restrict__ x, int N, int d,
                                                                   const double* __restrict__ centres, int K, int* labels,
                                                                   double* __restrict__ d2, int* __restrict__ changed,
                                                                   float* __restrict__ dist, const double* state) {
  if (step_done(state)) return;
  extern __shared__ __attribute__((aligned(16))) double km_smem[];
  __shared__ double best_v[kKmThreads];
  __shared__ int best_j[kKmThreads];
  double* ct = km_smem;                                            // [kKmTile x d]
  float* xr = reinterpret_cast<float*>(ct + (size_t)kKmTile * d);  // [kAssignRows x ldx]
  const int tid = threadIdx.x, r = tid & (kAssignRows - 1), g = tid / kAssignRows;
  const int r0 = blockIdx.x * kAssignRows, rows = min(kAssignRows, N - r0), ldx = d | 1;
  for (int e = tid; e < kAssignRows * d; e += kKmThreads) {
    const int rr = e / d, k = e - rr * d;
    xr[rr * ldx + k] = rr < rows ? x[(size_t)r0 * d + e] : 0.f;
  }
  double bv = INFINITY;
  int bj = kNoIndex;
  const float* xrow = xr + r * ldx;
  for (int t0 = 0; t0 < K; t0 += kKmTile) {
    __syncthreads();                                               // the rows are staged; the last tile has been read
    for (int e = tid; e < kKmTile * d; e += kKmThreads) ct[e] = t0 + e / d < K ? centres[(size_t)t0 * d + e] : 0.0;
    __syncthreads();
    double acc[kPerThread];
#pragma unroll
    for (int u = 0; u < kPerThread; ++u) acc[u] = 0.0;
    const double* cg = ct + g * d;
    for (int k = 0; k < d; ++k) {
      const double xv = (double)xrow[k];
#pragma unroll
      for (int u = 0; u < kPerThread; ++u) {
        const double df = xv - cg[u * kAssignGroups * d + k];
        acc[u] = fma(df, df, acc[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < kPerThread; ++u) {
      const int j = t0 + g + kAssignGroups * u;                    // ascending in u and in t0: "<" keeps the lowest
      if (dist && j < K && r < rows) dist[(size_t)(r0 + r) * K + j] = (float)sqrt(acc[u]);
      if (j < K && acc[u] < bv) {
        bv = acc[u];
        bj = j;
      }
    }
  }
  best_v[tid] = bv;
  best_j[tid] = bj;
  __syncthreads();
  if (g == 0) {                                                    // wave 0: one lane per row
#pragma unroll
    for (int h = 1; h < kAssignGroups; ++h) {
      const double v = best_v[h * kAssignRows + r];
      const int j = best_j[h * kAssignRows + r];
      if (v < bv || (v == bv && j < bj)) {
        bv = v;
        bj = j;
      }
    }
    if (bj == kNoIndex) bj = 0;                                    // a row of NaNs
    int ch = 0;
    if (r < rows) {
      const int i = r0 + r;
      // the first step has no previous labels (the buffer holds whatever it held): every row counts as changed
      if (changed) ch = (state && state[0] == 0.0) ? 1 : labels[i] != bj;
      if (labels) labels[i] = bj;
      if (d2) d2[i] = bv;
    }
    if (changed) {
      ch = wave_sum(ch);
      if (r == 0) changed[blockIdx.x] = ch;
    }
  }
}

// ---------------------------------------------------------------- update
__global__ __launch_bounds__(kKmThreads) void kmeans_hist_kernel(const int* __restrict__ labels, int N, int K,
                                                                 const double* __restrict__ d2, int* __restrict__ hist,
                                                                 double* __restrict__ chunk_sum, const double* state) {
  if (step_done(state)) return;
  __shared__ int h[kKmMaxK];
  __shared__ double wpart[kKmThreads / 64];
  const int tid = threadIdx.x, c0 = blockIdx.x * kKmChunk, c1 = min(N, c0 + kKmChunk);
  for (int j = tid; j < K; j += kKmThreads) h[j] = 0;
  __syncthreads();
  double s = 0.0;
  for (int i = c0 + tid; i < c1; i += kKmThreads) {
    const int l = labels[i];
    if ((unsigned)l < (unsigned)K) atomicAdd(&h[l], 1);
    if (d2) s += d2[i];
  }
  __syncthreads();
  for (int j = tid; j < K; j += kKmThreads) hist[(size_t)blockIdx.x * K + j] = h[j];
  if (d2) chunk_sum_store(s, wpart, chunk_sum + blockIdx.x);       // the same in every thread
}

// hist [chunks x K]: counts in, first positions out (cluster-major, then chunk); start [K + 1]
__global__ __launch_bounds__(kOneThreads) void kmeans_scan_kernel(int* __restrict__ hist, int chunks, int K,
                                                                  int* __restrict__ start, const double* state) {
  if (step_done(state)) return;
  __shared__ int wtot[kOneThreads / 64];
  const int c = threadIdx.x, lane = c & 63, wave = c >> 6;
  int t = 0;
  if (c < K)
    for (int ch = 0; ch < chunks; ++ch) t += hist[(size_t)ch * K + c];
  int incl = t;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  if (lane == 63) wtot[wave] = incl;
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; ++w) base += wtot[w];
  if (c < K) {
    int run = base + incl - t;
    start[c] = run;
    if (c == K - 1) start[K] = run + t;
    for (int ch = 0; ch < chunks; ++ch) {
      const int n = hist[(size_t)ch * K + c];
      hist[(size_t)ch * K + c] = run;
      run += n;
    }
  }
}

__global__ __launch_bounds__(kKmThreads) void kmeans_place_kernel(const int* __restrict__ labels, int N, int K,
                                                                  const int* __restrict__ offs, int* __restrict__ order,
                                                                  const double* state) {
  if (step_done(state)) return;
  constexpr int kOwn = kKmChunk / kKmThreads;
  __shared__ int lab[kKmChunk];
  const int tid = threadIdx.x, c0 = blockIdx.x * kKmChunk, n = min(kKmChunk, N - c0);
  for (int e = tid; e < kKmChunk; e += kKmThreads) lab[e] = e < n ? labels[c0 + e] : -1;
  __syncthreads();
  int mine[kOwn], pos[kOwn];
#pragma unroll
  for (int u = 0; u < kOwn; ++u) {
    mine[u] = lab[tid + u * kKmThreads];
    pos[u] = 0;
  }
  for (int e = 0; e < n; ++e) {
    const int l = lab[e];                                          // a broadcast
#pragma unroll
    for (int u = 0; u < kOwn; ++u) pos[u] += (l == mine[u]) & (e < tid + u * kKmThreads);
  }
#pragma unroll
  for (int u = 0; u < kOwn; ++u) {
    const int r = tid + u * kKmThreads;
    if (r < n && (unsigned)mine[u] < (unsigned)K) order[offs[(size_t)blockIdx.x * K + mine[u]] + pos[u]] = c0 + r;
  }
}

__global__ __launch_bounds__(kKmThreads) void kmeans_segsum_kernel(const float* __restrict__ x, int N, int d, int W, int K,
                                                                   const int* __restrict__ order, const int* __restrict__ start,
                                                                   double* __restrict__ partial, const double* state) {
  if (step_done(state)) return;
  __shared__ double part[kKmThreads];
  const int tid = threadIdx.x, c = tid & (W - 1), g = tid / W, G = kKmThreads / W;
  const int total = min(start[K], N);
  const int p0 = blockIdx.x * kKmChunk, p1 = min(total, p0 + kKmChunk);
  if (p0 >= p1) return;                                            // the same in every thread
  int lo = 0, hi = K - 1;                                          // the first cluster that ends after p0
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (start[mid + 1] > p0) hi = mid; else lo = mid + 1;
  }
  for (int cl = lo; cl < K; ++cl) {
    const int s0 = start[cl], s1 = start[cl + 1];
    if (s0 >= p1) break;
    const int a = max(p0, s0), b = min(p1, s1);
    if (a >= b) continue;                                          // an empty cluster
    double s = 0.0;
    if (c < d) {
#pragma unroll 4
      for (int p = a + g; p < b; p += G) {
        const int i = order[p];
        s += (unsigned)i < (unsigned)N ? (double)x[(size_t)i * d + c] : 0.0;
      }
    }
    const bool owner = g == 0 && c < d;
    const double t = group_fold(s, part, c, W, G, owner);
    if (owner) partial[((size_t)blockIdx.x + cl) * d + c] = t;
    __syncthreads();
  }
}

__global__ __launch_bounds__(kKmThreads) void kmeans_sums_kernel(const double* __restrict__ partial, const int* __restrict__ start,
                                                                 int K, int d, double* __restrict__ sums, const double* state) {
  if (step_done(state)) return;
  const int idx = blockIdx.x * kKmThreads + threadIdx.x;
  if (idx >= K * d) return;
  const int cl = idx / d, c = idx - cl * d;
  const int a = start[cl], b = start[cl + 1];
  double t = 0.0;
  if (a < b)
    for (int s = a / kKmChunk; s <= (b - 1) / kKmChunk; ++s) t += partial[((size_t)s + cl) * d + c];
  sums[idx] = t;
}

// ---------------------------------------------------------------- finish
__global__ __launch_bounds__(kOneThreads) void kmeans_finish_kernel(const float* __restrict__ x, int N, int d, int K,
                                                                    const int* __restrict__ labels, double* d2,
                                                                    const int* __restrict__ start, double* sums, double* centres,
                                                                    const int* __restrict__ changed, int nchanged,
                                                                    const double* __restrict__ chunk_sum, int chunks,
                                                                    double tol_abs, double* state) {
  if (step_done(state)) return;
  __shared__ int cnt[kKmMaxK];
  __shared__ int taken_i[kKmMaxK];
  __shared__ double taken_v[kKmMaxK];
  __shared__ double red_v[kOneThreads];
  __shared__ long long red_l[kOneThreads];
  __shared__ int red_i[kOneThreads];
  const int tid = threadIdx.x;
  for (int c = tid; c < K; c += kOneThreads) cnt[c] = start[c + 1] - start[c];
  long long ch = 0;
  for (int b = tid; b < nchanged; b += kOneThreads) ch += changed[b];
  const long long n_changed = block_sum(ch, red_l);                // (its barriers also publish cnt)

  // the empty-cluster rule
  int nreloc = 0;
  for (int e = 0; e < K; ++e) {
    if (cnt[e] != 0) continue;                                     // LDS, behind a barrier: the same in every thread
    double bv = -1.0;
    int bi = kNoIndex;
    for (int i = tid; i < N; i += kOneThreads) {                   // ascending i, ">": the lowest index of the largest d2
      const double v = d2[i];
      if (v > bv) {
        const int l = labels[i];
        if ((unsigned)l < (unsigned)K && cnt[l] >= 2) {
          bv = v;
          bi = i;
        }
      }
    }
    red_v[tid] = bv;
    red_i[tid] = bi;
    __syncthreads();
    for (int s = kOneThreads / 2; s > 0; s >>= 1) {
      if (tid < s) {
        const double v = red_v[tid + s];
        const int i = red_i[tid + s];
        if (v > red_v[tid] || (v == red_v[tid] && i < red_i[tid])) {
          red_v[tid] = v;
          red_i[tid] = i;
        }
      }
      __syncthreads();
    }
    const int pick = red_i[0];
    const double pv = red_v[0];
    __syncthreads();
    if (pick == kNoIndex) continue;                                   // no donor (cannot happen while K <= N)
    const int donor = labels[pick];
    for (int c = tid; c < d; c += kOneThreads) {
      const double xv = (double)x[(size_t)pick * d + c];
      sums[(size_t)donor * d + c] -= xv;
      sums[(size_t)e * d + c] = xv;
    }
    if (tid == 0) {
      taken_i[nreloc] = pick;
      taken_v[nreloc] = pv;
      d2[pick] = -1.0;                                             // never the largest again; restored below
      cnt[donor] -= 1;
      cnt[e] = 1;
    }
    ++nreloc;
    __syncthreads();
  }
  for (int t = tid; t < nreloc; t += kOneThreads) d2[taken_i[t]] = taken_v[t];
  __syncthreads();

  double sh = 0.0;
  for (int idx = tid; idx < K * d; idx += kOneThreads) {
    const int n = cnt[idx / d];
    if (n > 0) {
      const double cn = sums[idx] / (double)n;
      const double df = cn - centres[idx];
      sh = fma(df, df, sh);
      centres[idx] = cn;
    }
  }
  const double shift = block_sum(sh, red_v);

  const double inertia = ordered_total<kOneThreads>(chunk_sum, chunks, red_v);   // thread 0's
  if (tid == 0) {
    const double it = state[0] + 1.0;
    const bool done = (it > 1.0 && n_changed == 0) || shift <= tol_abs;
    state[0] = it;
    state[1] = done ? 1.0 : 0.0;
    state[2] = (double)n_changed;
    state[3] = shift;
    state[4] = inertia;
    state[5] += (double)nreloc;
    state[6] = (double)nreloc;
    state[7] = 0.0;
  }
}

// ---------------------------------------------------------------- inertia of a stand-alone assign
__global__ __launch_bounds__(kKmThreads) void kmeans_chunk_sum_kernel(const double* __restrict__ d2, int N,
                                                                      double* __restrict__ chunk_sum) {
  __shared__ double wpart[kKmThreads / 64];
  const int tid = threadIdx.x, c0 = blockIdx.x * kKmChunk, c1 = min(N, c0 + kKmChunk);
  double s = 0.0;
  for (int i = c0 + tid; i < c1; i += kKmThreads) s += d2[i];
  chunk_sum_store(s, wpart, chunk_sum + blockIdx.x);
}

__global__ __launch_bounds__(kOneThreads) void kmeans_total_kernel(const double* __restrict__ chunk_sum, int chunks,
                                                                   double* __restrict__ out) {
  __shared__ double buf[kOneThreads];
  const double total = ordered_total<kOneThreads>(chunk_sum, chunks, buf);
  if (threadIdx.x == 0) out[0] = total;
}

// ---------------------------------------------------------------- seed
__global__ __launch_bounds__(kKmThreads) void kmeans_seed_first_kernel(const float* __restrict__ x, int N, int d,
                                                                       const double* __restrict__ u, int* __restrict__ idx,
                                                                       double* __restrict__ centres) {
  const double f = floor(u[0] * (double)N);
  const int i = !(f >= 0.0) ? 0 : (f >= (double)N ? N - 1 : (int)f);
  if (threadIdx.x == 0) idx[0] = i;
  for (int c = threadIdx.x; c < d; c += kKmThreads) centres[c] = (double)x[(size_t)i * d + c];
}

__global__ __launch_bounds__(kKmThreads) void kmeans_seed_dist_kernel(const float* __restrict__ x, int N, int d,
                                                                      const int* __restrict__ idx, int t, double* __restrict__ d2min,
                                                                      double* __restrict__ prefix, double* __restrict__ totals) {
  __shared__ double pick[kKmMaxD];
  __shared__ double v[kKmChunk];
  const int tid = threadIdx.x, c0 = blockIdx.x * kKmChunk, n = min(kKmChunk, N - c0);
  int last = idx[t - 1];
  last = min(max(last, 0), N - 1);
  for (int c = tid; c < d; c += kKmThreads) pick[c] = (double)x[(size_t)last * d + c];
  __syncthreads();
  for (int e = tid; e < n; e += kKmThreads) {
    const float* xi = x + (size_t)(c0 + e) * d;
    double s = 0.0;
    for (int k = 0; k < d; ++k) {
      const double df = (double)xi[k] - pick[k];
      s = fma(df, df, s);
    }
    if (t > 1) s = fmin(s, d2min[c0 + e]);
    d2min[c0 + e] = s;
    v[e] = s;
  }
  __syncthreads();
  if (tid == 0) {                                                  // the running sums of the chunk, in index order
    double run = 0.0;
    for (int e = 0; e < n; ++e) {
      run += v[e];
      v[e] = run;
    }
    totals[blockIdx.x] = run;
  }
  __syncthreads();
  for (int e = tid; e < n; e += kKmThreads) prefix[c0 + e] = v[e];
}

__global__ __launch_bounds__(kOneThreads) void kmeans_seed_pick_kernel(const float* __restrict__ x, int N, int d, int t,
                                                                       const double* __restrict__ u,
                                                                       const double* __restrict__ prefix,
                                                                       const double* __restrict__ totals, int chunks,
                                                                       int* idx, double* __restrict__ centres) {
  __shared__ double base[kMaxChunks + 1];                          // base[ch]: the chunks before ch, added in order
  __shared__ int chunk_s, pick_s;
  const int tid = threadIdx.x;
  for (int ch = tid; ch < chunks; ch += kOneThreads) base[ch + 1] = totals[ch];
  if (tid == 0) {
    chunk_s = kNoIndex;
    pick_s = kNoIndex;
  }
  __syncthreads();
  if (tid == 0) {
    double run = 0.0;
    for (int ch = 0; ch < chunks; ++ch) {
      const double tot = base[ch + 1];
      base[ch] = run;
      run += tot;
    }
    base[chunks] = run;
  }
  __syncthreads();
  const double total = base[chunks];
  int pick;
  if (total > 0.0) {                                               // the same in every thread
    const double target = u[t] * total;
    for (int ch = tid; ch < chunks; ch += kOneThreads)
      if (base[ch + 1] > target) atomicMin(&chunk_s, ch);          // base[ch + 1] == base[ch] + the chunk's last running sum
    __syncthreads();
    const int ch = chunk_s;
    if (ch != kNoIndex) {
      const int c0 = ch * kKmChunk, n = min(kKmChunk, N - c0);
      for (int e = tid; e < n; e += kOneThreads)
        if (base[ch] + prefix[c0 + e] > target) atomicMin(&pick_s, c0 + e);
    }
    __syncthreads();
    pick = pick_s == kNoIndex ? N - 1 : pick_s;
  } else {                                                         // fewer distinct points than centres: the lowest unused index
    for (int j = tid; j <= t && j < N; j += kOneThreads) {
      bool used = false;
      for (int m = 0; m < t; ++m) used |= idx[m] == j;
      if (!used) atomicMin(&pick_s, j);
    }
    __syncthreads();
    pick = pick_s == kNoIndex ? N - 1 : pick_s;
  }
  __syncthreads();
  if (tid == 0) idx[t] = pick;
  for (int c = tid; c < d; c += kOneThreads) centres[(size_t)t * d + c] = (double)x[(size_t)pick * d + c];
}

// ---------------------------------------------------------------- scores
__global__ __launch_bounds__(kKmThreads) void cluster_contingency_kernel(const int* __restrict__ a, int Ka,
                                                                         const int* __restrict__ b, int Kb, int N,
                                                                         unsigned long long* table) {
  const int i = blockIdx.x * kKmThreads + threadIdx.x;
  if (i >= N) return;
  const int ai = a[i], bi = b[i];
  if ((unsigned)ai < (unsigned)Ka && (unsigned)bi < (unsigned)Kb) atomicAdd(&table[(size_t)ai * Kb + bi], 1ull);
}

__global__ __launch_bounds__(kOneThreads) void cluster_scores_kernel(const long long* __restrict__ table, int Ka, int Kb,
                                                                     double* __restrict__ out) {
  __shared__ long long ra[kKmMaxK];
  __shared__ long long cb[kKmMaxK];
  __shared__ double red_v[kOneThreads];
  __shared__ long long red_l[kOneThreads];
  const int tid = threadIdx.x;
  long long rs = 0, cs = 0, cm = 0;
  if (tid < Ka)
    for (int j = 0; j < Kb; ++j) rs += table[(size_t)tid * Kb + j];
  if (tid < Kb)
    for (int i = 0; i < Ka; ++i) {
      const long long v = table[(size_t)i * Kb + tid];
      cs += v;
      cm = v > cm ? v : cm;
    }
  ra[tid] = rs;
  cb[tid] = cs;
  long long sq = 0;
  for (int e = tid; e < Ka * Kb; e += kOneThreads) {
    const long long v = table[e];
    sq += v * v;
  }
  const long long n = block_sum(rs, red_l);                        // (its barriers also publish ra and cb)
  const long long sum_a2 = block_sum(rs * rs, red_l), sum_b2 = block_sum(cs * cs, red_l);
  const long long ss = block_sum(sq, red_l), pure = block_sum(cm, red_l);
  const long long na = block_sum((long long)(rs > 0), red_l), nb = block_sum((long long)(cs > 0), red_l);
  if (n == 0) {                                                    // the same in every thread
    if (tid < 8) out[tid] = 0.0;
    return;
  }
  const double dn = (double)n;
  const double ha = block_sum(rs > 0 ? ((double)rs / dn) * log(dn / (double)rs) : 0.0, red_v);
  const double hb = block_sum(cs > 0 ? ((double)cs / dn) * log(dn / (double)cs) : 0.0, red_v);
  double m = 0.0;
  for (int e = tid; e < Ka * Kb; e += kOneThreads) {
    const long long v = table[e];
    if (v > 0) {
      const int i = e / Kb, j = e - i * Kb;                        // v n and a_i b_j are below 2^53: exact as doubles
      m += ((double)v / dn) * log((double)(v * n) / (double)(ra[i] * cb[j]));
    }
  }
  double mi = block_sum(m, red_v);
  if (tid == 0) {
    mi = mi > 0.0 ? mi : 0.0;
    double nmi;
    if (na == 1 && nb == 1) nmi = 1.0;
    else if (mi == 0.0) nmi = 0.0;
    else nmi = mi / (0.5 * (ha + hb));
    const long long tp = ss - n, fp = sum_b2 - ss, fn = sum_a2 - ss, tn = n * n - fp - fn - ss;
    double ari = 1.0;
    if (fn != 0 || fp != 0) {
      const double dtp = (double)tp, dfp = (double)fp, dfn = (double)fn, dtn = (double)tn;
      ari = 2.0 * (dtp * dtn - dfn * dfp) / ((dtp + dfn) * (dfn + dtn) + (dtp + dfp) * (dfp + dtn));
    }
    out[0] = ha;
    out[1] = hb;
    out[2] = mi;
    out[3] = nmi;
    out[4] = ari;
    out[5] = (double)pure / dn;
    out[6] = dn;
    out[7] = 0.0;
  }
}

// ---------------------------------------------------------------- silhouette
__global__ __launch_bounds__(kKmThreads) void silhouette_gather_kernel(const float* __restrict__ x, int N, int d,
                                                                       const int* __restrict__ order, float* __restrict__ xs) {
  const size_t e = (size_t)blockIdx.x * kKmThreads + threadIdx.x;
  if (e >= (size_t)N * d) return;
  const int p = (int)(e / d), c = (int)(e - (size_t)p * d);
  const int i = order[p];
  xs[e] = (unsigned)i < (unsigned)N ? x[(size_t)i * d + c] : 0.f;
}

// strip [rows x N]: squared distances of the points at positions row0 .. of the order to every position
__global__ __launch_bounds__(kKmThreads) void silhouette_reduce_kernel(const float* __restrict__ strip, int N, int row0, int rows,
                                                                       const int* __restrict__ order, const int* __restrict__ start,
                                                                       int K, double* __restrict__ out) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * (kKmThreads / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;                                           // by the wave; no barrier below
  const int p = row0 + r;
  const float* row = strip + (size_t)r * N;
  double own = 0.0, best = INFINITY;
  int n_own = 0;
  for (int c = 0; c < K; ++c) {
    const int a = max(start[c], 0), b = min(start[c + 1], N);
    if (a >= b) continue;
    double s = 0.0;
    for (int q = a + lane; q < b; q += 64) s += sqrt((double)row[q]);
    s = wave_sum(s);
    if (p >= a && p < b) {
      own = s;
      n_own = b - a;
    } else {
      best = fmin(best, s / (double)(b - a));
    }
  }
  if (lane == 0) {
    double sil = 0.0;
    if (n_own > 1 && best < INFINITY) {
      const double a = own / (double)(n_own - 1), m = fmax(a, best);
      if (m > 0.0) sil = (best - a) / m;
    }
    const int i = order[p];
    if ((unsigned)i < (unsigned)N) out[i] = sil;
  }
}

// ---------------------------------------------------------------- host side
struct KmLayout {
  size_t partial, sums, chunk_sum, d2min, prefix, totals, hist, changed, bytes;
};

static int km_chunks(int N) { return (N + kKmChunk - 1) / kKmChunk; }
static int km_blocks(int N) { return (N + kAssignRows - 1) / kAssignRows; }

static KmLayout km_layout(int N, int d, int K) {
  KmLayout w;
  WsCursor ws;
  const size_t chunks = (size_t)km_chunks(N);
  w.partial = ws.take((chunks + K) * d * sizeof(double));
  w.sums = ws.take((size_t)K * d * sizeof(double));
  w.chunk_sum = ws.take(chunks * sizeof(double));
  w.d2min = ws.take((size_t)N * sizeof(double));
  w.prefix = ws.take((size_t)N * sizeof(double));
  w.totals = ws.take(chunks * sizeof(double));
  w.hist = ws.take(chunks * K * sizeof(int));
  w.changed = ws.take((size_t)km_blocks(N) * sizeof(int));
  w.bytes = ws.o;
  return w;
}

static int km_assign_launch(const float* x, int N, int d, const double* centres, int K, int* labels, double* d2, int* changed,
                            float* dist, const double* state, hipStream_t stream) {
  constexpr int kMaxLds = kKmTile * kKmMaxD * (int)sizeof(double) + kAssignRows * (kKmMaxD | 1) * (int)sizeof(float);
  static_assert(kMaxLds + kKmThreads * 12 <= 160 * 1024, "a tile of centres and a block's rows fit the workgroup's LDS at d = 256");
  // Only a wide input (d > 64) needs more LDS than a launch gets unasked: the latents' d = 40 iterates without this host call.
  if (assign_lds_bytes(d) > 32 * 1024) {
    const int rc = set_max_lds((const void*)kmeans_assign_kernel, kMaxLds, "kmeans_assign");
    if (rc) return rc;
  }
  kmeans_assign_kernel<<<km_blocks(N), kKmThreads, assign_lds_bytes(d), stream>>>(x, N, d, centres, K, labels, d2, changed, dist,
                                                                                  state);
  return check_launch("kmeans_assign_kernel");
}

// hist .. sums: order, start and the cluster sums of `labels`
static int km_update_launch(const float* x, int N, int d, const int* labels, int K, const double* d2, int* order, int* start,
                            double* sums, char* ws, const KmLayout& w, const double* state, hipStream_t stream) {
  const int chunks = km_chunks(N);
  int* hist = reinterpret_cast<int*>(ws + w.hist);
  double* partial = reinterpret_cast<double*>(ws + w.partial);
  const int W = pow2_width(d, kKmThreads);
  kmeans_hist_kernel<<<chunks, kKmThreads, 0, stream>>>(labels, N, K, d2, hist, reinterpret_cast<double*>(ws + w.chunk_sum), state);
  int rc = check_launch("kmeans_hist_kernel");
  if (rc) return rc;
  kmeans_scan_kernel<<<1, kOneThreads, 0, stream>>>(hist, chunks, K, start, state);
  if ((rc = check_launch("kmeans_scan_kernel"))) return rc;
  kmeans_place_kernel<<<chunks, kKmThreads, 0, stream>>>(labels, N, K, hist, order, state);
  if ((rc = check_launch("kmeans_place_kernel"))) return rc;
  kmeans_segsum_kernel<<<chunks, kKmThreads, 0, stream>>>(x, N, d, W, K, order, start, partial, state);
  if ((rc = check_launch("kmeans_segsum_kernel"))) return rc;
  kmeans_sums_kernel<<<(K * d + kKmThreads - 1) / kKmThreads, kKmThreads, 0, stream>>>(partial, start, K, d, sums, state);
  return check_launch("kmeans_sums_kernel");
}

}  // namespace evae

using namespace evae;

extern "C" int evae_kmeans_max_clusters(void) { return kKmMaxK; }
extern "C" int evae_kmeans_max_features(void) { return kKmMaxD; }
extern "C" int evae_kmeans_max_points(void) { return kKmMaxN; }
extern "C" int evae_kmeans_chunk_rows(void) { return kKmChunk; }
extern "C" int evae_kmeans_centre_tile(void) { return kKmTile; }

extern "C" size_t evae_kmeans_workspace_bytes(int N, int d, int K) {
  if (N < 1 || d < 1 || K < 1) return 0;
  return km_layout(N, d, K).bytes;
}

#define KM_SIZES(who)                                                                               \
  EVAE_REQUIRE(N >= 1 && N <= kKmMaxN, who ": N=%d outside [1, %d]", N, kKmMaxN);                   \
  EVAE_REQUIRE(d >= 1 && d <= kKmMaxD, who ": d=%d outside [1, %d]", d, kKmMaxD);                   \
  EVAE_REQUIRE(K >= 1 && K <= kKmMaxK, who ": K=%d outside [1, %d]", K, kKmMaxK)

#define KM_WORKSPACE(who)                                                                           \
  EVAE_REQUIRE(ws && ((uintptr_t)ws & 255) == 0, who ": null or misaligned workspace");             \
  EVAE_REQUIRE(ws_bytes >= evae_kmeans_workspace_bytes(N, d, K), who ": workspace of %zu bytes, %zu needed", ws_bytes, \
               evae_kmeans_workspace_bytes(N, d, K))

extern "C" int evae_kmeans_assign(const float* x, int N, int d, const double* centres, int K, int* labels, double* d2,
                                  evae_stream_t stream_) {
  KM_SIZES("kmeans_assign");
  EVAE_REQUIRE(x && centres && labels && d2, "kmeans_assign: null pointer");
  EVAE_REQUIRE(aligned8(centres) && aligned8(d2), "kmeans_assign: misaligned centres or d2");
  return km_assign_launch(x, N, d, centres, K, labels, d2, nullptr, nullptr, nullptr, (hipStream_t)stream_);
}

extern "C" int evae_kmeans_transform(const float* x, int N, int d, const double* centres, int K, float* out, evae_stream_t stream_) {
  KM_SIZES("kmeans_transform");
  EVAE_REQUIRE(x && centres && out, "kmeans_transform: null pointer");
  EVAE_REQUIRE(aligned8(centres), "kmeans_transform: misaligned centres");
  return km_assign_launch(x, N, d, centres, K, nullptr, nullptr, nullptr, out, nullptr, (hipStream_t)stream_);
}

extern "C" int evae_kmeans_update(const float* x, int N, int d, const int* labels, int K, int* order, int* start, double* sums,
                                  void* ws, size_t ws_bytes, evae_stream_t stream_) {
  KM_SIZES("kmeans_update");
  EVAE_REQUIRE(x && labels && order && start && sums, "kmeans_update: null pointer");
  EVAE_REQUIRE(aligned8(sums), "kmeans_update: misaligned sums");
  KM_WORKSPACE("kmeans_update");
  return km_update_launch(x, N, d, labels, K, nullptr, order, start, sums, static_cast<char*>(ws), km_layout(N, d, K), nullptr,
                          (hipStream_t)stream_);
}

extern "C" int evae_kmeans_step(const float* x, int N, int d, int K, double* centres, int* labels, double* d2, int* order,
                                int* start, double tol_abs, double* state, void* ws, size_t ws_bytes, evae_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  KM_SIZES("kmeans_step");
  EVAE_REQUIRE(K <= N, "kmeans_step: K=%d centres for N=%d points", K, N);
  EVAE_REQUIRE(x && centres && labels && d2 && order && start && state, "kmeans_step: null pointer");
  EVAE_REQUIRE(aligned8(centres) && aligned8(d2) && aligned8(state), "kmeans_step: misaligned centres, d2 or state");
  EVAE_REQUIRE(tol_abs >= 0.0, "kmeans_step: tol_abs=%g", tol_abs);
  KM_WORKSPACE("kmeans_step");
  const KmLayout w = km_layout(N, d, K);
  char* base = static_cast<char*>(ws);
  int* changed = reinterpret_cast<int*>(base + w.changed);
  double* sums = reinterpret_cast<double*>(base + w.sums);
  int rc = km_assign_launch(x, N, d, centres, K, labels, d2, changed, nullptr, state, stream);
  if (rc) return rc;
  if ((rc = km_update_launch(x, N, d, labels, K, d2, order, start, sums, base, w, state, stream))) return rc;
  kmeans_finish_kernel<<<1, kOneThreads, 0, stream>>>(x, N, d, K, labels, d2, start, sums, centres, changed, km_blocks(N),
                                                      reinterpret_cast<const double*>(base + w.chunk_sum), km_chunks(N), tol_abs,
                                                      state);
  return check_launch("kmeans_finish_kernel");
}

extern "C" int evae_kmeans_seed(const float* x, int N, int d, int K, const double* u, int* idx, double* centres, void* ws,
                                size_t ws_bytes, evae_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  KM_SIZES("kmeans_seed");
  EVAE_REQUIRE(K <= N, "kmeans_seed: K=%d centres for N=%d points", K, N);
  EVAE_REQUIRE(x && u && idx && centres, "kmeans_seed: null pointer");
  EVAE_REQUIRE(aligned8(u) && aligned8(centres), "kmeans_seed: misaligned u or centres");
  KM_WORKSPACE("kmeans_seed");
  const KmLayout w = km_layout(N, d, K);
  char* base = static_cast<char*>(ws);
  double* d2min = reinterpret_cast<double*>(base + w.d2min);
  double* prefix = reinterpret_cast<double*>(base + w.prefix);
  double* totals = reinterpret_cast<double*>(base + w.totals);
  const int chunks = km_chunks(N);
  kmeans_seed_first_kernel<<<1, kKmThreads, 0, stream>>>(x, N, d, u, idx, centres);
  int rc = check_launch("kmeans_seed_first_kernel");
  for (int t = 1; t < K && !rc; ++t) {
    kmeans_seed_dist_kernel<<<chunks, kKmThreads, 0, stream>>>(x, N, d, idx, t, d2min, prefix, totals);
    if ((rc = check_launch("kmeans_seed_dist_kernel"))) break;
    kmeans_seed_pick_kernel<<<1, kOneThreads, 0, stream>>>(x, N, d, t, u, prefix, totals, chunks, idx, centres);
    rc = check_launch("kmeans_seed_pick_kernel");
  }
  return rc;
}

extern "C" int evae_kmeans_inertia(const double* d2, int N, double* out, void* ws, size_t ws_bytes, evae_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  EVAE_REQUIRE(N >= 1 && N <= kKmMaxN, "kmeans_inertia: N=%d outside [1, %d]", N, kKmMaxN);
  EVAE_REQUIRE(d2 && out && ws, "kmeans_inertia: null pointer");
  EVAE_REQUIRE(aligned8(d2) && aligned8(out) && aligned8(ws), "kmeans_inertia: misaligned pointer");
  const int chunks = km_chunks(N);
  EVAE_REQUIRE(ws_bytes >= (size_t)chunks * sizeof(double), "kmeans_inertia: workspace of %zu bytes, %zu needed", ws_bytes,
               (size_t)chunks * sizeof(double));
  double* chunk_sum = static_cast<double*>(ws);
  kmeans_chunk_sum_kernel<<<chunks, kKmThreads, 0, stream>>>(d2, N, chunk_sum);
  int rc = check_launch("kmeans_chunk_sum_kernel");
  if (rc) return rc;
  kmeans_total_kernel<<<1, kOneThreads, 0, stream>>>(chunk_sum, chunks, out);
  return check_launch("kmeans_total_kernel");
}

extern "C" int evae_cluster_contingency(const int* a, int Ka, const int* b, int Kb, int N, long long* table,
                                        evae_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  EVAE_REQUIRE(N >= 1 && N <= kKmMaxN, "cluster_contingency: N=%d outside [1, %d]", N, kKmMaxN);
  EVAE_REQUIRE(Ka >= 1 && Ka <= kKmMaxK && Kb >= 1 && Kb <= kKmMaxK, "cluster_contingency: %d x %d outside [1, %d]^2", Ka, Kb,
               kKmMaxK);
  EVAE_REQUIRE(a && b && table && aligned8(table), "cluster_contingency: null or misaligned pointer");
  const hipError_t e = hipMemsetAsync(table, 0, (size_t)Ka * Kb * sizeof(long long), stream);
  if (e != hipSuccess) {
    set_error("cluster_contingency: clearing the table: %s", hipGetErrorString(e));
    return EVAE_ELAUNCH;
  }
  cluster_contingency_kernel<<<(N + kKmThreads - 1) / kKmThreads, kKmThreads, 0, stream>>>(
      a, Ka, b, Kb, N, reinterpret_cast<unsigned long long*>(table));
  return check_launch("cluster_contingency_kernel");
}

extern "C" int evae_cluster_scores(const long long* table, int Ka, int Kb, double* out, evae_stream_t stream_) {
  EVAE_REQUIRE(Ka >= 1 && Ka <= kKmMaxK && Kb >= 1 && Kb <= kKmMaxK, "cluster_scores: %d x %d outside [1, %d]^2", Ka, Kb, kKmMaxK);
  EVAE_REQUIRE(table && out && aligned8(table) && aligned8(out), "cluster_scores: null or misaligned pointer");
  cluster_scores_kernel<<<1, kOneThreads, 0, (hipStream_t)stream_>>>(table, Ka, Kb, out);
  return check_launch("cluster_scores_kernel");
}

static size_t silhouette_rows_bytes(int N, int d) { return align_up((size_t)N * d * sizeof(float), 256); }

extern "C" size_t evae_silhouette_workspace_bytes(int N, int d, int strip_rows) {
  if (N < 1 || d < 1) return 0;
  return silhouette_rows_bytes(N, d) + evae_tsne_knn_workspace_bytes(N, strip_rows);
}

extern "C" int evae_silhouette_samples(const float* x, int N, int d, const int* order, const int* start, int K, double* out,
                                       void* ws, size_t ws_bytes, int strip_rows, evae_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int max_points = evae_tsne_nn_max_points();
  EVAE_REQUIRE(N >= 2 && N <= max_points, "silhouette_samples: N=%d outside [2, %d]", N, max_points);
  EVAE_REQUIRE(d >= 1 && d <= kKmMaxD, "silhouette_samples: d=%d outside [1, %d]", d, kKmMaxD);
  EVAE_REQUIRE(K >= 1 && K <= N, "silhouette_samples: K=%d outside [1, N = %d]", K, N);
  EVAE_REQUIRE(strip_rows >= 0, "silhouette_samples: strip_rows=%d (0 = automatic)", strip_rows);
  EVAE_REQUIRE(x && order && start && out && ws, "silhouette_samples: null pointer");
  EVAE_REQUIRE(aligned8(out) && ((uintptr_t)ws & 255) == 0, "silhouette_samples: misaligned out or workspace");
  EVAE_REQUIRE(ws_bytes >= evae_silhouette_workspace_bytes(N, d, strip_rows), "silhouette_samples: workspace of %zu bytes, %zu needed",
               ws_bytes, evae_silhouette_workspace_bytes(N, d, strip_rows));
  const int R = strip_rows_of(N, strip_rows);
  float* xs = static_cast<float*>(ws);
  float* strip = reinterpret_cast<float*>(static_cast<char*>(ws) + silhouette_rows_bytes(N, d));
  const size_t items = (size_t)N * d;
  silhouette_gather_kernel<<<(unsigned)((items + kKmThreads - 1) / kKmThreads), kKmThreads, 0, stream>>>(x, N, d, order, xs);
  int rc = check_launch("silhouette_gather_kernel");
  if (rc) return rc;
  constexpr int kRowsPerBlock = kKmThreads / 64;
  return for_each_strip(xs, N, d, R, strip, stream_, [&](int r0, int rows) {
    silhouette_reduce_kernel<<<(rows + kRowsPerBlock - 1) / kRowsPerBlock, kKmThreads, 0, stream>>>(strip, N, r0, rows, order, start,
                                                                                                     K, out);
    return check_launch("silhouette_reduce_kernel");
  });
}
