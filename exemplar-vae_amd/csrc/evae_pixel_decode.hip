// Cached ancestral sampler of the `pixelcnn` decoder: ONE persistent kernel evaluates the eval-mode network of models/PixelCNN.py --
// PixelSNAIL([28, 28], 64, 64, 3, 1, 4, 64) and the 1x1 mean head with its sigmoid -- for the pixels t0 <= t < t1 in raster order,
// one pixel of every layer at a time, over a per-image cache of the layers' inputs at the pixels before.  It replaces the 784 whole
// decoder passes of pixelcnn_generate (reference models/PixelCNN.py:91-120).
//
// What pixel t = (i, j) needs from earlier pixels, and what it leaves for later ones (names of utils/nn.py):
//   * the first causal convolutions read (x, image(z1), image(z2)) at (i-1, j-1..j+1) [horizontal, shifted down] and at (i-1, j-1),
//     (i, j-1) [vertical, shifted right]: straight from x and the latent images.  Row 0 of the horizontal and column 0 of the
//     vertical term are exact zeros (no bias): their inputs AND their bias are left out there.
//   * a causal 3x3 convolution at (i, j) reads its (ELU'd, zero-padded) input at the 7 live taps (i-2, j-1..j+1), (i-1, j-1..j+1),
//     (i, j-1) -- never at (i, j).  So conv1 AND conv2 of all four residual blocks at pixel t depend on cached values alone: the
//     cache holds, per block r, plane 2r = ELU(block input) and plane 2r+1 = ELU(conv1 output), 64 channels per pixel.  conv1's
//     output at t is computed only to fill plane 2r+1 at t; the residual chain at t is h_{r+1} = GLU(conv2_r(t)) + h_r.
//   * the attention of query t runs over the cached key / value projections of pixels < t (pixel 0: output 0, the start mask); the
//     columns j >= t, which the reference fills with -1e4, are left out as in csrc/evae_attn.hip (same condition for equality).
//
// Cache per image (floats): 8 planes [784][64], then K [8 heads][784][4], then V [8][784][4] = kPdCacheFloats.  Pixel t writes
// position t of every plane and of K / V; it reads positions < t only.  A fresh cache is zeros.  Every value that crosses pixels
// lives in the cache, in x or in nothing: [0, 784) in several launches over one cache is bit-identical to one launch.
//
// Plan: a workgroup of 256 threads owns G images (1, 2 or 4: one kernel instance each, chosen per launch) and walks the pixels; image b of a launch
// always belongs to block b / G, workgroups never wait for each other, no atomics.  Every layer at one pixel is a matrix-vector
// product y = W x, K <= 448, O <= 260, for the G images at once: the weights are packed TRANSPOSED ([K][O], O a multiple of 4) so
// that a thread loads one float4 of 4 outputs per k and feeds 4 x G accumulators; the k range is dealt to n = min(256 / (O/4), 16)
// chunks of threads (k = chunk, chunk + n, ...), whose partial sums go through LDS and are added in chunk order by the thread that
// applies the epilogue (bias, ELU, GLU + residual, sigmoid).  The order of every sum is fixed: runs are bit-identical.  Products
// that do not depend on each other share a phase (all barriers are in uniform control flow; per pixel: gather | first convs |
// blocks 0-1 | blocks 2-3 | key & query conv1 | their conv2 | q and k/v projections | attention | out_resblock conv1 + aux | conv2 |
// out | mean head: 20 barriers).  The weights (1.64 MB, 7 live taps of 9) stream from L2 once per pixel and workgroup, the cached
// keys and values (on average 100 KB per image) once per pixel and image: the kernel is bound by what one CU reads from L2.
//
// Images per workgroup, measured (whole pixelcnn_generate calls on 'cached', ms, median of 3, MI355X; the three instances of ONE build,
// tools/pixelsnail_generate_bench.py):
//        B =   10    100    256    257    384    512    550    768   1024   2048
//   G = 1     23.8   25.1   30.3   49.5   54.9   57.1   77.0   83.3  110.2  219.3
//   G = 2     27.3   30.3   34.1   34.0   35.7   36.6   62.4   69.1   71.1  142.1
//   G = 4     36.3   42.1   44.4   44.1   45.0   45.7   46.5   47.4   50.2   99.1
// More images amortise the weight stream but lengthen every phase of the chain; fewer use more CUs.  Up to 256 images (one per CU)
// G = 1 is fastest; beyond that its workgroups queue in rounds, and G = 2 (257 to 512 images: one round of at most 256 workgroups)
// and G = 4 (from 513) win by far more than three times the spread of the calls: evae_pixel_decode_choose_images below.
// EVAE_PD_IMAGES (1) is the G of evae_pixel_decode.  The cache of an image does not depend on G; the means do at rounding level (the
// attention deals 256 / (8 G) lanes to a head).  LDS at G = 1: 43936 bytes (7 taps x 8 planes = 14 KB, four partial-sum regions of
// 4 KB, 5 KB of vectors, 8 KB of biases), 79424 at G = 2, 150400 at G = 4; the registers (256 VGPRs + 94 / 182 / 228 AGPRs, no
// scratch) keep every instance at one workgroup per CU.
//
// Start pixels (image completion): with uniforms, image b is drawn from pixel start[b] on; before it x is read as given, as in a
// teacher-forced launch, and only the store of x at the end of the pixel loop is skipped.  One launch with start equals, per image
// and bit for bit, a teacher-forced launch over [0, start) followed by a sampling one over [start, 784) on the same cache.
#include "evae_common.h"

namespace evae {
namespace {

constexpr int kPdThreads = 256;
#ifndef EVAE_PD_IMAGES
#define EVAE_PD_IMAGES 1                   // (1, 2 or 4: the table above)
#endif
constexpr int kPdImages = EVAE_PD_IMAGES;    // the build's default images per workgroup (evae_pixel_decode_images_per_block): 1, 2 or 4
constexpr int kPdC = 64;                     // channels of the residual stream, of the blocks' inner width and of `out`
constexpr int kPdSide = 28;
constexpr int kPdL = kPdSide * kPdSide;
constexpr int kPdTaps = 7;
constexpr int kPdK = kPdTaps * kPdC;         // 448
constexpr int kPdRes = 4;
constexpr int kPdPlanes = 2 * kPdRes;
constexpr int kPdHeads = 8;
constexpr int kPdAttn = 32;                  // heads x 4
constexpr int kPdKeyC = 2 * kPdC + 2;        // 130
constexpr int kPdQryC = kPdC + 2;            // 66
constexpr size_t kPdPlaneFloats = (size_t)kPdL * kPdC;
constexpr size_t kPdKOff = kPdPlanes * kPdPlaneFloats;
constexpr size_t kPdVOff = kPdKOff + (size_t)kPdL * kPdAttn;
constexpr size_t kPdCacheFloats = kPdVOff + (size_t)kPdL * kPdAttn;
constexpr int kPdMaxChunks = 16;
constexpr __host__ __device__ int pd_part(int G) { return 1024 * G; }      // floats of one partial-sum region: chunks x images x O <= 1024 x images for every product
constexpr int kPdRegions = 4;
constexpr __host__ __device__ bool pd_images_ok(int G) { return G == 1 || G == 2 || G == 4; }      // the attention deals 256 / (8 images) lanes to a head
static_assert(pd_images_ok(kPdImages), "EVAE_PD_IMAGES must be 1, 2 or 4");

// the packed buffer: slot s starts at float offset off[s] (a multiple of 4)
enum PdSlot {
  PD_IN_W, PD_HOR_B, PD_VER_B,                                   // [15][64]: rows 0-8 horizontal (dj, c), rows 9-14 vertical (di, c)
  PD_RES0,                                                       // + 4 r: conv1 W [448][64], b [64], conv2 W [448][128], b [128]
  PD_K1_W = PD_RES0 + 4 * kPdRes, PD_K1_B, PD_K2_W, PD_K2_B,    // key_resblock: [130][64], [64][260]
  PD_Q1_W, PD_Q1_B, PD_Q2_W, PD_Q2_B,                            // query_resblock: [66][64], [64][132]
  PD_AQ_W, PD_AQ_B, PD_AKV_W, PD_AKV_B,                          // attention: query [66][32]; key | value [130][64]
  PD_O1_W, PD_O1_B, PD_OA_B, PD_O2_W, PD_O2_B,                   // out_resblock: conv1 | aux_conv [96][64], both biases, conv2 [64][128]
  PD_F_W, PD_F_B,                                                // out.1 [64][64]
  PD_M_W, PD_M_B,                                                // p_x_mean [64][4] (column 0), [4]
  PD_BG,                                                         // background [2][784]
  PD_SLOTS
};
constexpr int kPdHeader = 9;                 // magic, channel, res_channel, height, width, n_res_block, heads, head width, total floats
constexpr int kPdMagic = 0x50584443;

inline int pd_slot_floats(int s) {
  if (s >= PD_RES0 && s < PD_K1_W) {
    const int q = (s - PD_RES0) & 3;
    return q == 0 ? kPdK * kPdC : q == 1 ? kPdC : q == 2 ? kPdK * 2 * kPdC : 2 * kPdC;
  }
  switch (s) {
    case PD_IN_W: return 15 * kPdC;
    case PD_K1_W: return kPdKeyC * kPdC;
    case PD_K2_W: return kPdC * 2 * kPdKeyC;
    case PD_K2_B: return 2 * kPdKeyC;
    case PD_Q1_W: return kPdQryC * kPdC;
    case PD_Q2_W: return kPdC * 2 * kPdQryC;
    case PD_Q2_B: return 2 * kPdQryC;
    case PD_AQ_W: return kPdQryC * kPdAttn;
    case PD_AQ_B: return kPdAttn;
    case PD_AKV_W: return kPdKeyC * 2 * kPdAttn;
    case PD_O1_W: return (kPdC + kPdAttn) * kPdC;
    case PD_O2_W: return kPdC * 2 * kPdC;
    case PD_O2_B: return 2 * kPdC;
    case PD_F_W: return kPdC * kPdC;
    case PD_M_W: return kPdC * 4;
    case PD_M_B: return 4;
    case PD_BG: return 2 * kPdL;
    default: return kPdC;                   // the 64-wide biases
  }
}

// the bias slots: the layout keeps them in one block of at most kPdBiasMax floats, which every workgroup copies to LDS once
constexpr int kPdBiasMax = 2048;
constexpr __host__ __device__ bool pd_is_bias(int s) {
  return s == PD_HOR_B || s == PD_VER_B || (s >= PD_RES0 && s < PD_K1_W && ((s - PD_RES0) & 1)) || s == PD_K1_B || s == PD_K2_B ||
         s == PD_Q1_B || s == PD_Q2_B || s == PD_AQ_B || s == PD_AKV_B || s == PD_O1_B || s == PD_OA_B || s == PD_O2_B || s == PD_F_B ||
         s == PD_M_B;
}

struct PdParams {
  const float* w;
  const float* latent;     // [B][2][784]
  float* x;                // [B][784]
  const float* u;          // [B][784] or null (teacher-forced: x is read only)
  const int* start;        // [B] or null: with u, image b keeps x[b][t] for t < start[b] and is sampled from there (null: 0 for all)
  float* mean;             // [B][784]
  float* cache;            // [B][kPdCacheFloats]
  int B, t0, t1;
  int bias0, bias_n;       // the block of bias slots: floats [bias0, bias0 + bias_n) of w
  int off[PD_SLOTS];
};

// the vectors of one image in LDS (float offsets)
enum PdVec {
  V_IN0 = 0,                // 15 inputs of the first convolutions
  V_HIN = 16,               // block input (horizontal + vertical)
  V_H = V_HIN + 64,         // residual stream
  V_KIN = V_H + 64,         // (block input, block output, background) [130]
  V_KINE = V_KIN + 132,     // its ELU
  V_QIN = V_KINE + 132,     // (block output, background) [66]
  V_QINE = V_QIN + 68,
  V_M1K = V_QINE + 68,      // ELU(conv1) of key_resblock / query_resblock / out_resblock
  V_M1Q = V_M1K + 64,
  V_KEY = V_M1Q + 64,       // key_resblock output [130]
  V_QRY = V_KEY + 132,      // query_resblock output [66]
  V_Q = V_QRY + 68,         // projected query [32]
  V_EO = V_Q + 32,          // (ELU(block output), ELU(attention output)) [96]
  V_M1O = V_EO + 96,
  V_H5E = V_M1O + 64,       // ELU(out_resblock output)
  V_Y = V_H5E + 64,         // out.1
  V_END = V_Y + 64
};
constexpr __host__ __device__ int pd_lds_floats(int G) {      // (+ slot offsets, biases)
  return G * (kPdPlanes * kPdK + V_END) + kPdRegions * pd_part(G) + 64 + kPdBiasMax;
}
static_assert(pd_lds_floats(4) * sizeof(float) <= 160 * 1024, "the largest instance must fit the LDS of a CU");

__device__ __forceinline__ float pd_elu(float v) { return v > 0.f ? v : expm1f(v); }
__device__ __forceinline__ float pd_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }
constexpr __host__ __device__ int pd_chunks(int O) { return kPdThreads / (O / 4) > kPdMaxChunks ? kPdMaxChunks : kPdThreads / (O / 4); }
constexpr int kPdLoadBatch = 28;             // weight loads (float4) a thread issues before it uses the first one

// partial sums of y[g][o] = sum_k Wt[k][o] in[g * stride + k] into part[(chunk * G + g) * O + o].  K and O are compile-time: a
// thread's (at most 56) steps are unrolled in batches of kPdLoadBatch loads, all issued before the first multiply-add -- the
// products are bound by the latency of these L2 reads, not by their bandwidth.
template <int G, int K, int O>
__device__ __forceinline__ void pd_matvec(const float* __restrict__ Wt, const float* in, int stride, float* part) {
  constexpr int O4 = O / 4, NCH = pd_chunks(O), TRIPS = (K + NCH - 1) / NCH;
  constexpr int BATCHES = (TRIPS + kPdLoadBatch - 1) / kPdLoadBatch, UB = (TRIPS + BATCHES - 1) / BATCHES;
  const int c = threadIdx.x / O4, o4 = threadIdx.x - c * O4;
  if (c >= NCH) return;
  float4 acc[G];
#pragma unroll
  for (int g = 0; g < G; ++g) acc[g] = make_float4(0.f, 0.f, 0.f, 0.f);
  const float4* w4 = reinterpret_cast<const float4*>(Wt) + o4;
#pragma unroll
  for (int k0 = 0; k0 < TRIPS; k0 += UB) {
    float4 w[UB];
#pragma unroll
    for (int q = 0; q < UB; ++q) {
      const int k = c + (k0 + q) * NCH;
      if (k0 + q < TRIPS && k < K) w[q] = w4[(size_t)k * O4];
    }
#pragma unroll
    for (int q = 0; q < UB; ++q) {
      const int k = c + (k0 + q) * NCH;
      if (k0 + q < TRIPS && k < K) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const float a = in[g * stride + k];
          acc[g].x = fmaf(a, w[q].x, acc[g].x);
          acc[g].y = fmaf(a, w[q].y, acc[g].y);
          acc[g].z = fmaf(a, w[q].z, acc[g].z);
          acc[g].w = fmaf(a, w[q].w, acc[g].w);
        }
      }
    }
  }
#pragma unroll
  for (int g = 0; g < G; ++g) reinterpret_cast<float4*>(part)[(c * G + g) * O4 + o4] = acc[g];
}

// y[g][o] without its bias: the chunks' partial sums in chunk order
template <int G, int O>
__device__ __forceinline__ float pd_sum(const float* part, int g, int o) {
  constexpr int NCH = pd_chunks(O);
  float s = part[g * O + o];
#pragma unroll
  for (int c = 1; c < NCH; ++c) s += part[(c * G + g) * O + o];
  return s;
}

template <int G>
__global__ __launch_bounds__(kPdThreads) void pixel_decode_kernel(PdParams p) {
  extern __shared__ float4 pd_smem[];
  float* taps = reinterpret_cast<float*>(pd_smem);       // [G][8 planes][7 taps][64]
  constexpr int kPdPart = pd_part(G);
  float* part = taps + G * kPdPlanes * kPdK;             // [4 regions][kPdPart]
  float* vec = part + kPdRegions * kPdPart;              // [G][V_END]
  int* off = reinterpret_cast<int*>(vec + G * V_END);    // the slot offsets (in LDS: 41 values that would otherwise sit in SGPRs)
  const int tid = threadIdx.x;
  const int b0 = blockIdx.x * G;
  const float* W = p.w;
  float* SB = reinterpret_cast<float*>(off + 64);        // the biases; off[] of a bias slot is relative to this block
  if (tid < PD_SLOTS) off[tid] = pd_is_bias(tid) ? p.off[tid] - p.bias0 : p.off[tid];
  for (int e = tid; e < p.bias_n; e += kPdThreads) SB[e] = W[p.bias0 + e];
  __syncthreads();
  const float* bg = W + off[PD_BG];
  // the first pixel the owner thread of image b0 + tid draws (earlier ones are read as given); read once, before the pixel loop
  int first = 0;
  if (tid < G && b0 + tid < p.B && p.start != nullptr) first = p.start[b0 + tid];

  for (int t = p.t0; t < p.t1; ++t) {
    const int i = t / kPdSide, j = t - i * kPdSide;

    // ---- gather: the 7 taps of the 8 cached planes, and the inputs of the first convolutions -------------------------------
    for (int e = tid; e < G * kPdPlanes * kPdTaps * (kPdC / 4); e += kPdThreads) {
      const int c4 = e & 15;
      int r = e >> 4;
      const int tap = r % kPdTaps;
      r /= kPdTaps;
      const int pl = r & (kPdPlanes - 1), g = r >> 3;
      const int di = tap / 3, dj = tap - di * 3;
      const int row = i - 2 + di, col = j - 1 + dj;
      const int b = b0 + g;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (b < p.B && row >= 0 && col >= 0 && col < kPdSide)
        v = reinterpret_cast<const float4*>(p.cache + (size_t)b * kPdCacheFloats + (size_t)pl * kPdPlaneFloats +
                                            (size_t)(row * kPdSide + col) * kPdC)[c4];
      reinterpret_cast<float4*>(taps + (g * kPdPlanes + pl) * kPdK + tap * kPdC)[c4] = v;
    }
    if (tid < G * 16) {
      const int g = tid >> 4, k = tid & 15, b = b0 + g;
      float v = 0.f;
      if (b < p.B && k < 15) {
        int row, col, c;
        if (k < 9) { row = i - 1; col = j - 1 + k / 3; c = k % 3; }          // horizontal: (i-1, j-1+dj)
        else if (k < 12) { row = i - 1; col = j - 1; c = k - 9; }            // vertical, filter row 0: (i-1, j-1)
        else { row = i; col = j - 1; c = k - 12; }                           // vertical, filter row 1: (i, j-1)
        const bool live = k < 9 ? i >= 1 : j >= 1;                           // the shifted-in row / column is zero
        if (live && row >= 0 && col >= 0 && col < kPdSide) {
          const size_t pix = (size_t)row * kPdSide + col;
          v = c == 0 ? p.x[(size_t)b * kPdL + pix] : p.latent[((size_t)b * 2 + (c - 1)) * kPdL + pix];
        }
      }
      vec[g * V_END + V_IN0 + k] = v;
    }
    __syncthreads();

    // ---- first convolutions (K = 15: horizontal and vertical in one product, their biases added where their term exists) --------
    pd_matvec<G, 15, kPdC>(W + off[PD_IN_W], vec + V_IN0, V_END, part);
    __syncthreads();
    for (int e = tid; e < G * kPdC; e += kPdThreads) {
      const int g = e >> 6, c = e & 63, b = b0 + g;
      float v = pd_sum<G, kPdC>(part, g, c);
      if (i >= 1) v += SB[off[PD_HOR_B] + c];
      if (j >= 1) v += SB[off[PD_VER_B] + c];
      vec[g * V_END + V_HIN + c] = v;
      vec[g * V_END + V_H + c] = v;
      if (b < p.B) p.cache[(size_t)b * kPdCacheFloats + (size_t)t * kPdC + c] = pd_elu(v);        // plane 0
    }
    __syncthreads();

    // ---- the four causal residual blocks, two per phase: their 7-tap products read cached planes only; the chain over r is
    //      element-wise (h += GLU(conv2_r)), one thread per (image, channel) ----------------------------------------------------------
    for (int half = 0; half < 2; ++half) {
      for (int q = 0; q < 2; ++q) {
        const int r = half * 2 + q;
        pd_matvec<G, kPdK, kPdC>(W + off[PD_RES0 + 4 * r], taps + (2 * r) * kPdK, kPdPlanes * kPdK, part + (2 * q) * kPdPart);
        pd_matvec<G, kPdK, 2 * kPdC>(W + off[PD_RES0 + 4 * r + 2], taps + (2 * r + 1) * kPdK, kPdPlanes * kPdK, part + (2 * q + 1) * kPdPart);
      }
      __syncthreads();
      for (int e = tid; e < G * kPdC; e += kPdThreads) {
        const int g = e >> 6, c = e & 63, b = b0 + g;
        float* cache = p.cache + (size_t)(b < p.B ? b : 0) * kPdCacheFloats + (size_t)t * kPdC + c;
        float h = vec[g * V_END + V_H + c];
        for (int q = 0; q < 2; ++q) {
          const int r = half * 2 + q;
          const float m1 = pd_sum<G, kPdC>(part + (2 * q) * kPdPart, g, c) + SB[off[PD_RES0 + 4 * r + 1] + c];
          const float* p2 = part + (2 * q + 1) * kPdPart;
          const float a = pd_sum<G, 2 * kPdC>(p2, g, c) + SB[off[PD_RES0 + 4 * r + 3] + c];
          const float gt = pd_sum<G, 2 * kPdC>(p2, g, kPdC + c) + SB[off[PD_RES0 + 4 * r + 3] + kPdC + c];
          h = fmaf(a, pd_sigmoid(gt), h);
          if (b < p.B) {
            cache[(size_t)(2 * r + 1) * kPdPlaneFloats] = pd_elu(m1);
            if (r + 1 < kPdRes) cache[(size_t)(2 * r + 2) * kPdPlaneFloats] = pd_elu(h);
          }
        }
        vec[g * V_END + V_H + c] = h;
        if (half == 1) {
          // the inputs of key_resblock (block input, block output, background), query_resblock and out_resblock's conv1
          float* v = vec + g * V_END;
          const float hin = v[V_HIN + c], eh = pd_elu(h);
          v[V_KIN + c] = hin;
          v[V_KINE + c] = pd_elu(hin);
          v[V_KIN + kPdC + c] = h;
          v[V_KINE + kPdC + c] = eh;
          v[V_QIN + c] = h;
          v[V_QINE + c] = eh;
          v[V_EO + c] = eh;
          if (c < 2) {
            const float co = bg[c * kPdL + t], ec = pd_elu(co);
            v[V_KIN + 2 * kPdC + c] = co;
            v[V_KINE + 2 * kPdC + c] = ec;
            v[V_QIN + kPdC + c] = co;
            v[V_QINE + kPdC + c] = ec;
          }
        }
      }
      __syncthreads();
    }

    // ---- key_resblock and query_resblock (1x1) ----------------------------------------------------------------------------------
    pd_matvec<G, kPdKeyC, kPdC>(W + off[PD_K1_W], vec + V_KINE, V_END, part);
    pd_matvec<G, kPdQryC, kPdC>(W + off[PD_Q1_W], vec + V_QINE, V_END, part + kPdPart);
    __syncthreads();
    for (int e = tid; e < G * kPdC; e += kPdThreads) {
      const int g = e >> 6, c = e & 63;
      vec[g * V_END + V_M1K + c] = pd_elu(pd_sum<G, kPdC>(part, g, c) + SB[off[PD_K1_B] + c]);
      vec[g * V_END + V_M1Q + c] = pd_elu(pd_sum<G, kPdC>(part + kPdPart, g, c) + SB[off[PD_Q1_B] + c]);
    }
    __syncthreads();
    pd_matvec<G, kPdC, 2 * kPdKeyC>(W + off[PD_K2_W], vec + V_M1K, V_END, part);
    pd_matvec<G, kPdC, 2 * kPdQryC>(W + off[PD_Q2_W], vec + V_M1Q, V_END, part + kPdPart);
    __syncthreads();
    for (int e = tid; e < G * (kPdKeyC + kPdQryC); e += kPdThreads) {
      const int g = e / (kPdKeyC + kPdQryC);
      int c = e - g * (kPdKeyC + kPdQryC);
      float* v = vec + g * V_END;
      if (c < kPdKeyC) {
        const float a = pd_sum<G, 2 * kPdKeyC>(part, g, c) + SB[off[PD_K2_B] + c];
        const float gt = pd_sum<G, 2 * kPdKeyC>(part, g, kPdKeyC + c) + SB[off[PD_K2_B] + kPdKeyC + c];
        v[V_KEY + c] = fmaf(a, pd_sigmoid(gt), v[V_KIN + c]);
      } else {
        c -= kPdKeyC;
        const float a = pd_sum<G, 2 * kPdQryC>(part + kPdPart, g, c) + SB[off[PD_Q2_B] + c];
        const float gt = pd_sum<G, 2 * kPdQryC>(part + kPdPart, g, kPdQryC + c) + SB[off[PD_Q2_B] + kPdQryC + c];
        v[V_QRY + c] = fmaf(a, pd_sigmoid(gt), v[V_QIN + c]);
      }
    }
    __syncthreads();

    // ---- the projections: q of this pixel; k and v of this pixel go to the cache (later pixels attend to them) ----------------
    pd_matvec<G, kPdQryC, kPdAttn>(W + off[PD_AQ_W], vec + V_QRY, V_END, part);
    pd_matvec<G, kPdKeyC, 2 * kPdAttn>(W + off[PD_AKV_W], vec + V_KEY, V_END, part + kPdPart);
    __syncthreads();
    for (int e = tid; e < G * 3 * kPdAttn; e += kPdThreads) {
      const int g = e / (3 * kPdAttn), b = b0 + g;
      int c = e - g * (3 * kPdAttn);
      if (c < kPdAttn) {
        vec[g * V_END + V_Q + c] = pd_sum<G, kPdAttn>(part, g, c) + SB[off[PD_AQ_B] + c];
      } else {
        c -= kPdAttn;                                                         // 0..31 key, 32..63 value
        const float v = pd_sum<G, 2 * kPdAttn>(part + kPdPart, g, c) + SB[off[PD_AKV_B] + c];
        const int d = c & (kPdAttn - 1), head = d >> 2;
        if (b < p.B)
          p.cache[(size_t)b * kPdCacheFloats + (c < kPdAttn ? kPdKOff : kPdVOff) + ((size_t)head * kPdL + t) * 4 + (d & 3)] = v;
      }
    }
    __syncthreads();

    // ---- attention of query t over the keys of pixels < t: 256 / (8 G) lanes per (image, head), key n + lanes * m to lane n;
    //      each lane keeps a running maximum (raised once per batch of 16 keys), the lanes are merged in a fixed butterfly ----------
    {
      constexpr int LANES = kPdThreads / (kPdHeads * G);
      const int pair = tid / LANES, lane = tid - pair * LANES;
      const int g = pair / kPdHeads, head = pair - g * kPdHeads, b = b0 + g;
      const float* qv = vec + g * V_END + V_Q + head * 4;
      const float4 q = make_float4(qv[0] * 0.5f, qv[1] * 0.5f, qv[2] * 0.5f, qv[3] * 0.5f);      // 1 / sqrt(4): exact
      const size_t base = (size_t)(b < p.B ? b : 0) * kPdCacheFloats + (size_t)head * kPdL * 4;
      const float4* k4 = reinterpret_cast<const float4*>(p.cache + base + kPdKOff);
      const float4* v4 = reinterpret_cast<const float4*>(p.cache + base + kPdVOff);
      float m = -INFINITY, sum = 0.f;
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      const int n_keys = b < p.B ? t : 0;
      constexpr int UB = 16;                                                   // keys a lane loads before it uses the first
      for (int n0 = lane; n0 < n_keys; n0 += LANES * UB) {
        float4 kk[UB], vv[UB];
#pragma unroll
        for (int q_ = 0; q_ < UB; ++q_) {
          const int n = n0 + q_ * LANES;
          if (n < n_keys) { kk[q_] = k4[n]; vv[q_] = v4[n]; }
        }
        // one rescale per batch: the batch's maximum first, then UB independent exponentials
        float sc[UB], bm = m;
#pragma unroll
        for (int q_ = 0; q_ < UB; ++q_) {
          sc[q_] = -INFINITY;
          if (n0 + q_ * LANES < n_keys) sc[q_] = fmaf(q.w, kk[q_].w, fmaf(q.z, kk[q_].z, fmaf(q.y, kk[q_].y, q.x * kk[q_].x)));
          bm = fmaxf(bm, sc[q_]);
        }
        if (bm > m) {
          const float f = expf(m - bm);                                       // (m = -inf: 0)
          sum *= f; acc.x *= f; acc.y *= f; acc.z *= f; acc.w *= f;
          m = bm;
        }
#pragma unroll
        for (int q_ = 0; q_ < UB; ++q_) {
          if (n0 + q_ * LANES < n_keys) {
            const float pe = expf(sc[q_] - m);
            sum += pe;
            acc.x = fmaf(pe, vv[q_].x, acc.x); acc.y = fmaf(pe, vv[q_].y, acc.y);
            acc.z = fmaf(pe, vv[q_].z, acc.z); acc.w = fmaf(pe, vv[q_].w, acc.w);
          }
        }
      }
#pragma unroll
      for (int d = 1; d < LANES; d <<= 1) {
        const float m2 = __shfl_xor(m, d), s2 = __shfl_xor(sum, d);
        const float ax = __shfl_xor(acc.x, d), ay = __shfl_xor(acc.y, d), az = __shfl_xor(acc.z, d), aw = __shfl_xor(acc.w, d);
        const float mm = fmaxf(m, m2);
        // both sides of a pair compute the same two products and add them in the same (lower lane first) order
        const bool low = (lane & d) == 0;
        const float f_own = m == -INFINITY ? 0.f : expf(m - mm), f_oth = m2 == -INFINITY ? 0.f : expf(m2 - mm);
        const float fa = low ? f_own : f_oth, fb = low ? f_oth : f_own;
        sum = (low ? sum : s2) * fa + (low ? s2 : sum) * fb;
        acc.x = (low ? acc.x : ax) * fa + (low ? ax : acc.x) * fb;
        acc.y = (low ? acc.y : ay) * fa + (low ? ay : acc.y) * fb;
        acc.z = (low ? acc.z : az) * fa + (low ? az : acc.z) * fb;
        acc.w = (low ? acc.w : aw) * fa + (low ? aw : acc.w) * fb;
        m = mm;
      }
      if (lane == 0) {
        const float inv = sum > 0.f ? 1.0f / sum : 0.f;                        // pixel 0: no key, output 0
        float* eo = vec + g * V_END + V_EO + kPdC + head * 4;
        eo[0] = pd_elu(acc.x * inv); eo[1] = pd_elu(acc.y * inv); eo[2] = pd_elu(acc.z * inv); eo[3] = pd_elu(acc.w * inv);
      }
    }
    __syncthreads();

    // ---- out_resblock (conv1 + aux_conv as one product over 96 inputs), the final ELU, out.1, the mean head ----------------------
    pd_matvec<G, kPdC + kPdAttn, kPdC>(W + off[PD_O1_W], vec + V_EO, V_END, part);
    __syncthreads();
    for (int e = tid; e < G * kPdC; e += kPdThreads) {
      const int g = e >> 6, c = e & 63;
      vec[g * V_END + V_M1O + c] = pd_elu(pd_sum<G, kPdC>(part, g, c) + SB[off[PD_O1_B] + c] + SB[off[PD_OA_B] + c]);
    }
    __syncthreads();
    pd_matvec<G, kPdC, 2 * kPdC>(W + off[PD_O2_W], vec + V_M1O, V_END, part);
    __syncthreads();
    for (int e = tid; e < G * kPdC; e += kPdThreads) {
      const int g = e >> 6, c = e & 63;
      const float a = pd_sum<G, 2 * kPdC>(part, g, c) + SB[off[PD_O2_B] + c];
      const float gt = pd_sum<G, 2 * kPdC>(part, g, kPdC + c) + SB[off[PD_O2_B] + kPdC + c];
      vec[g * V_END + V_H5E + c] = pd_elu(fmaf(a, pd_sigmoid(gt), vec[g * V_END + V_H + c]));
    }
    __syncthreads();
    pd_matvec<G, kPdC, kPdC>(W + off[PD_F_W], vec + V_H5E, V_END, part);
    __syncthreads();
    for (int e = tid; e < G * kPdC; e += kPdThreads) {
      const int g = e >> 6, c = e & 63;
      vec[g * V_END + V_Y + c] = pd_sum<G, kPdC>(part, g, c) + SB[off[PD_F_B] + c];
    }
    __syncthreads();
    pd_matvec<G, kPdC, 4>(W + off[PD_M_W], vec + V_Y, V_END, part);
    __syncthreads();
    if (tid < G) {
      const int b = b0 + tid;
      if (b < p.B) {
        const float mu = pd_sigmoid(pd_sum<G, 4>(part, tid, 0) + SB[off[PD_M_B]]);
        const size_t e = (size_t)b * kPdL + t;
        p.mean[e] = mu;
        if (p.u != nullptr && t >= first) p.x[e] = p.u[e] < mu ? 1.0f : 0.0f;  // before pixel t + 1 reads it (barrier below)
      }
    }
    __syncthreads();
  }
}

}  // namespace
}  // namespace evae

using namespace evae;

namespace {
template <int G>
void pd_launch(const PdParams& p, hipStream_t s) {
  constexpr size_t lds = (size_t)pd_lds_floats(G) * sizeof(float);
  static bool attr = false;                  // once per instance
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)pixel_decode_kernel<G>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    attr = true;
  }
  pixel_decode_kernel<G><<<(p.B + G - 1) / G, kPdThreads, lds, s>>>(p);
}
}  // namespace

extern "C" int evae_pixel_decode_images_per_block(void) { return kPdImages; }
extern "C" int evae_pixel_decode_table_len(void) { return kPdHeader + PD_SLOTS; }
extern "C" size_t evae_pixel_decode_cache_floats(void) { return kPdCacheFloats; }
extern "C" size_t evae_pixel_decode_lds_bytes(void) { return (size_t)pd_lds_floats(kPdImages) * sizeof(float); }
extern "C" size_t evae_pixel_decode_lds_bytes_for(int g) { return pd_images_ok(g) ? (size_t)pd_lds_floats(g) * sizeof(float) : 0; }
extern "C" int evae_pixel_decode_slot_floats(int slot) { return slot >= 0 && slot < PD_SLOTS ? pd_slot_floats(slot) : -1; }

// The images per workgroup the library picks for a launch of B images (host arithmetic).  A range of B leaves 1 only where the larger
// G beat 1 at the measured sizes on both of its sides by more than 3 x the larger spread (the table in the header: 257 and 512 for
// 2; 512, 550 and every larger size for 4, where 2 needs a second round of workgroups from 513 on).
extern "C" int evae_pixel_decode_choose_images(int B) { return B <= 256 ? 1 : B <= 512 ? 2 : 4; }

extern "C" int evae_pixel_decode_ex(const float* packed, const int* table, int table_len, const float* latent, float* x, const float* u,
                                    const int* start, float* mean, float* cache, int B, int t0, int t1, int images_per_block,
                                    evae_stream_t s) {
  EVAE_REQUIRE(pd_images_ok(images_per_block), "pixel_decode: %d images per workgroup are not built (1, 2 or 4 only)", images_per_block);
  EVAE_REQUIRE(table && table_len == kPdHeader + PD_SLOTS, "pixel_decode: the offset table must hold %d entries", kPdHeader + PD_SLOTS);
  EVAE_REQUIRE(table[0] == kPdMagic, "pixel_decode: not a packed-weight table");
  EVAE_REQUIRE(table[1] == kPdC && table[2] == kPdC, "pixel_decode: channel counts %d / %d are not supported (%d only)", table[1],
               table[2], kPdC);
  EVAE_REQUIRE(table[3] == kPdSide && table[4] == kPdSide, "pixel_decode: %d x %d images are not supported (%d x %d only)", table[3],
               table[4], kPdSide, kPdSide);
  EVAE_REQUIRE(table[5] == kPdRes && table[6] == kPdHeads && table[7] == 4,
               "pixel_decode: %d residual blocks, %d heads of width %d are not supported (%d, %d, 4 only)", table[5], table[6], table[7],
               kPdRes, kPdHeads);
  PdParams p;
  for (int sl = 0; sl < PD_SLOTS; ++sl) {
    const int o = table[kPdHeader + sl];
    EVAE_REQUIRE(o >= 0 && (o & 3) == 0 && (int64_t)o + pd_slot_floats(sl) <= (int64_t)table[8],
                 "pixel_decode: slot %d at offset %d does not fit the packed buffer of %d floats", sl, o, table[8]);
    p.off[sl] = o;
  }
  int lo = 0x7fffffff, hi = 0;
  for (int sl = 0; sl < PD_SLOTS; ++sl)
    if (pd_is_bias(sl)) {
      lo = p.off[sl] < lo ? p.off[sl] : lo;
      hi = p.off[sl] + pd_slot_floats(sl) > hi ? p.off[sl] + pd_slot_floats(sl) : hi;
    }
  EVAE_REQUIRE(hi - lo <= kPdBiasMax, "pixel_decode: the bias slots span %d floats, not one block of at most %d", hi - lo, kPdBiasMax);
  p.bias0 = lo;
  p.bias_n = hi - lo;
  EVAE_REQUIRE(B >= 0, "pixel_decode: bad sizes");
  EVAE_REQUIRE(t0 >= 0 && t0 <= t1, "pixel_decode: the pixel range [%d, %d) is not a range", t0, t1);
  EVAE_REQUIRE(t1 <= kPdL, "pixel_decode: the pixel range ends at %d, past the %d pixels of an image", t1, kPdL);
  if (B == 0 || t0 == t1) return EVAE_OK;
  EVAE_REQUIRE(packed && latent && x && mean && cache && (((uintptr_t)packed | (uintptr_t)cache) & 15) == 0,
               "pixel_decode: null or unaligned pointer");
  p.w = packed; p.latent = latent; p.x = x; p.u = u; p.start = u != nullptr ? start : nullptr; p.mean = mean; p.cache = cache;
  p.B = B; p.t0 = t0; p.t1 = t1;
  switch (images_per_block) {
    case 1: pd_launch<1>(p, (hipStream_t)s); break;
    case 2: pd_launch<2>(p, (hipStream_t)s); break;
    default: pd_launch<4>(p, (hipStream_t)s); break;
  }
  return check_launch("pixel_decode");
}

extern "C" int evae_pixel_decode(const float* packed, const int* table, int table_len, const float* latent, float* x, const float* u,
                                 float* mean, float* cache, int B, int t0, int t1, evae_stream_t s) {
  return evae_pixel_decode_ex(packed, table, table_len, latent, x, u, nullptr, mean, cache, B, t0, t1, kPdImages, s);
}
