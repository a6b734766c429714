// PixelSNAIL decoder kernels: fused causal attention (forward + backward), ELU -> dropout, and the GLU residual.
// Replaces reference utils/nn.py:339-365 (CausalAttention.forward behind its three projections), the activation -> dropout of
// GatedResBlock.forward (utils/nn.py:293,298-299) and its `gate(out) + input` tail (utils/nn.py:307-308).
//
// Causal attention, per (image b, head h), dh = 4, L positions, inputs as rows [B*L, H*dh] (head h = columns [4h, 4h+4)):
//     s_ij = (q_i . k_j) / sqrt(dh);  s_ij := -1e4 where j >= i;  p_i = softmax_j(s_i) over all L columns;  p_0 := 0 (start mask);
//     p := dropout(p);  out_i = sum_j p_ij v_j.
// The kernels LEAVE THE COLUMNS j >= i OUT instead of adding their exp(-1e4 - max_j s_ij).  In float32 the two agree exactly while
//     max_{j<i} s_ij > -1e4 + 104        (exp(-104) < 2^-149: every filled column then rounds to a zero term of the sum);
// below that the reference's filled columns would carry weight and this kernel is not its equal.  Row 0 has no column j < 0: its
// output and its gradient contribution are exactly zero, which is what the reference's uniform row times the start mask gives.
//
// No [L x L] tensor reaches memory.  Forward keeps one log-sum-exp per row ([B, H, L]); backward recomputes p_ij = exp(s_ij - lse_i):
//     dp_ij = m_ij / (1 - p_drop) (dO_i . v_j);  delta_i = sum_{j<i} p_ij dp_ij / sum_{j<i} p_ij  (= dO_i . out_i in exact arithmetic);
//     ds_ij = p_ij (dp_ij - delta_i);
//     dq_i = sum_{j<i} ds_ij k_j / sqrt(dh)   (row pass);   dk_j = sum_{i>j} ds_ij q_i / sqrt(dh),  dv_j = sum_{i>j} p_ij m_ij/(1-p_drop) dO_i
//     (column pass).  Every sum is one thread's loop in a fixed order: no atomics, bit-identical from run to run.
// delta comes from the recomputed p, summed in the row pass and handed to the column pass through a [B, H, L] scratch array; it is not
// taken as dO_i . out_i, for two reasons.  (1) A row with ONE column (i = 1) has p = 1 and ds = dp - dp, an exact zero as in the
// reference's softmax backward; dO . round(out) leaves a rounding residue there.  (2) The recomputed p of a row carry one common factor
// (1 + e), e the rounding of that row's log-sum-exp; dividing by their sum makes sum_j ds_ij vanish again, which is what keeps the
// gradient of anything the softmax ignores (the key projection's bias) at rounding level.  The row pass is still ONE loop: with the
// shift d~_i = dO_i . out_i,  dq_i = [sum_j p (dp - d~) k_j - (delta_i - d~_i) sum_j p k_j] / sqrt(dh); the second term is a
// rounding-sized correction, so nothing of size cancels.  The backward kernels are compiled without floating-point contraction:
// dp has to be the same rounded number wherever it is used (explicit fmaf calls stay fused).
//
// Plan: one workgroup of 256 threads per (b, h).  Row pass (forward, dq): K and V of the head in LDS (32 L bytes), one thread per
// row, all lanes of a wave walk j = 0, 1, ... together (LDS broadcast reads).  Column pass (dk, dv): Q, dO (16 L bytes each), lse and
// delta (4 L each) in LDS = 40 L bytes, one thread per column, lanes walk i = L-1, L-2, ... together.  Rows (columns) are taken in
// pairs i and L-1-i so that every thread does L-1 steps whatever its row.  LDS stays within the 64 KiB a workgroup gets without
// asking for more: 40 L <= 65536 -> L <= kAttnMaxLen = 1536 (the model's L is 784 = 31 KB).  dh = 4 is too narrow for MFMA.
//
// Dropout masks (attention and ELU -> dropout): Philox4x32-10, never stored.  Element e of the flattened tensor ([B, H, L, L] for the
// attention probabilities, e = ((b H + h) L + i) L + j in 64-bit arithmetic; the flat storage index for the element-wise op) takes
// word e % 4 of quad e / 4; counter (quad_lo, quad_hi, offset_lo, offset_hi), key (seed_lo, seed_hi); keep <=> u01(word) >= p_drop,
// kept values scaled by 1 / (1 - p_drop).  p_drop = 0 draws nothing and runs the code without a mask.
// Where (seed, offset) come from is the ONLY difference between the host-argument launches and the *_dev ones: a DropRng is a launch
// argument; a DropDev names the two device words [seed, step counter] of a captured step's control block (evae/graph.py) plus the
// ordinal of the mask within the step, and drop_source() turns either into the DropRng the mask code runs on -- one uniform load of
// the two words at kernel entry, offset = evae_dropout_step_offset(counter, ordinal).  A replayed graph node carries the pointer and
// the ordinal; the counter it reads is the replay's.
#include "evae_common.h"
#include "evae_philox.h"

namespace evae {
namespace {

constexpr int kAttnThreads = 256;
constexpr int kAttnDh = 4;
constexpr int kAttnMaxLen = 1536;

struct DropRng {
  uint2 key;
  uint32_t off_lo, off_hi;
  float p, scale;
};

// where a *_dev launch takes its Philox words from
struct DropDev {
  const int64_t* seed_ctr;    // device: [seed, step counter]
  uint32_t ordinal;
  float p, scale;
};

constexpr uint32_t kDropMaxOrdinal = 65536;
// 2^63 | (counter mod 2^47) << 16 | ordinal: bit 63 keeps a step's masks apart from the host counter's offsets 0, 1, 2, ...
__host__ __device__ __forceinline__ uint64_t drop_step_offset(uint64_t counter, uint32_t ordinal) {
  return (1ull << 63) | ((counter & ((1ull << 47) - 1)) << 16) | (uint64_t)ordinal;
}

__host__ __device__ __forceinline__ DropRng drop_rng_of(uint64_t seed, uint64_t offset, float p, float scale) {
  DropRng g;
  g.key = make_uint2((uint32_t)seed, (uint32_t)(seed >> 32));
  g.off_lo = (uint32_t)offset;
  g.off_hi = (uint32_t)(offset >> 32);
  g.p = p;
  g.scale = scale;
  return g;
}

// the DropRng of a kernel with dropout; without dropout nothing is read (seed_ctr may be null)
template <bool DROP>
__device__ __forceinline__ DropRng drop_source(const DropRng& g) { return g; }
template <bool DROP>
__device__ __forceinline__ DropRng drop_source(const DropDev& d) {
  if (!DROP) return drop_rng_of(0, 0, d.p, d.scale);
  const uint64_t seed = (uint64_t)d.seed_ctr[0], counter = (uint64_t)d.seed_ctr[1];      // (the same address in every lane: one scalar load)
  return drop_rng_of(seed, drop_step_offset(counter, d.ordinal), d.p, d.scale);
}

__device__ __forceinline__ uint32_t pick_word(const uint4& r, uint32_t w) { return w == 0 ? r.x : (w == 1 ? r.y : (w == 2 ? r.z : r.w)); }
__device__ __forceinline__ uint4 drop_quad(const DropRng& g, uint64_t quad) {
  return philox4x32(make_uint4((uint32_t)quad, (uint32_t)(quad >> 32), g.off_lo, g.off_hi), g.key);
}
// keep scale (1 / (1 - p) or 0) of element e
__device__ __forceinline__ float drop_keep(const DropRng& g, uint64_t e) {
  return u01(pick_word(drop_quad(g, e >> 2), (uint32_t)e & 3u)) >= g.p ? g.scale : 0.0f;
}
// ... for a thread that walks consecutive e: one Philox call per four elements
struct QuadCache {
  uint64_t quad;
  uint4 r;
};
__device__ __forceinline__ float drop_keep(const DropRng& g, QuadCache& c, uint64_t e) {
  const uint64_t quad = e >> 2;
  if (quad != c.quad) {
    c.quad = quad;
    c.r = drop_quad(g, quad);
  }
  return u01(pick_word(c.r, (uint32_t)e & 3u)) >= g.p ? g.scale : 0.0f;
}

__device__ __forceinline__ float dot4(const float4& a, const float4& b) { return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x))); }
__device__ __forceinline__ void axpy4(float4& acc, float a, const float4& x) {
  acc.x = fmaf(a, x.x, acc.x); acc.y = fmaf(a, x.y, acc.y); acc.z = fmaf(a, x.z, acc.z); acc.w = fmaf(a, x.w, acc.w);
}
__device__ __forceinline__ float4 scale4(const float4& a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }

// the r-th index a thread takes: pair p = (0 .. ceil(L/2)-1) gives rows p and L-1-p (the middle row of an odd L once)
#define EVAE_ATTN_FOR_ROWS(i)                                                   \
  for (int p_ = threadIdx.x; p_ < (L + 1) / 2; p_ += kAttnThreads)              \
    for (int half_ = 0, i = p_; half_ < 2 && !(half_ == 1 && L - 1 - p_ == p_); ++half_, i = L - 1 - p_)

// float4 index of row i of head h of image b in a [B*L, H*4] matrix: (b L + i) H + h
template <bool DROP, class Src>
__global__ __launch_bounds__(kAttnThreads) void attn_fwd_kernel(const float4* __restrict__ q, const float4* __restrict__ k,
                                                                const float4* __restrict__ v, int H, int L, Src src,
                                                                float4* __restrict__ out, float* __restrict__ lse) {
  const DropRng g = drop_source<DROP>(src);
  extern __shared__ float4 attn_smem[];
  float4* sk = attn_smem;
  float4* sv = attn_smem + L;
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const size_t base = (size_t)b * L * H + h;
  for (int j = threadIdx.x; j < L; j += kAttnThreads) {
    sk[j] = k[base + (size_t)j * H];
    sv[j] = v[base + (size_t)j * H];
  }
  __syncthreads();
  EVAE_ATTN_FOR_ROWS(i) {
    const float4 qi = scale4(q[base + (size_t)i * H], 0.5f);          // 1 / sqrt(dh), dh = 4: exact
    float m = -INFINITY;
    for (int j = 0; j < i; ++j) m = fmaxf(m, dot4(qi, sk[j]));
    float sum = 0.f;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    const uint64_t e0 = ((uint64_t)bh * L + i) * L;
    QuadCache qc;
    qc.quad = ~0ull;
    for (int j = 0; j < i; ++j) {
      const float pe = expf(dot4(qi, sk[j]) - m);
      sum += pe;
      axpy4(acc, DROP ? pe * drop_keep(g, qc, e0 + j) : pe, sv[j]);
    }
    const float inv = i > 0 ? 1.0f / sum : 0.f;
    out[base + (size_t)i * H] = scale4(acc, inv);
    lse[(size_t)bh * L + i] = i > 0 ? m + logf(sum) : 0.f;
  }
}

template <bool DROP, class Src>
__global__ __launch_bounds__(kAttnThreads) void attn_bwd_dq_kernel(const float4* __restrict__ q, const float4* __restrict__ k,
                                                                   const float4* __restrict__ v, const float4* __restrict__ out,
                                                                   const float* __restrict__ lse, const float4* __restrict__ dout,
                                                                   int H, int L, Src src, float4* __restrict__ dq,
                                                                   float* __restrict__ delta_out) {
#pragma clang fp contract(off)
  const DropRng g = drop_source<DROP>(src);
  extern __shared__ float4 attn_smem[];
  float4* sk = attn_smem;
  float4* sv = attn_smem + L;
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const size_t base = (size_t)b * L * H + h;
  for (int j = threadIdx.x; j < L; j += kAttnThreads) {
    sk[j] = k[base + (size_t)j * H];
    sv[j] = v[base + (size_t)j * H];
  }
  __syncthreads();
  EVAE_ATTN_FOR_ROWS(i) {
    const size_t o = base + (size_t)i * H;
    const float4 qi = scale4(q[o], 0.5f), doi = dout[o];
    const float li = lse[(size_t)bh * L + i], shift = dot4(doi, out[o]);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f), pk = make_float4(0.f, 0.f, 0.f, 0.f);      // sum p (dp - shift) k_j, sum p k_j
    float pdsum = 0.f, psum = 0.f;
    const uint64_t e0 = ((uint64_t)bh * L + i) * L;
    QuadCache qc;
    qc.quad = ~0ull;
    for (int j = 0; j < i; ++j) {
      const float4 kj = sk[j];
      const float p = expf(dot4(qi, kj) - li);
      float dp = dot4(doi, sv[j]);
      if (DROP) dp *= drop_keep(g, qc, e0 + j);
      pdsum += p * dp;
      psum += p;
      axpy4(acc, p * (dp - shift), kj);
      axpy4(pk, p, kj);
    }
    const float delta = i > 0 ? pdsum / psum : 0.f, corr = delta - shift;
    dq[o] = make_float4(0.5f * (acc.x - corr * pk.x), 0.5f * (acc.y - corr * pk.y), 0.5f * (acc.z - corr * pk.z),
                        0.5f * (acc.w - corr * pk.w));
    delta_out[(size_t)bh * L + i] = delta;
  }
}

template <bool DROP, class Src>
__global__ __launch_bounds__(kAttnThreads) void attn_bwd_dkv_kernel(const float4* __restrict__ q, const float4* __restrict__ k,
                                                                    const float4* __restrict__ v, const float* __restrict__ lse,
                                                                    const float* __restrict__ delta, const float4* __restrict__ dout,
                                                                    int H, int L, Src src, float4* __restrict__ dk,
                                                                    float4* __restrict__ dv) {
#pragma clang fp contract(off)
  const DropRng g = drop_source<DROP>(src);
  extern __shared__ float4 attn_smem[];
  float4* sq = attn_smem;                                   // q_i / sqrt(dh)
  float4* sdo = attn_smem + L;
  float* slse = reinterpret_cast<float*>(attn_smem + 2 * (size_t)L);
  float* sdelta = slse + L;
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const size_t base = (size_t)b * L * H + h;
  for (int i = threadIdx.x; i < L; i += kAttnThreads) {
    const size_t o = base + (size_t)i * H;
    const float4 doi = dout[o];
    sq[i] = scale4(q[o], 0.5f);
    sdo[i] = doi;
    slse[i] = lse[(size_t)bh * L + i];
    sdelta[i] = delta[(size_t)bh * L + i];
  }
  __syncthreads();
  EVAE_ATTN_FOR_ROWS(j) {
    const size_t o = base + (size_t)j * H;
    const float4 kj = k[o], vj = v[o];
    float4 ak = make_float4(0.f, 0.f, 0.f, 0.f), av = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i = L - 1; i > j; --i) {                       // (row 0 is never an i here: its p is zero)
      const float4 qi = sq[i], doi = sdo[i];
      const float p = expf(dot4(qi, kj) - slse[i]);
      float dp = dot4(doi, vj), pm = p;
      if (DROP) {
        const float keep = drop_keep(g, ((uint64_t)bh * L + i) * L + j);
        dp *= keep;
        pm *= keep;
      }
      axpy4(av, pm, doi);
      axpy4(ak, p * (dp - sdelta[i]), qi);
    }
    dk[o] = ak;
    dv[o] = av;
  }
}

// ---- ELU -> dropout ---------------------------------------------------------------------------------------------------------------------
// one thread = one quad of the flat index = one Philox call
template <bool DROP, class Src>
__global__ __launch_bounds__(256) void elu_dropout_fwd_kernel(const float* __restrict__ x, size_t n, Src src, float* __restrict__ out) {
  const DropRng g = drop_source<DROP>(src);
  const size_t quad = (size_t)blockIdx.x * 256 + threadIdx.x, e0 = quad * 4;
  if (e0 >= n) return;
  uint4 r = make_uint4(0, 0, 0, 0);
  if (DROP) r = drop_quad(g, quad);
  const uint32_t rr[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (e0 + t >= n) break;
    const float xv = x[e0 + t];
    float a = xv > 0.f ? xv : expm1f(xv);
    if (DROP) a *= u01(rr[t]) >= g.p ? g.scale : 0.f;
    out[e0 + t] = a;
  }
}

template <bool DROP, class Src>
__global__ __launch_bounds__(256) void elu_dropout_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, size_t n, Src src,
                                                              float* __restrict__ dx) {
  const DropRng g = drop_source<DROP>(src);
  const size_t quad = (size_t)blockIdx.x * 256 + threadIdx.x, e0 = quad * 4;
  if (e0 >= n) return;
  uint4 r = make_uint4(0, 0, 0, 0);
  if (DROP) r = drop_quad(g, quad);
  const uint32_t rr[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (e0 + t >= n) break;
    const float xv = x[e0 + t];
    float d = dy[e0 + t] * (xv > 0.f ? 1.0f : expf(xv));
    if (DROP) d *= u01(rr[t]) >= g.p ? g.scale : 0.f;
    dx[e0 + t] = d;
  }
}

// ---- GLU residual: out[m, c] = ab[m, c] * sigmoid(ab[m, C + c]) + x[m, c] ------------------------------------------------------------------
__device__ __forceinline__ float sigmoid_exact(float b) { return 1.0f / (1.0f + expf(-b)); }

__global__ __launch_bounds__(256) void glu_res_fwd_kernel(const float* __restrict__ ab, const float* __restrict__ x, size_t n, int Cc,
                                                          float* __restrict__ out) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const size_t m = e / (size_t)Cc, c = e - m * Cc;
  const float a = ab[m * 2 * Cc + c], b = ab[m * 2 * Cc + Cc + c];
  out[e] = fmaf(a, sigmoid_exact(b), x[e]);
}

__global__ __launch_bounds__(256) void glu_res_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ ab, size_t n, int Cc,
                                                          float* __restrict__ dab) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const size_t m = e / (size_t)Cc, c = e - m * Cc;
  const float a = ab[m * 2 * Cc + c], s = sigmoid_exact(ab[m * 2 * Cc + Cc + c]), d = dout[e];
  dab[m * 2 * Cc + c] = d * s;
  dab[m * 2 * Cc + Cc + c] = d * a * s * (1.0f - s);
}

bool drop_p_ok(const char* what, float p_drop) {
  if (!(p_drop >= 0.f && p_drop < 1.f)) {
    set_error("%s: p_drop %g outside [0, 1)", what, (double)p_drop);
    return false;
  }
  return true;
}

bool drop_rng(const char* what, float p_drop, uint64_t seed, uint64_t offset, DropRng* g) {
  if (!drop_p_ok(what, p_drop)) return false;
  *g = drop_rng_of(seed, offset, p_drop, 1.0f / (1.0f - p_drop));
  return true;
}

// the source of a *_dev launch; p_drop = 0 never reads seed_ctr, so it may be null then
bool drop_dev(const char* what, float p_drop, const int64_t* seed_ctr, uint32_t ordinal, DropDev* d) {
  if (!drop_p_ok(what, p_drop)) return false;
  if (ordinal >= kDropMaxOrdinal) {
    set_error("%s: dropout ordinal %u does not fit the step offset (< %u)", what, ordinal, kDropMaxOrdinal);
    return false;
  }
  if (p_drop > 0.f && (seed_ctr == nullptr || ((uintptr_t)seed_ctr & 7) != 0)) {
    set_error("%s: seed_ctr is null or not 8-byte aligned", what);
    return false;
  }
  d->seed_ctr = seed_ctr;
  d->ordinal = ordinal;
  d->p = p_drop;
  d->scale = 1.0f / (1.0f - p_drop);
  return true;
}

bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}

int attn_check(const char* what, int B, int H, int L, int dh) {
  EVAE_REQUIRE(dh == kAttnDh, "%s: head width %d is not supported (dh = %d only)", what, dh, kAttnDh);
  EVAE_REQUIRE(B >= 0 && H > 0 && L > 0, "%s: bad sizes", what);
  EVAE_REQUIRE(evae_causal_attn_lds_bytes(L, 0) != 0, "%s: L = %d exceeds the LDS plan (L <= %d)", what, L, kAttnMaxLen);
  EVAE_REQUIRE((int64_t)B * H <= 0x7fffffffLL, "%s: B * H does not fit a launch grid", what);
  return EVAE_OK;
}

}  // namespace
}  // namespace evae

using namespace evae;

extern "C" int evae_causal_attn_max_len(void) { return kAttnMaxLen; }

extern "C" size_t evae_causal_attn_lds_bytes(int L, int pass) {
  if (L <= 0 || L > kAttnMaxLen || pass < 0 || pass > 1) return 0;
  return pass == 0 ? (size_t)L * 2 * sizeof(float4) : (size_t)L * (2 * sizeof(float4) + 2 * sizeof(float));
}

// The launches behind the host-argument entry points (Src = DropRng) and the *_dev ones (Src = DropDev): one body each.
namespace {

template <class Src>
int attn_fwd_launch(const char* what, const float* q, const float* k, const float* v, int B, int H, int L, const Src& g, float* out,
                    float* lse, evae_stream_t s) {
  if (B == 0) return EVAE_OK;
  EVAE_REQUIRE(q && k && v && out && lse && aligned16(q, k, v, out), "%s: null or unaligned pointer", what);
  const size_t lds = evae_causal_attn_lds_bytes(L, 0);
  const float4 *q4 = (const float4*)q, *k4 = (const float4*)k, *v4 = (const float4*)v;
  if (g.p > 0.f)
    attn_fwd_kernel<true><<<B * H, kAttnThreads, lds, (hipStream_t)s>>>(q4, k4, v4, H, L, g, (float4*)out, lse);
  else
    attn_fwd_kernel<false><<<B * H, kAttnThreads, lds, (hipStream_t)s>>>(q4, k4, v4, H, L, g, (float4*)out, lse);
  return check_launch(what);
}

template <class Src>
int attn_bwd_launch(const char* what, const float* q, const float* k, const float* v, const float* out, const float* lse,
                    const float* dout, int B, int H, int L, const Src& g, float* delta, float* dq, float* dk, float* dv,
                    evae_stream_t s) {
  if (B == 0) return EVAE_OK;
  EVAE_REQUIRE(q && k && v && out && lse && dout && delta && dq && dk && dv && aligned16(q, k, v, out) && aligned16(dout, dq, dk, dv),
               "%s: null or unaligned pointer", what);
  const size_t lds0 = evae_causal_attn_lds_bytes(L, 0), lds1 = evae_causal_attn_lds_bytes(L, 1);
  const float4 *q4 = (const float4*)q, *k4 = (const float4*)k, *v4 = (const float4*)v, *o4 = (const float4*)out, *d4 = (const float4*)dout;
  if (g.p > 0.f) {
    attn_bwd_dq_kernel<true><<<B * H, kAttnThreads, lds0, (hipStream_t)s>>>(q4, k4, v4, o4, lse, d4, H, L, g, (float4*)dq, delta);
    attn_bwd_dkv_kernel<true><<<B * H, kAttnThreads, lds1, (hipStream_t)s>>>(q4, k4, v4, lse, delta, d4, H, L, g, (float4*)dk, (float4*)dv);
  } else {
    attn_bwd_dq_kernel<false><<<B * H, kAttnThreads, lds0, (hipStream_t)s>>>(q4, k4, v4, o4, lse, d4, H, L, g, (float4*)dq, delta);
    attn_bwd_dkv_kernel<false><<<B * H, kAttnThreads, lds1, (hipStream_t)s>>>(q4, k4, v4, lse, delta, d4, H, L, g, (float4*)dk, (float4*)dv);
  }
  return check_launch(what);
}

template <class Src>
int elu_dropout_fwd_launch(const char* what, const float* x, size_t n, const Src& g, float* out, evae_stream_t s) {
  if (n == 0) return EVAE_OK;
  EVAE_REQUIRE(x && out, "%s: null pointer", what);
  const size_t nblk = ((n + 3) / 4 + 255) / 256;
  EVAE_REQUIRE(nblk <= 0x7fffffffu, "%s: too many elements", what);
  if (g.p > 0.f)
    elu_dropout_fwd_kernel<true><<<(unsigned)nblk, 256, 0, (hipStream_t)s>>>(x, n, g, out);
  else
    elu_dropout_fwd_kernel<false><<<(unsigned)nblk, 256, 0, (hipStream_t)s>>>(x, n, g, out);
  return check_launch(what);
}

template <class Src>
int elu_dropout_bwd_launch(const char* what, const float* dy, const float* x, size_t n, const Src& g, float* dx, evae_stream_t s) {
  if (n == 0) return EVAE_OK;
  EVAE_REQUIRE(dy && x && dx, "%s: null pointer", what);
  const size_t nblk = ((n + 3) / 4 + 255) / 256;
  EVAE_REQUIRE(nblk <= 0x7fffffffu, "%s: too many elements", what);
  if (g.p > 0.f)
    elu_dropout_bwd_kernel<true><<<(unsigned)nblk, 256, 0, (hipStream_t)s>>>(dy, x, n, g, dx);
  else
    elu_dropout_bwd_kernel<false><<<(unsigned)nblk, 256, 0, (hipStream_t)s>>>(dy, x, n, g, dx);
  return check_launch(what);
}

}  // namespace

extern "C" uint64_t evae_dropout_step_offset(uint64_t counter, uint32_t ordinal) {
  return ordinal < kDropMaxOrdinal ? drop_step_offset(counter, ordinal) : 0;
}

extern "C" int evae_causal_attn_fwd(const float* q, const float* k, const float* v, int B, int H, int L, int dh, float p_drop,
                                    uint64_t seed, uint64_t offset, float* out, float* lse, evae_stream_t s) {
  if (int rc = attn_check("causal_attn_fwd", B, H, L, dh)) return rc;
  DropRng g;
  if (!drop_rng("causal_attn_fwd", p_drop, seed, offset, &g)) return EVAE_EINVAL;
  return attn_fwd_launch("causal_attn_fwd", q, k, v, B, H, L, g, out, lse, s);
}

extern "C" int evae_causal_attn_fwd_dev(const float* q, const float* k, const float* v, int B, int H, int L, int dh, float p_drop,
                                        const int64_t* seed_ctr, uint32_t ordinal, float* out, float* lse, evae_stream_t s) {
  if (int rc = attn_check("causal_attn_fwd_dev", B, H, L, dh)) return rc;
  DropDev g;
  if (!drop_dev("causal_attn_fwd_dev", p_drop, seed_ctr, ordinal, &g)) return EVAE_EINVAL;
  return attn_fwd_launch("causal_attn_fwd_dev", q, k, v, B, H, L, g, out, lse, s);
}

extern "C" int evae_causal_attn_bwd(const float* q, const float* k, const float* v, const float* out, const float* lse,
                                    const float* dout, int B, int H, int L, int dh, float p_drop, uint64_t seed, uint64_t offset,
                                    float* delta, float* dq, float* dk, float* dv, evae_stream_t s) {
  if (int rc = attn_check("causal_attn_bwd", B, H, L, dh)) return rc;
  DropRng g;
  if (!drop_rng("causal_attn_bwd", p_drop, seed, offset, &g)) return EVAE_EINVAL;
  return attn_bwd_launch("causal_attn_bwd", q, k, v, out, lse, dout, B, H, L, g, delta, dq, dk, dv, s);
}

extern "C" int evae_causal_attn_bwd_dev(const float* q, const float* k, const float* v, const float* out, const float* lse,
                                        const float* dout, int B, int H, int L, int dh, float p_drop, const int64_t* seed_ctr,
                                        uint32_t ordinal, float* delta, float* dq, float* dk, float* dv, evae_stream_t s) {
  if (int rc = attn_check("causal_attn_bwd_dev", B, H, L, dh)) return rc;
  DropDev g;
  if (!drop_dev("causal_attn_bwd_dev", p_drop, seed_ctr, ordinal, &g)) return EVAE_EINVAL;
  return attn_bwd_launch("causal_attn_bwd_dev", q, k, v, out, lse, dout, B, H, L, g, delta, dq, dk, dv, s);
}

extern "C" int evae_elu_dropout_fwd(const float* x, size_t n, float p_drop, uint64_t seed, uint64_t offset, float* out, evae_stream_t s) {
  DropRng g;
  if (!drop_rng("elu_dropout_fwd", p_drop, seed, offset, &g)) return EVAE_EINVAL;
  return elu_dropout_fwd_launch("elu_dropout_fwd", x, n, g, out, s);
}

extern "C" int evae_elu_dropout_fwd_dev(const float* x, size_t n, float p_drop, const int64_t* seed_ctr, uint32_t ordinal, float* out,
                                        evae_stream_t s) {
  DropDev g;
  if (!drop_dev("elu_dropout_fwd_dev", p_drop, seed_ctr, ordinal, &g)) return EVAE_EINVAL;
  return elu_dropout_fwd_launch("elu_dropout_fwd_dev", x, n, g, out, s);
}

extern "C" int evae_elu_dropout_bwd(const float* dy, const float* x, size_t n, float p_drop, uint64_t seed, uint64_t offset, float* dx,
                                    evae_stream_t s) {
  DropRng g;
  if (!drop_rng("elu_dropout_bwd", p_drop, seed, offset, &g)) return EVAE_EINVAL;
  return elu_dropout_bwd_launch("elu_dropout_bwd", dy, x, n, g, dx, s);
}

extern "C" int evae_elu_dropout_bwd_dev(const float* dy, const float* x, size_t n, float p_drop, const int64_t* seed_ctr, uint32_t ordinal,
                                        float* dx, evae_stream_t s) {
  DropDev g;
  if (!drop_dev("elu_dropout_bwd_dev", p_drop, seed_ctr, ordinal, &g)) return EVAE_EINVAL;
  return elu_dropout_bwd_launch("elu_dropout_bwd_dev", dy, x, n, g, dx, s);
}

extern "C" int evae_glu_res_fwd(const float* ab, const float* x, int64_t M, int C, float* out, evae_stream_t s) {
  EVAE_REQUIRE(M >= 0 && C > 0, "glu_res_fwd: bad sizes");
  if (M == 0) return EVAE_OK;
  EVAE_REQUIRE(ab && x && out, "glu_res_fwd: null pointer");
  const size_t n = (size_t)M * C, nblk = (n + 255) / 256;
  EVAE_REQUIRE(nblk <= 0x7fffffffu, "glu_res_fwd: too many elements");
  glu_res_fwd_kernel<<<(unsigned)nblk, 256, 0, (hipStream_t)s>>>(ab, x, n, C, out);
  return check_launch("glu_res_fwd");
}

extern "C" int evae_glu_res_bwd(const float* dout, const float* ab, int64_t M, int C, float* dab, evae_stream_t s) {
  EVAE_REQUIRE(M >= 0 && C > 0, "glu_res_bwd: bad sizes");
  if (M == 0) return EVAE_OK;
  EVAE_REQUIRE(dout && ab && dab, "glu_res_bwd: null pointer");
  const size_t n = (size_t)M * C, nblk = (n + 255) / 256;
  EVAE_REQUIRE(nblk <= 0x7fffffffu, "glu_res_bwd: too many elements");
  glu_res_bwd_kernel<<<(unsigned)nblk, 256, 0, (hipStream_t)s>>>(dout, ab, n, C, dab);
  return check_launch("glu_res_bwd");
}
