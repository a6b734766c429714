// VampPrior: log-density of z_i under a uniform mixture of diagonal Gaussians with PER-COMPONENT mean and log-variance
// (reference models/BaseModel.py:84-96,124-128), its backward by recomputation, and the pseudo-input transpose + clamp.
//
//   p_ij = cst_j - 1/2 sum_d (z_id - mu_jd)^2 w_jd,   w_jd = exp(-lv_jd),   cst_j = -1/2 sum_d (lv_jd + log 2 pi)
//
// Layout: a wave owns a row (a query in the query-side kernel, a component in the component-side kernel) and its lanes own
// the latent dimensions d = lane, lane + 64, ... (NCH chunks of 64, zdim <= 512), so the row sits in registers at any zdim; the
// sum over d is the xor butterfly, which leaves the SAME bits in every lane.  Direct differences on the VALU: with lv down to
// -6, w reaches 403 and the expanded form z^2 w - 2 z mu w + mu^2 w cancels in fp32.
// The forward, the dz kernel and the dmu/dlv kernel all form p_ij through pair_acc() / the butterfly / one fma, in the same
// order: p_ij is bit-identical in the three, so (p_ij - M_i) is exact where the weight matters and exp((p_ij - M_i) - log sum)
// stays a normalised softmax at any magnitude of the log-density (the token convention of evae_prior_merge).
// Every reduction has a fixed order; there are no floating-point atomics.
#include "evae_common.h"

namespace evae {
namespace {

constexpr int MQ_WAVES = 8;            // query-side kernel: waves per block ...
constexpr int MQ_QPW = 2;              // ... queries per wave (each LDS read of a component serves both)
constexpr int MQ_QPB = MQ_WAVES * MQ_QPW;
constexpr int MQ_TILE = 4096;          // floats per staged array (mu, w): 2 x 16 KiB of LDS per block
constexpr int MQ_TC_MAX = 64;          // components per staged tile: min(64, MQ_TILE / (64 NCH)), always a multiple of 4
constexpr int MC_WAVES = 4;            // component-side kernel: waves (= components) per block

// one term of the distance; explicit roundings so that no kernel contracts it differently from another
__device__ __forceinline__ float pair_acc(float acc, float z, float mu, float w) {
  const float t = __fsub_rn(z, mu);
  return __fmaf_rn(__fmul_rn(t, t), w, acc);
}

// a wave reads one component's log-variance row: w (this lane's dimensions) and cst_j (all lanes)
template <int NCH>
__device__ __forceinline__ float component_consts(const float* __restrict__ lv_row, int zdim, int lane, float (&w)[NCH]) {
  float part = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int d = c * 64 + lane;
    const bool in = d < zdim;
    const float lv = in ? lv_row[d] : 0.f;
    w[c] = in ? expf(-lv) : 0.f;
    part += in ? (lv + kLog2Pi) : 0.f;
  }
  return -0.5f * wave_sum(part);
}

// ------------------------------------------------------------------------------------------------
// query side: blockIdx.x = 16 queries, blockIdx.y = one split of the component range.
//   BWD = false: online log-sum-exp over the split -> partial planes (max, sumexp, 0) [nsplit x B]; optional prob [B x C]
//   BWD = true : r_ij = g_i exp((p_ij - M_i) - log sum_i), dz_i += r_ij (mu_j - z_i) w_j -> the split's dz partial
// ------------------------------------------------------------------------------------------------
template <int NCH, bool BWD>
__global__ __launch_bounds__(MQ_WAVES * 64) void mixture_query_kernel(
    const float* __restrict__ z, int B, const float* __restrict__ mu, const float* __restrict__ lv, int C, int zdim, int cps,
    float logn, float* __restrict__ pm, float* __restrict__ ps, float* __restrict__ pn, float* __restrict__ prob,
    const float* __restrict__ token, const float* __restrict__ gout, float* __restrict__ dz_out) {
  constexpr int ZP = NCH * 64;
  constexpr int TC = (MQ_TILE / ZP) < MQ_TC_MAX ? (MQ_TILE / ZP) : MQ_TC_MAX;
  __shared__ float s_mu[MQ_TILE];
  __shared__ float s_w[MQ_TILE];
  __shared__ float s_cst[MQ_TC_MAX];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int split = blockIdx.y;
  const int c_lo = split * cps;
  const int c_hi = min(C, c_lo + cps);
  const int q0 = blockIdx.x * MQ_QPB + wave * MQ_QPW;

  float zr[MQ_QPW][NCH];
  float m[MQ_QPW], s[MQ_QPW], M[MQ_QPW], ls[MQ_QPW], g[MQ_QPW];
  float dz[MQ_QPW][NCH];
#pragma unroll
  for (int qi = 0; qi < MQ_QPW; ++qi) {
    const int q = q0 + qi;
    const bool qv = q < B;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int d = c * 64 + lane;
      zr[qi][c] = (qv && d < zdim) ? z[(size_t)q * zdim + d] : 0.f;
      dz[qi][c] = 0.f;
    }
    m[qi] = -INFINITY; s[qi] = 0.f;
    M[qi] = 0.f; ls[qi] = 0.f; g[qi] = 0.f;
    if (BWD && qv) { M[qi] = token[q]; ls[qi] = token[B + q]; g[qi] = gout[q]; }
  }

  for (int t0 = c_lo; t0 < c_hi; t0 += TC) {
    __syncthreads();
    // stage the tile: one exp per component element; slots past the split's end are neutral (w = 0, cst = -inf)
    for (int jj = wave; jj < TC; jj += MQ_WAVES) {
      const int j = t0 + jj;
      float w[NCH];
      float cst = -INFINITY;
      if (j < c_hi) {
        cst = component_consts<NCH>(lv + (size_t)j * zdim, zdim, lane, w);
      } else {
#pragma unroll
        for (int c = 0; c < NCH; ++c) w[c] = 0.f;
      }
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int d = c * 64 + lane;
        s_mu[jj * ZP + d] = (j < c_hi && d < zdim) ? mu[(size_t)j * zdim + d] : 0.f;
        s_w[jj * ZP + d] = w[c];
      }
      if (lane == 0) s_cst[jj] = cst;
    }
    __syncthreads();
    const int nt = min(TC, (c_hi - t0 + 3) & ~3);
    for (int jj = 0; jj < nt; jj += 4) {
      float p[MQ_QPW][4];
#pragma unroll
      for (int qi = 0; qi < MQ_QPW; ++qi)
#pragma unroll
        for (int k = 0; k < 4; ++k) p[qi][k] = 0.f;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float mv = s_mu[(jj + k) * ZP + c * 64 + lane];
          const float wv = s_w[(jj + k) * ZP + c * 64 + lane];
#pragma unroll
          for (int qi = 0; qi < MQ_QPW; ++qi) p[qi][k] = pair_acc(p[qi][k], zr[qi][c], mv, wv);
        }
      }
#pragma unroll
      for (int qi = 0; qi < MQ_QPW; ++qi)
#pragma unroll
        for (int k = 0; k < 4; ++k) p[qi][k] = __fmaf_rn(-0.5f, wave_sum(p[qi][k]), s_cst[jj + k]);

      if (!BWD) {
#pragma unroll
        for (int qi = 0; qi < MQ_QPW; ++qi) {
          const float mn = fmaxf(fmaxf(m[qi], fmaxf(p[qi][0], p[qi][1])), fmaxf(p[qi][2], p[qi][3]));
          // the first slot of a split is a real component, so mn is finite from the first group on
          s[qi] = s[qi] * expf(m[qi] - mn) + ((expf(p[qi][0] - mn) + expf(p[qi][1] - mn)) + (expf(p[qi][2] - mn) + expf(p[qi][3] - mn)));
          m[qi] = mn;
          if (prob != nullptr) {
            const int q = q0 + qi, j = t0 + jj + lane;
            const float pv = lane == 0 ? p[qi][0] : lane == 1 ? p[qi][1] : lane == 2 ? p[qi][2] : p[qi][3];
            if (lane < 4 && q < B && j < c_hi) prob[(size_t)q * C + j] = pv - logn;
          }
        }
      } else {
        float r[MQ_QPW][4];
#pragma unroll
        for (int qi = 0; qi < MQ_QPW; ++qi)
#pragma unroll
          for (int k = 0; k < 4; ++k) r[qi][k] = g[qi] * expf((p[qi][k] - M[qi]) - ls[qi]);
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float mv = s_mu[(jj + k) * ZP + c * 64 + lane];
            const float wv = s_w[(jj + k) * ZP + c * 64 + lane];
#pragma unroll
            for (int qi = 0; qi < MQ_QPW; ++qi) dz[qi][c] += r[qi][k] * ((mv - zr[qi][c]) * wv);
          }
        }
      }
    }
  }

#pragma unroll
  for (int qi = 0; qi < MQ_QPW; ++qi) {
    const int q = q0 + qi;
    if (q >= B) continue;
    if (!BWD) {
      if (lane == 0) {
        pm[(size_t)split * B + q] = m[qi];
        ps[(size_t)split * B + q] = s[qi];
        pn[(size_t)split * B + q] = 0.f;
      }
    } else {
      float* dst = dz_out + ((size_t)split * B + q) * zdim;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int d = c * 64 + lane;
        if (d < zdim) dst[d] = dz[qi][c];
      }
    }
  }
}

// dz = sum over the splits' partials, split 0 first
__global__ __launch_bounds__(256) void mixture_dz_reduce_kernel(const float* __restrict__ part, int nsplit, size_t n,
                                                                float* __restrict__ dz) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float a = part[i];
  for (int sp = 1; sp < nsplit; ++sp) a += part[(size_t)sp * n + i];
  dz[i] = a;
}

// ------------------------------------------------------------------------------------------------
// component side: a wave owns component j (mu, w, the two gradient rows in registers) and walks every query in order, four at
// a time: dmu_j and dlv_j are finished by their wave, no cross-block traffic.
// ------------------------------------------------------------------------------------------------
template <int NCH>
__global__ __launch_bounds__(MC_WAVES * 64) void mixture_component_kernel(
    const float* __restrict__ z, int B, const float* __restrict__ mu, const float* __restrict__ lv, int C, int zdim,
    const float* __restrict__ token, const float* __restrict__ gout, float* __restrict__ dmu, float* __restrict__ dlv) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * MC_WAVES + (threadIdx.x >> 6);
  if (j >= C) return;
  float mr[NCH], w[NCH], am[NCH], al[NCH];
  const float cst = component_consts<NCH>(lv + (size_t)j * zdim, zdim, lane, w);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int d = c * 64 + lane;
    mr[c] = d < zdim ? mu[(size_t)j * zdim + d] : 0.f;
    am[c] = 0.f; al[c] = 0.f;
  }
  for (int qb = 0; qb < B; qb += 4) {
    float zr[4][NCH], acc[4], M[4], ls[4], g[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int q = min(qb + k, B - 1);
      const bool qv = qb + k < B;
      M[k] = token[q]; ls[k] = token[B + q]; g[k] = qv ? gout[q] : 0.f;
      acc[k] = 0.f;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int d = c * 64 + lane;
        zr[k][c] = d < zdim ? z[(size_t)q * zdim + d] : 0.f;
        acc[k] = pair_acc(acc[k], zr[k][c], mr[c], w[c]);
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float p = __fmaf_rn(-0.5f, wave_sum(acc[k]), cst);
      const float r = g[k] * expf((p - M[k]) - ls[k]);
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const float t = zr[k][c] - mr[c];
        const float tw = t * w[c];
        am[c] += r * tw;
        al[c] += r * (0.5f * (t * tw - 1.f));
      }
    }
  }
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int d = c * 64 + lane;
    if (d < zdim) {
      if (dmu != nullptr) dmu[(size_t)j * zdim + d] = am[c];
      if (dlv != nullptr) dlv[(size_t)j * zdim + d] = al[c];
    }
  }
}

// ------------------------------------------------------------------------------------------------
// pseudo-inputs X[c, d] = clamp(W[d, c], 0, 1): 64 x 64 tiles through LDS, rows of 65 floats so that the transposed read
// (lane stride 65) touches 64 different banks.
// ------------------------------------------------------------------------------------------------
constexpr int PT = 64;

__global__ __launch_bounds__(256) void pseudo_inputs_fwd_kernel(const float* __restrict__ W, int D, int C, float* __restrict__ X) {
  __shared__ float tile[PT][PT + 1];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c0 = blockIdx.x * PT, d0 = blockIdx.y * PT;
  for (int r = ty; r < PT; r += 4) {
    const int d = d0 + r, c = c0 + tx;
    if (d < D && c < C) tile[r][tx] = fminf(fmaxf(W[(size_t)d * C + c], 0.f), 1.f);
  }
  __syncthreads();
  for (int r = ty; r < PT; r += 4) {
    const int c = c0 + r, d = d0 + tx;
    if (c < C && d < D) X[(size_t)c * D + d] = tile[tx][r];
  }
}

__global__ __launch_bounds__(256) void pseudo_inputs_bwd_kernel(const float* __restrict__ W, const float* __restrict__ dX, int D,
                                                                int C, float* __restrict__ dW) {
  __shared__ float tile[PT][PT + 1];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c0 = blockIdx.x * PT, d0 = blockIdx.y * PT;
  for (int r = ty; r < PT; r += 4) {
    const int c = c0 + r, d = d0 + tx;
    if (c < C && d < D) tile[r][tx] = dX[(size_t)c * D + d];
  }
  __syncthreads();
  for (int r = ty; r < PT; r += 4) {
    const int d = d0 + r, c = c0 + tx;
    if (d < D && c < C) {
      const float w = W[(size_t)d * C + c];
      dW[(size_t)d * C + c] = (w > 0.f && w < 1.f) ? tile[tx][r] : 0.f;     // hardtanh backward: strict inequalities
    }
  }
}

struct MixPlan { int nch, tc, nsplit, cps; };

// fixed by (B, C, zdim) alone: the partial layout, and with it the bits of the result, do not depend on the device
MixPlan mix_plan(int B, int C, int zdim) {
  MixPlan p;
  p.nch = zdim <= 64 ? 1 : zdim <= 128 ? 2 : zdim <= 256 ? 4 : 8;
  p.tc = MQ_TILE / (p.nch * 64) < MQ_TC_MAX ? MQ_TILE / (p.nch * 64) : MQ_TC_MAX;
  const int nqb = cdiv(B, MQ_QPB);
  // few queries against many components: split the component range until ~512 blocks are in flight
  int want = 512 / nqb;
  if (want < 1) want = 1;
  int ns = cdiv(C, p.tc);
  if (ns > want) ns = want;
  p.cps = (cdiv(C, ns) + 3) & ~3;
  p.nsplit = cdiv(C, p.cps);
  return p;
}

int check_sizes(const char* what, int B, int C, int zdim) {
  EVAE_REQUIRE(B >= 1 && C >= 1, "%s: bad sizes B=%d C=%d", what, B, C);
  EVAE_REQUIRE(zdim >= 1 && zdim <= 512, "%s: zdim=%d outside [1, 512]", what, zdim);
  return EVAE_OK;
}

}  // namespace
}  // namespace evae

using namespace evae;

extern "C" size_t evae_mixture_lse_fwd_workspace_bytes(int B, int C, int zdim) {
  if (B < 1 || C < 1 || zdim < 1 || zdim > 512) return 256;
  const MixPlan p = mix_plan(B, C, zdim);
  return align_up((size_t)3 * p.nsplit * B * sizeof(float), 256);
}

extern "C" int evae_mixture_lse_fwd(const float* z, int B, const float* means, const float* log_var, int C, int zdim,
                                    float n_components, float* out_logp, float* out_lse, float* out_prob, void* ws,
                                    size_t ws_bytes, evae_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  int rc = check_sizes("mixture_lse_fwd", B, C, zdim);
  if (rc != EVAE_OK) return rc;
  EVAE_REQUIRE(z && means && log_var && out_logp && ws, "mixture_lse_fwd: null pointer");
  EVAE_REQUIRE(n_components > 0.f, "mixture_lse_fwd: n_components=%g must be positive", (double)n_components);
  if (ws_bytes < evae_mixture_lse_fwd_workspace_bytes(B, C, zdim)) {
    set_error("mixture_lse_fwd: workspace %zu < %zu bytes", ws_bytes, evae_mixture_lse_fwd_workspace_bytes(B, C, zdim));
    return EVAE_EWORKSPACE;
  }
  const MixPlan p = mix_plan(B, C, zdim);
  float* pm = (float*)ws;
  float* ps = pm + (size_t)p.nsplit * B;
  float* pn = ps + (size_t)p.nsplit * B;
  const dim3 grid(cdiv(B, MQ_QPB), p.nsplit);
  const float logn = logf(n_components);
#define EVAE_MIX_FWD(N)                                                                                                  \
  mixture_query_kernel<N, false><<<grid, MQ_WAVES * 64, 0, stream>>>(z, B, means, log_var, C, zdim, p.cps, logn, pm, ps, pn, \
                                                                     out_prob, nullptr, nullptr, nullptr)
  switch (p.nch) {
    case 1: EVAE_MIX_FWD(1); break;
    case 2: EVAE_MIX_FWD(2); break;
    case 4: EVAE_MIX_FWD(4); break;
    default: EVAE_MIX_FWD(8); break;
  }
#undef EVAE_MIX_FWD
  rc = check_launch("mixture_query_kernel(fwd)");
  if (rc != EVAE_OK) return rc;
  // the fixed-order merge of the exemplar prior with no masked entries: logp = LSE - log(n_components), and the token
  return evae_prior_merge(pm, ps, pn, p.nsplit, B, n_components, out_logp, out_lse, stream_);
}

extern "C" size_t evae_mixture_lse_bwd_workspace_bytes(int B, int C, int zdim) {
  if (B < 1 || C < 1 || zdim < 1 || zdim > 512) return 256;
  const MixPlan p = mix_plan(B, C, zdim);
  if (p.nsplit == 1) return 256;
  return align_up((size_t)p.nsplit * B * zdim * sizeof(float), 256);
}

extern "C" int evae_mixture_lse_bwd(const float* z, int B, const float* means, const float* log_var, int C, int zdim,
                                    const float* lse, const float* grad_out, float* dz, float* dmeans, float* dlog_var,
                                    void* ws, size_t ws_bytes, evae_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  int rc = check_sizes("mixture_lse_bwd", B, C, zdim);
  if (rc != EVAE_OK) return rc;
  EVAE_REQUIRE(z && means && log_var && lse && grad_out, "mixture_lse_bwd: null pointer");
  const MixPlan p = mix_plan(B, C, zdim);
  if (dz != nullptr) {
    if (p.nsplit > 1 && (ws == nullptr || ws_bytes < evae_mixture_lse_bwd_workspace_bytes(B, C, zdim))) {
      set_error("mixture_lse_bwd: workspace %zu < %zu bytes", ws_bytes, evae_mixture_lse_bwd_workspace_bytes(B, C, zdim));
      return EVAE_EWORKSPACE;
    }
    float* part = p.nsplit > 1 ? (float*)ws : dz;
    const dim3 grid(cdiv(B, MQ_QPB), p.nsplit);
#define EVAE_MIX_DZ(N)                                                                                                    \
  mixture_query_kernel<N, true><<<grid, MQ_WAVES * 64, 0, stream>>>(z, B, means, log_var, C, zdim, p.cps, 0.f, nullptr, nullptr, \
                                                                    nullptr, nullptr, lse, grad_out, part)
    switch (p.nch) {
      case 1: EVAE_MIX_DZ(1); break;
      case 2: EVAE_MIX_DZ(2); break;
      case 4: EVAE_MIX_DZ(4); break;
      default: EVAE_MIX_DZ(8); break;
    }
#undef EVAE_MIX_DZ
    rc = check_launch("mixture_query_kernel(bwd)");
    if (rc != EVAE_OK) return rc;
    if (p.nsplit > 1) {
      const size_t n = (size_t)B * zdim;
      mixture_dz_reduce_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(part, p.nsplit, n, dz);
      rc = check_launch("mixture_dz_reduce_kernel");
      if (rc != EVAE_OK) return rc;
    }
  }
  if (dmeans != nullptr || dlog_var != nullptr) {
    const int grid = cdiv(C, MC_WAVES);
#define EVAE_MIX_DC(N) \
  mixture_component_kernel<N><<<grid, MC_WAVES * 64, 0, stream>>>(z, B, means, log_var, C, zdim, lse, grad_out, dmeans, dlog_var)
    switch (p.nch) {
      case 1: EVAE_MIX_DC(1); break;
      case 2: EVAE_MIX_DC(2); break;
      case 4: EVAE_MIX_DC(4); break;
      default: EVAE_MIX_DC(8); break;
    }
#undef EVAE_MIX_DC
    rc = check_launch("mixture_component_kernel");
    if (rc != EVAE_OK) return rc;
  }
  return EVAE_OK;
}

extern "C" int evae_pseudo_inputs_fwd(const float* weight, int D, int C, float* out, evae_stream_t stream_) {
  EVAE_REQUIRE(D >= 1 && C >= 1, "pseudo_inputs_fwd: bad sizes D=%d C=%d", D, C);
  EVAE_REQUIRE(weight && out, "pseudo_inputs_fwd: null pointer");
  EVAE_REQUIRE(cdiv(D, PT) <= 65535, "pseudo_inputs_fwd: D=%d too large", D);
  const dim3 grid(cdiv(C, PT), cdiv(D, PT));
  pseudo_inputs_fwd_kernel<<<grid, 256, 0, (hipStream_t)stream_>>>(weight, D, C, out);
  return check_launch("pseudo_inputs_fwd_kernel");
}

extern "C" int evae_pseudo_inputs_bwd(const float* weight, const float* dout, int D, int C, float* dweight,
                                      evae_stream_t stream_) {
  EVAE_REQUIRE(D >= 1 && C >= 1, "pseudo_inputs_bwd: bad sizes D=%d C=%d", D, C);
  EVAE_REQUIRE(weight && dout && dweight, "pseudo_inputs_bwd: null pointer");
  EVAE_REQUIRE(cdiv(D, PT) <= 65535, "pseudo_inputs_bwd: D=%d too large", D);
  const dim3 grid(cdiv(C, PT), cdiv(D, PT));
  pseudo_inputs_bwd_kernel<<<grid, 256, 0, (hipStream_t)stream_>>>(weight, dout, D, C, dweight);
  return check_launch("pseudo_inputs_bwd_kernel");
}
