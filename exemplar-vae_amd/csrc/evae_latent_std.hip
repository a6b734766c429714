// The latent block of a standard-normal-prior step (--prior standard; reference models/BaseModel.py:111-122 log_p_z, utils/
// distributions.py:36-41 log_normal_standard) for the B batch rows: forward and backward in ONE launch each.
//
//   forward   z_mean = x wm^T + bm, lv_pre = x wl^T + bl, logvar = clamp(lv_pre), z = z_mean + eps exp(logvar / 2), log q(z | x)
//             -- thin_heads_kernel of evae_thin_heads.h, the same instructions in the same order -- and log p(z) = sum_d (-z^2 / 2 -
//             log(2 pi) / 2) from the sample while it is in registers;
//   backward  the reparameterisation, log q, the Hardtanh of the log-variance head and the prior's share of dz (-d log p / dz = z)
//             element-wise, then the heads' data gradient dA = dmu wm + dlv_pre wl with the gate derivative of the layer below in
//             its epilogue: evae_reparam_logq_bwd_hardtanh + evae_dense_bwd_data on the gate path, as one graph node.
//
// Both are latency-bound pieces over weight-sized traffic (2 x Z x K floats, L2-resident beside <= a few hundred rows): the block
// shapes are evae_thin.h's -- 256 threads, a 16-row tile, four waves splitting the contraction, partial tiles met in LDS in a fixed
// order -- so a step's result does not depend on the launch geometry.  No block waits for another one.
#include "evae_thin_heads.h"

namespace evae {

struct HeadsStdBwdArgs {
  const float* logvar; const float* lv_pre; const float* eps; const float* z; const float* dz;     // [M x Z], dense
  const float* cKL;                                                                                // [M]
  const float* wm; const float* wl;                                                                // [Z x K]
  const float* out_prev; const float* s_prev;                                                      // [M x K], dense
  float lo, hi;
  int M, Z, K;
  float* dmu; float* dlv_pre; int ldd;
  float* dh; float* dg; int ldo;
};

// grid (cdiv(K, 16), cdiv(M, 16)).  A block recomputes (dmu, dlv_pre) of its 16 rows from the Z-wide inputs into LDS (Z <= 64,
// zero-padded: 5 loads and one exp per element against 2 Z weight loads per output), the blocks of column tile 0 store them for the
// heads' weight gradients, and the product runs as in thin_layer_kernel<.., BWD>: lane (i, kq) holds row i of the operand and column
// n0 + i of the weights for the four contraction indices 16 c + 4 kq + j, bank by bank, wave w the chunks w, w + 4, ... -- that
// kernel's order of summation, so [dh | dg] has the bits of evae_dense_bwd_data fed with the stored (dmu, dlv_pre) where the thin
// kernel serves it.
__global__ __launch_bounds__(256) void heads_std_bwd_kernel(const HeadsStdBwdArgs t) {
  __shared__ float sd[2][64][20];        // [bank][contraction index][row]: lane (i, kq) reads word 80 kq + i (+ const): no conflicts
  __shared__ float part[4][16][17];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, kq = lane >> 4;
  const int n0 = blockIdx.x * 16, m0 = blockIdx.y * 16;
  for (int e = tid; e < 16 * 64; e += 256) {
    const int r = e >> 6, k = e & 63, m = m0 + r;
    float gmu = 0.f, glp = 0.f;
    if (m < t.M && k < t.Z) {
      const size_t o = (size_t)m * t.Z + k;
      const float ck = t.cKL[m];
      const float gz = t.dz[o] + ck * t.z[o];                                  // decoder's gradient + the prior's share
      const float dl = 0.5f * gz * expf(0.5f * t.logvar[o]) * t.eps[o] - 0.5f * ck;   // ((z - mu)^2 / var = eps^2: no gradient)
      const float pre = t.lv_pre[o];
      gmu = gz;
      glp = (pre > t.lo && pre < t.hi) ? dl : 0.f;
      if (blockIdx.x == 0) {
        const size_t od = (size_t)m * t.ldd + k;
        t.dmu[od] = gmu;
        t.dlv_pre[od] = glp;
      }
    }
    sd[0][k][r] = gmu;
    sd[1][k][r] = glp;
  }
  __syncthreads();
  thin_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const int kcol = (n0 + i < t.K) ? n0 + i : t.K - 1;
  const int nchunk = (t.Z + 15) >> 4;                      // <= 4: a wave has at most one chunk per bank
  for (int bank = 0; bank < 2; ++bank) {
    const float* W = bank ? t.wl : t.wm;
    for (int c = wave; c < nchunk; c += 4) {
      const int kb = c * 16 + 4 * kq;
      float w[4], a[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        w[j] = (kb + j < t.Z) ? W[(size_t)(kb + j) * t.K + kcol] : 0.f;
        a[j] = sd[bank][kb + j][i];
      }
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], w[0], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], w[1], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], w[2], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], w[3], acc, 0, 0, 0);
    }
  }
  // C layout of the 16 x 16 tile: register r <-> row 4 (lane >> 4) + r, column lane & 15
#pragma unroll
  for (int r = 0; r < 4; ++r) part[wave][4 * kq + r][i] = acc[r];
  __syncthreads();
  const int row = tid >> 4, col = tid & 15;
  const int m = m0 + row, n = n0 + col;
  if (m >= t.M || n >= t.K) return;
  const float v = ((part[0][row][col] + part[1][row][col]) + part[2][row][col]) + part[3][row][col];
  // dh = v s, dg = v (h s)(1 - s): the gate derivative of the layer below (thin_layer_kernel's THIN_GATE_BWD epilogue)
  const size_t oe = (size_t)m * t.K + n, o = (size_t)m * t.ldo + n;
  const float go = t.out_prev[oe], s = t.s_prev[oe];
  t.dh[o] = v * s;
  t.dg[o] = v * go * (1.0f - s);
}

// log N(x | 0, I) summed over a row: log_normal_diag_fwd_kernel with mean = logvar = 0 (the same terms, no zero tensors read)
__global__ __launch_bounds__(256) void log_normal_std_fwd_kernel(const float* __restrict__ x, int B, int zdim, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;
  float acc = 0.f;
  for (int k = lane; k < zdim; k += 64) {
    const float d = x[(size_t)row * zdim + k];
    acc += -0.5f * (kLog2Pi + d * d);
  }
  acc = wave_sum(acc);
  if (lane == 0) out[row] = acc;
}

__global__ __launch_bounds__(256) void log_normal_std_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dout, int B,
                                                                 int zdim, float* __restrict__ dx) {
  const size_t n = (size_t)B * zdim;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  dx[i] = -(dout[i / zdim] * x[i]);
}

// the sizes the two one-launch kernels take: few rows (a batch; the tiled kernels own thousands of rows), float4 rows of x, all
// Z columns of a row inside one block
static bool heads_std_ok(int M, int K, int Z, int ldx) {
  return M >= 1 && M <= 1024 && K >= 16 && K % 4 == 0 && ldx >= K && ldx % 4 == 0 && Z >= 1 && Z <= 64;
}

}  // namespace evae

using namespace evae;

extern "C" int evae_heads_std_applies(int M, int K, int Z, int ldx) { return heads_std_ok(M, K, Z, ldx) ? 1 : 0; }

extern "C" int evae_heads_reparam_std_fwd(const float* x, int M, int K, int ldx, const float* wm, const float* bm, const float* wl,
                                          const float* bl, int Z, float lv_lo, float lv_hi, const float* eps, float* z_mean,
                                          float* lv_pre, float* logvar, float* z, float* logq, float* logp, evae_stream_t stream_) {
  EVAE_REQUIRE(heads_std_ok(M, K, Z, ldx), "heads_reparam_std_fwd: not a size of the one-launch kernel (M=%d K=%d Z=%d ldx=%d); "
               "evae_heads_std_applies says so up front", M, K, Z, ldx);
  EVAE_REQUIRE(x && wm && wl && eps && z_mean && logvar && z && logp, "heads_reparam_std_fwd: null pointer");
  EVAE_REQUIRE((((uintptr_t)x | (uintptr_t)wm | (uintptr_t)wl) & 15) == 0, "heads_reparam_std_fwd: x, wm, wl must be 16-byte aligned");
  ThinHeadsArgs t = {x, ldx, M, K, Z, wm, bm, wl, bl, lv_lo, lv_hi, eps, nullptr, z_mean, lv_pre, logvar, z, logq, nullptr, nullptr, 0};
  t.logp = logp;
  return launch_thin_heads<true>(t, (hipStream_t)stream_, "heads_reparam_std_fwd");
}

extern "C" int evae_heads_std_bwd(const float* z_mean, const float* logvar, const float* lv_pre, const float* eps, const float* z,
                                  const float* dz, const float* cKL, const float* neg_cKL, float lv_lo, float lv_hi, int M, int Z,
                                  const float* wm, const float* wl, int K, const float* out_prev, const float* s_prev, float* dmu,
                                  float* dlv_pre, int ldd, float* dh, float* dg, int ldo, evae_stream_t stream_) {
  (void)z_mean; (void)neg_cKL;         // (z - z_mean = eps exp(logvar / 2), and neg_cKL = -cKL: carried for the callers' symmetry)
  EVAE_REQUIRE(M >= 1 && M <= 1024 && Z >= 1 && Z <= 64 && K >= 1 && ldd >= Z && ldo >= K,
               "heads_std_bwd: bad sizes M=%d Z=%d K=%d ldd=%d ldo=%d (1 <= M <= 1024, Z <= 64)", M, Z, K, ldd, ldo);
  EVAE_REQUIRE(logvar && lv_pre && eps && z && dz && cKL && wm && wl && out_prev && s_prev && dmu && dlv_pre && dh && dg,
               "heads_std_bwd: null pointer");
  const HeadsStdBwdArgs t = {logvar, lv_pre, eps, z, dz, cKL, wm, wl, out_prev, s_prev, lv_lo, lv_hi, M, Z, K, dmu, dlv_pre, ldd,
                             dh, dg, ldo};
  heads_std_bwd_kernel<<<dim3(cdiv(K, 16), cdiv(M, 16)), 256, 0, (hipStream_t)stream_>>>(t);
  return check_launch("heads_std_bwd");
}

extern "C" int evae_log_normal_std_fwd(const float* x, int B, int zdim, float* out, evae_stream_t stream_) {
  EVAE_REQUIRE(B >= 0 && zdim > 0, "log_normal_std_fwd: bad sizes");
  if (B == 0) return EVAE_OK;
  EVAE_REQUIRE(x && out, "log_normal_std_fwd: null pointer");
  log_normal_std_fwd_kernel<<<cdiv(B, 4), 256, 0, (hipStream_t)stream_>>>(x, B, zdim, out);
  return check_launch("log_normal_std_fwd");
}

extern "C" int evae_log_normal_std_bwd(const float* x, const float* dout, int B, int zdim, float* dx, evae_stream_t stream_) {
  EVAE_REQUIRE(B >= 0 && zdim > 0 && (long long)B * zdim <= 0x7fffffffll * 256, "log_normal_std_bwd: bad sizes");
  if (B == 0) return EVAE_OK;
  EVAE_REQUIRE(x && dout && dx, "log_normal_std_bwd: null pointer");
  const size_t n = (size_t)B * zdim;
  log_normal_std_bwd_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream_>>>(x, dout, B, zdim, dx);
  return check_launch("log_normal_std_bwd");
}
