// The layered path (layered_path.h): actor-critic MLP forward/backward on gfx950 MFMA + the PPO
// loss heads + split-K gradient reduction, one launch per layer and direction.
//
// Every dense fc-layer product is one MFMA GEMM template (v_mfma_f32_32x32x2_f32: exact f32
// inputs, f32 accumulate -- the reference computes in f32, so parity keeps f32 operands):
//   forward   Y  = act(X W^T + b)          A = X  [rows][in]  (optionally gathered by row index)
//   input grad dX = (dY W) * act'(X)        A = dY [rows][out], B = W [out][in]
//   weight grad dW = dY^T X  (split-K over the minibatch rows, per-split slabs, + bias colsums)
// Operands are staged global -> registers -> LDS ([k][m] / [k][n], row stride +2 words: the
// transposing store is conflict-free for 32-lane write groups, the MFMA fragment reads are
// consecutive), double-buffered with one barrier per k-tile.  Actor and critic layers of equal
// shape run in one launch (blockIdx.z = net).
//
// Heads (output widths A and 1) are wave-per-row VALU kernels: tanh/mean, sampling, log-prob,
// clipped surrogate, Huber, and the head backward, with torch's formulas (SURVEY.md s8(a) A3-A4,
// A11-A13).  Reductions are in a fixed order (split slabs summed 0..S-1), so results are
// bit-reproducible run to run.
#include <algorithm>

#include "common.h"
#include "ctx.h"
#include "gemm_ops.h"
#include "layered_path.h"
#include "ppo_loss.h"
#include "reduce_slabs.h"
#include "timing.h"

namespace ppo {

// ============================================================================================
// Heads
// ============================================================================================
struct PolicyHeadArgs {
  const float *ha;   // actor last hidden (n, da) or null
  const float *hc;   // critic last hidden (n, dc) or null
  int da, dc, n, act_dim;
  const float *wa, *ba, *logstd;  // actor head (A, da), (A) or null, (A)
  const float *wc, *bc;           // critic head (1, dc), (1)
  float omv;
  const float *eps;               // (n, A) or null -> Philox(seed, offset + row*A + a)
  uint64_t seed, offset;
  const uint64_t *offset_base;    // device counter added to offset (ppo_ctx_set_rng_counter)
  float *action, *logp, *value, *mean;
  int bf16;                       // precision bf16: head operands rounded to bf16 (f32 accumulate)
};

// One wave per env row.  Sampling and log-prob: ppo_loss.h, summed a = 0..A-1.
template <int HPL>
__global__ __launch_bounds__(256) void policy_head_kernel(PolicyHeadArgs q) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= q.n) return;
  if (q.ha) {
    float h[HPL];
    const float *hr = q.ha + static_cast<int64_t>(row) * q.da;
#pragma unroll
    for (int j = 0; j < HPL; ++j) {
      const int k = lane + 64 * j;
      h[j] = (k < q.da) ? (q.bf16 ? bf16_round(hr[k]) : hr[k]) : 0.f;
    }
    float my_z = 0.f;
    for (int a = 0; a < q.act_dim; ++a) {
      const float *w = q.wa + static_cast<int64_t>(a) * q.da;
      float part = 0.f;
#pragma unroll
      for (int j = 0; j < HPL; ++j) {
        const int k = lane + 64 * j;
        if (k < q.da) part = fmaf(h[j], q.bf16 ? bf16_round(w[k]) : w[k], part);
      }
      const float z = wave_sum(part);
      if (lane == a) my_z = z;
    }
    float lp = 0.f;
    if (lane < q.act_dim) {
      const int a = lane;
      const float z = q.ba ? my_z + q.ba[a] : my_z;
      const float mu = q.omv * tanhf(z);
      const float sd = expf(q.logstd[a]);
      const int64_t idx = static_cast<int64_t>(row) * q.act_dim + a;
      const float e =
          q.eps ? q.eps[idx]
                : philox_normal_at(q.seed, q.offset + (q.offset_base ? *q.offset_base : 0) + idx);
      const float x = normal_sample(e, sd, mu);
      if (q.action) q.action[idx] = x;
      if (q.mean) q.mean[idx] = mu;
      lp = normal_logp_term(x - mu, sd * sd, logf(sd));
    }
    if (q.logp) {
      float s = 0.f;
      for (int a = 0; a < q.act_dim; ++a) s += __shfl(lp, a, 64);
      if (lane == 0) q.logp[row] = s;
    }
  }
  if (q.hc && q.value) {
    const float *hr = q.hc + static_cast<int64_t>(row) * q.dc;
    float part = 0.f;
#pragma unroll
    for (int j = 0; j < HPL; ++j) {
      const int k = lane + 64 * j;
      if (k < q.dc)
        part = q.bf16 ? fmaf(bf16_round(hr[k]), bf16_round(q.wc[k]), part) : fmaf(hr[k], q.wc[k], part);
    }
    const float v = wave_sum(part);
    if (lane == 0) q.value[row] = q.bc ? v + q.bc[0] : v;
  }
}

struct UpdateHeadArgs {
  const float *ha, *hc;          // last hidden (rows, da) / (rows, dc), minibatch order
  float *ga, *gc;                // OUT: dH_L (rows, da) / (rows, dc)
  float *dza, *dzc;              // OUT: d(head pre-activation) (rows, A) / (rows, 1)
  int da, dc, act_dim, act;
  const float *wa, *ba, *logstd, *wc, *bc;
  float omv;
  const int32_t *rows;           // storage row of minibatch row j
  int rows_max;
  const int32_t *rows_n;         // device count (nullable)
  const float *actions, *old_logp, *adv, *vtarget;  // storage arrays
  LossCoef coef;
  float *logstd_part;            // (splits, A)
  float *loss_part;              // (splits, 2): sum over rows of actor / critic loss terms
  int splits;
  // fused head weight gradient (update_head_q4_kernel<NJ, true>): per split, at hw_part +
  // split * hw_stride: actor W (A, da) | actor b (A) at off_ba | critic W (dc) at off_wc |
  // critic b at off_bc
  float *hw_part;
  int hw_stride, off_ba, off_wc, off_bc;
  int bf16;                      // precision bf16: every head product on bf16-rounded operands
};

// operand rounding of precision mode bf16 (identity in f32 mode)
__device__ __forceinline__ float rb(float x, int bf16) { return bf16 ? bf16_round(x) : x; }
__device__ __forceinline__ float4 rb4(float4 v, int bf16) {
  return bf16 ? make_float4(bf16_round(v.x), bf16_round(v.y), bf16_round(v.z), bf16_round(v.w)) : v;
}

// Fast head: 4 lanes per row, 16 rows per wave pass, D = 16*NJ columns (actor and critic last
// hidden widths equal).  Lane (row r = lane>>2, quarter qd = lane&3) holds float4 chunks
// 16t + 4qd of its row; a head dot product is NJ float4 FMAs against LDS-staged head weights
// (same address for the 16 rows -> LDS broadcast) plus a 2-step shuffle over the row's 4 lanes.
// Per-action work (tanh, log-prob, dz) is spread over the 4 lanes: lane qd owns actions
// a = 4k + qd.  The formulas are ppo_loss.h's.
// FW (A <= kFusedHeadAct): also accumulate the head layer's weight gradient, dW = dz^T H_L and
// db = sum dz per net, over the block's rows while H_L is hot in L1/L2 -- lane owns float4
// column chunk c = lane + 64u of both nets -- so the split-K head GEMM (a second full read of
// H_L) is not launched.  Waves combine in a fixed order; one partial per block.
constexpr int kFusedHeadAct = 8;
template <int NJ, bool FW>
// two workgroups per CU where the registers allow it (NJ <= 16: 512 blocks then run in one round)
__global__ __launch_bounds__(256, NJ <= 16 ? 2 : 1) void update_head_q4_kernel(UpdateHeadArgs q) {
  constexpr int D = 16 * NJ;
  // action groups of 4 per lane: the fused-wgrad instantiation runs only for A <= kFusedHeadAct,
  // so it sizes its per-action registers for that (kMaxAct / 4 groups cost it 30 VGPRs)
  constexpr int KA = FW ? kFusedHeadAct / 4 : kMaxAct / 4;
  constexpr int CH = (4 * NJ + 63) / 64;  // float4 column chunks per lane (fused wgrad)
  constexpr int AF = FW ? kFusedHeadAct : 1;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ float red[4][kMaxAct + 2];
  __shared__ float dvs[4][16];
  const int A = q.act_dim;
  float *wsh = smem;                   // (A + 1) x D: actor head rows, then the critic row
  float *lps = smem + (A + 1) * D;     // [4 waves][16 rows][kMaxAct] log-probs
  float *dzs = lps + 4 * 16 * kMaxAct;  // [4 waves][16 rows][kMaxAct] d(pre-tanh)
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int r = lane >> 2, qd = lane & 3;
  for (int i = tid; i < A * D; i += 256) wsh[i] = rb(q.wa[i], q.bf16);
  for (int i = tid; i < D; i += 256) wsh[A * D + i] = rb(q.wc[i], q.bf16);
  __syncthreads();
  const int count = q.rows_n ? *q.rows_n : q.rows_max;
  const int r0 = static_cast<int>((static_cast<int64_t>(blockIdx.x) * count) / q.splits);
  const int r1 = static_cast<int>((static_cast<int64_t>(blockIdx.x + 1) * count) / q.splits);
  float *lp_row = lps + (wid * 16 + r) * kMaxAct;
  float *dz_row = dzs + (wid * 16 + r) * kMaxAct;
  float ls_acc[KA];
#pragma unroll
  for (int k = 0; k < KA; ++k) ls_acc[k] = 0.f;
  float la_acc = 0.f, lc_acc = 0.f;
  float4 wa_acc[CH][AF], wc_acc[CH];
  float b_acc = 0.f;  // lane a < A: actor bias a; lane A: critic bias
#pragma unroll
  for (int u = 0; u < CH; ++u) {
    wc_acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int a = 0; a < AF; ++a) wa_acc[u][a] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  for (int base = r0 + 16 * wid; base < r1; base += 64) {  // wave-uniform trip count
    const int j = base + r;
    const bool valid = j < r1;
    const int64_t sr = valid ? q.rows[j] : 0;
    float4 h[NJ];
    const float4 *hrow = reinterpret_cast<const float4 *>(q.ha + static_cast<int64_t>(j) * D);
#pragma unroll
    for (int t = 0; t < NJ; ++t) h[t] = valid ? hrow[4 * t + qd] : make_float4(0, 0, 0, 0);
    // ---- actor head: z_a for the lane's own actions a = 4k + qd
    float zk[KA];
#pragma unroll
    for (int k = 0; k < KA; ++k) {
      zk[k] = 0.f;
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) {
        const int a = 4 * k + qq;
        if (a < A) {
          const float4 *w = reinterpret_cast<const float4 *>(wsh + a * D);
          float p = 0.f;
#pragma unroll
          for (int t = 0; t < NJ; ++t) {
            const float4 wv = w[4 * t + qd];
            const float4 hb = rb4(h[t], q.bf16);
            p = fmaf(hb.x, wv.x, p);
            p = fmaf(hb.y, wv.y, p);
            p = fmaf(hb.z, wv.z, p);
            p = fmaf(hb.w, wv.w, p);
          }
          p += __shfl_xor(p, 1, 64);
          p += __shfl_xor(p, 2, 64);
          if (qq == qd) zk[k] = p;
        }
      }
    }
    float yk[KA], dk[KA], vk[KA];
#pragma unroll
    for (int k = 0; k < KA; ++k) {
      const int a = 4 * k + qd;
      yk[k] = 0.f, dk[k] = 0.f, vk[k] = 1.f;
      if (a < A) {
        const float z = q.ba ? zk[k] + q.ba[a] : zk[k];
        const float y = tanhf(z);
        const float mu = q.omv * y;
        const float sd = expf(q.logstd[a]);
        const float x = valid ? q.actions[sr * A + a] : mu;
        const float d = x - mu;
        const float var = sd * sd;
        lp_row[a] = normal_logp_term(d, var, logf(sd));
        yk[k] = y, dk[k] = d, vk[k] = var;
      }
    }
    __threadfence_block();
    float logp = 0.f;
    for (int a = 0; a < A; ++a) logp += lp_row[a];
    const float old_lp = valid ? q.old_logp[sr] : logp;
    const float adv = valid ? q.adv[sr] : 0.f;
    const Surrogate sg = clipped_surrogate(logp, old_lp, adv, q.coef);
    const float dlogp = valid ? sg.dlogp : 0.f;
    if (valid && qd == 0) la_acc += sg.mn;
#pragma unroll
    for (int k = 0; k < KA; ++k) {
      const int a = 4 * k + qd;
      if (a < A) {
        const float dz = tanh_mean_grad(dlogp, dk[k], vk[k], q.omv, yk[k]);
        dz_row[a] = dz;
        if (valid) {
          ls_acc[k] += logstd_grad(dlogp, dk[k], vk[k], q.coef);
          q.dza[static_cast<int64_t>(j) * A + a] = dz;
        }
      }
    }
    __threadfence_block();
    // ---- dH_L(actor) = (dz . W_head) * act'(h)
    float4 *grow = reinterpret_cast<float4 *>(q.ga + static_cast<int64_t>(j) * D);
#pragma unroll
    for (int t = 0; t < NJ; ++t) {
      float4 s = make_float4(0, 0, 0, 0);
      for (int a = 0; a < A; ++a) {
        const float dz = rb(dz_row[a], q.bf16);
        const float4 wv = reinterpret_cast<const float4 *>(wsh + a * D)[4 * t + qd];
        s.x = fmaf(dz, wv.x, s.x);
        s.y = fmaf(dz, wv.y, s.y);
        s.z = fmaf(dz, wv.z, s.z);
        s.w = fmaf(dz, wv.w, s.w);
      }
      if (valid)
        grow[4 * t + qd] = make_float4(act_backward(s.x, h[t].x, q.act), act_backward(s.y, h[t].y, q.act),
                                       act_backward(s.z, h[t].z, q.act), act_backward(s.w, h[t].w, q.act));
    }
    // ---- critic
    const float4 *crow = reinterpret_cast<const float4 *>(q.hc + static_cast<int64_t>(j) * D);
#pragma unroll
    for (int t = 0; t < NJ; ++t) h[t] = valid ? crow[4 * t + qd] : make_float4(0, 0, 0, 0);
    const float4 *wc = reinterpret_cast<const float4 *>(wsh + A * D);
    float p = 0.f;
#pragma unroll
    for (int t = 0; t < NJ; ++t) {
      const float4 wv = wc[4 * t + qd];
      const float4 hb = rb4(h[t], q.bf16);
      p = fmaf(hb.x, wv.x, p);
      p = fmaf(hb.y, wv.y, p);
      p = fmaf(hb.z, wv.z, p);
      p = fmaf(hb.w, wv.w, p);
    }
    p += __shfl_xor(p, 1, 64);
    p += __shfl_xor(p, 2, 64);
    const float v = q.bc ? p + q.bc[0] : p;
    const float vt = valid ? q.vtarget[sr] : v;
    const float diff = v - vt;
    if (valid && qd == 0) lc_acc += huber(diff);
    const float dv = huber_grad(diff, q.coef.inv_b);
    if (valid && qd == 0) q.dzc[j] = dv;
    float4 *gcrow = reinterpret_cast<float4 *>(q.gc + static_cast<int64_t>(j) * D);
    const float dvb = rb(dv, q.bf16);
#pragma unroll
    for (int t = 0; t < NJ; ++t) {
      const float4 wv = wc[4 * t + qd];
      if (valid)
        gcrow[4 * t + qd] =
            make_float4(act_backward(dvb * wv.x, h[t].x, q.act), act_backward(dvb * wv.y, h[t].y, q.act),
                        act_backward(dvb * wv.z, h[t].z, q.act), act_backward(dvb * wv.w, h[t].w, q.act));
    }
    if constexpr (FW) {
      // head dW += dz^T H over this pass's 16 rows (dz rows of invalid j are exactly 0 and are
      // skipped anyway); H re-read by columns from L1/L2
      if (qd == 0) dvs[wid][r] = valid ? dv : 0.f;
      __threadfence_block();
      const int nrow = min(16, r1 - base);
      for (int rr = 0; rr < nrow; ++rr) {
        const int64_t jj = base + rr;
        const float *dzr = dzs + (wid * 16 + rr) * kMaxAct;
        const float dvr = dvs[wid][rr];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
          const int c = lane + 64 * u;
          if (c < 4 * NJ) {
            const float4 ha4 = rb4(reinterpret_cast<const float4 *>(q.ha + jj * D)[c], q.bf16);
            const float4 hc4 = rb4(reinterpret_cast<const float4 *>(q.hc + jj * D)[c], q.bf16);
#pragma unroll
            for (int a = 0; a < AF; ++a) {
              if (a < A) {
                const float dz = rb(dzr[a], q.bf16);
                wa_acc[u][a].x = fmaf(dz, ha4.x, wa_acc[u][a].x);
                wa_acc[u][a].y = fmaf(dz, ha4.y, wa_acc[u][a].y);
                wa_acc[u][a].z = fmaf(dz, ha4.z, wa_acc[u][a].z);
                wa_acc[u][a].w = fmaf(dz, ha4.w, wa_acc[u][a].w);
              }
            }
            const float dvrb = rb(dvr, q.bf16);
            wc_acc[u].x = fmaf(dvrb, hc4.x, wc_acc[u].x);
            wc_acc[u].y = fmaf(dvrb, hc4.y, wc_acc[u].y);
            wc_acc[u].z = fmaf(dvrb, hc4.z, wc_acc[u].z);
            wc_acc[u].w = fmaf(dvrb, hc4.w, wc_acc[u].w);
          }
        }
        if (lane < A) b_acc += dzr[lane];
        else if (lane == A) b_acc += dvr;
      }
    }
  }
  if constexpr (FW) {
    // combine the 4 waves' partials in wave order through LDS (the staged head weights and the
    // log-prob scratch are dead now), then one coalesced partial per block
    __syncthreads();
    float *acc_sh = wsh;   // (A + 1) x D
    float *bias_sh = lps;  // A + 1
    for (int w = 0; w < 4; ++w) {
      if (wid == w) {
#pragma unroll
        for (int u = 0; u < CH; ++u) {
          const int c = lane + 64 * u;
          if (c < 4 * NJ) {
#pragma unroll
            for (int a = 0; a <= AF; ++a) {
              if (a <= A) {
                const float4 v = (a == A || a == AF) ? wc_acc[u] : wa_acc[u][a < AF ? a : 0];
                float4 *dst = reinterpret_cast<float4 *>(acc_sh + a * D) + c;
                if (w == 0) {
                  *dst = v;
                } else {
                  const float4 o = *dst;
                  *dst = make_float4(o.x + v.x, o.y + v.y, o.z + v.z, o.w + v.w);
                }
              }
            }
          }
        }
        if (lane <= A) bias_sh[lane] = (w == 0) ? b_acc : bias_sh[lane] + b_acc;
      }
      __syncthreads();
    }
    float *dst = q.hw_part + static_cast<int64_t>(blockIdx.x) * q.hw_stride;
    for (int i = tid; i < A * D / 4; i += 256)
      reinterpret_cast<float4 *>(dst)[i] = reinterpret_cast<const float4 *>(acc_sh)[i];
    for (int i = tid; i < D / 4; i += 256)
      reinterpret_cast<float4 *>(dst + q.off_wc)[i] =
          reinterpret_cast<const float4 *>(acc_sh + A * D)[i];
    if (tid < A && q.ba) dst[q.off_ba + tid] = bias_sh[tid];
    if (tid == 0) dst[q.off_bc] = bias_sh[A];
  }
  // ---- fixed-order reductions: over the 16 rows of the wave (lane bits 2..5), then waves 0..3
#pragma unroll
  for (int k = 0; k < KA; ++k)
#pragma unroll
    for (int off = 4; off < 64; off <<= 1) ls_acc[k] += __shfl_xor(ls_acc[k], off, 64);
#pragma unroll
  for (int off = 4; off < 64; off <<= 1) {
    la_acc += __shfl_xor(la_acc, off, 64);
    lc_acc += __shfl_xor(lc_acc, off, 64);
  }
  if (r == 0) {
#pragma unroll
    for (int k = 0; k < KA; ++k)
      if (4 * k + qd < A) red[wid][4 * k + qd] = ls_acc[k];
    if (qd == 0) {
      red[wid][kMaxAct] = la_acc;
      red[wid][kMaxAct + 1] = lc_acc;
    }
  }
  __syncthreads();
  if (tid < A)
    q.logstd_part[static_cast<int64_t>(blockIdx.x) * A + tid] =
        ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
  if (tid == 0) {
    q.loss_part[2 * blockIdx.x] = ((red[0][kMaxAct] + red[1][kMaxAct]) + red[2][kMaxAct]) +
                                  red[3][kMaxAct];
    q.loss_part[2 * blockIdx.x + 1] =
        ((red[0][kMaxAct + 1] + red[1][kMaxAct + 1]) + red[2][kMaxAct + 1]) + red[3][kMaxAct + 1];
  }
}

// Generic head (any widths): one wave per row.  The formulas are ppo_loss.h's.
template <int HPL>
__global__ __launch_bounds__(256) void update_head_kernel(UpdateHeadArgs q) {
  __shared__ float red[4][kMaxAct + 2];
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int count = q.rows_n ? *q.rows_n : q.rows_max;
  const int r0 = static_cast<int>((static_cast<int64_t>(blockIdx.x) * count) / q.splits);
  const int r1 = static_cast<int>((static_cast<int64_t>(blockIdx.x + 1) * count) / q.splits);
  const int A = q.act_dim;
  float lsacc = 0.f;                 // lane a: d loss / d logstd_a over this wave's rows
  float la_acc = 0.f, lc_acc = 0.f;  // lane 0: loss sums
  for (int j = r0 + wid; j < r1; j += 4) {
    const int64_t sr = q.rows[j];
    // ---------------- actor ----------------
    float h[HPL];
    const float *hr = q.ha + static_cast<int64_t>(j) * q.da;
#pragma unroll
    for (int t = 0; t < HPL; ++t) {
      const int k = lane + 64 * t;
      h[t] = (k < q.da) ? hr[k] : 0.f;
    }
    float my_z = 0.f;
    for (int a = 0; a < A; ++a) {
      const float *w = q.wa + static_cast<int64_t>(a) * q.da;
      float part = 0.f;
#pragma unroll
      for (int t = 0; t < HPL; ++t) {
        const int k = lane + 64 * t;
        if (k < q.da) part = fmaf(rb(h[t], q.bf16), rb(w[k], q.bf16), part);
      }
      const float z = wave_sum(part);
      if (lane == a) my_z = z;
    }
    float lp = 0.f, y = 0.f, d = 0.f, var = 1.f;
    if (lane < A) {
      const float z = q.ba ? my_z + q.ba[lane] : my_z;
      y = tanhf(z);
      const float mu = q.omv * y;
      const float sd = expf(q.logstd[lane]);
      const float x = q.actions[sr * A + lane];
      d = x - mu;
      var = sd * sd;
      lp = normal_logp_term(d, var, logf(sd));
    }
    float logp = 0.f;
    for (int a = 0; a < A; ++a) logp += __shfl(lp, a, 64);
    const Surrogate sg = clipped_surrogate(logp, q.old_logp[sr], q.adv[sr], q.coef);
    float dz = 0.f;
    if (lane < A) {
      dz = tanh_mean_grad(sg.dlogp, d, var, q.omv, y);
      lsacc += logstd_grad(sg.dlogp, d, var, q.coef);
      q.dza[static_cast<int64_t>(j) * A + lane] = dz;
    }
    if (lane == 0) la_acc += sg.mn;
    // dH_L(actor) = (dz . W_head) * act'(h)
    float *gr = q.ga + static_cast<int64_t>(j) * q.da;
#pragma unroll
    for (int t = 0; t < HPL; ++t) {
      const int k = lane + 64 * t;
      if (k < q.da) {
        float s = 0.f;
        for (int a = 0; a < A; ++a)
          s = fmaf(rb(__shfl(dz, a, 64), q.bf16), rb(q.wa[static_cast<int64_t>(a) * q.da + k], q.bf16), s);
        gr[k] = act_backward(s, h[t], q.act);
      }
    }
    // ---------------- critic ----------------
    const float *cr = q.hc + static_cast<int64_t>(j) * q.dc;
#pragma unroll
    for (int t = 0; t < HPL; ++t) {
      const int k = lane + 64 * t;
      h[t] = (k < q.dc) ? cr[k] : 0.f;
    }
    float part = 0.f;
#pragma unroll
    for (int t = 0; t < HPL; ++t) {
      const int k = lane + 64 * t;
      if (k < q.dc) part = fmaf(rb(h[t], q.bf16), rb(q.wc[k], q.bf16), part);
    }
    float v = wave_sum(part);
    if (q.bc) v = v + q.bc[0];
    const float diff = v - q.vtarget[sr];
    if (lane == 0) lc_acc += huber(diff);
    const float dv = huber_grad(diff, q.coef.inv_b);
    if (lane == 0) q.dzc[j] = dv;
    float *gc = q.gc + static_cast<int64_t>(j) * q.dc;
#pragma unroll
    for (int t = 0; t < HPL; ++t) {
      const int k = lane + 64 * t;
      if (k < q.dc) gc[k] = act_backward(rb(dv, q.bf16) * rb(q.wc[k], q.bf16), h[t], q.act);
    }
  }
  // fixed-order block reduction: waves 0..3
  if (lane < A) red[wid][lane] = lsacc;
  if (lane == 0) {
    red[wid][kMaxAct] = la_acc;
    red[wid][kMaxAct + 1] = lc_acc;
  }
  __syncthreads();
  if (threadIdx.x < A) {
    const float s = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) +
                    red[3][threadIdx.x];
    q.logstd_part[static_cast<int64_t>(blockIdx.x) * A + threadIdx.x] = s;
  }
  if (threadIdx.x == 0) {
    q.loss_part[2 * blockIdx.x] = ((red[0][kMaxAct] + red[1][kMaxAct]) + red[2][kMaxAct]) +
                                  red[3][kMaxAct];
    q.loss_part[2 * blockIdx.x + 1] =
        ((red[0][kMaxAct + 1] + red[1][kMaxAct + 1]) + red[2][kMaxAct + 1]) + red[3][kMaxAct + 1];
  }
}

// ============================================================================================
// Minibatch state gather: xg[j][0:din] = states[rows[j]][:], zero padded to ldx (16-B rows), so
// both layer-1 GEMMs (forward and weight-gradient) stream one contiguous, vector-loadable buffer
// instead of re-gathering 68-B rows element by element.
// ============================================================================================
__global__ void gather_states_kernel(const float *__restrict__ states, const int32_t *__restrict__ rows,
                                     const int32_t *__restrict__ rows_n, int b, int din, int ldx,
                                     float *__restrict__ xg) {
  const int count = rows_n ? *rows_n : b;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= static_cast<int64_t>(count) * ldx) return;
  const int j = static_cast<int>(i / ldx), c = static_cast<int>(i % ldx);
  xg[i] = (c < din) ? states[static_cast<int64_t>(rows[j]) * din + c] : 0.f;
}

// head kernels' HPL: hidden columns per lane (64 lanes per row)
static int hpl_for(int width) {
  if (width <= 256) return 4;
  if (width <= 512) return 8;
  return 16;
}

// layered_path.h
int forward_hidden(ppo_ctx *ctx, const bool use[2], const float *x, const int32_t *x_rows, int rows,
                   const int32_t *rows_n, hipStream_t st, int ldx) {
  const int max_l = std::max(use[0] ? ctx->net[0].n_hidden : 0, use[1] ? ctx->net[1].n_hidden : 0);
  for (int l = 0; l < max_l; ++l) {
    GemmBatch gb{};
    gb.prec = ctx->prec;
    gb.k = 0;
    gb.rows_n = rows_n;
    gb.act = ctx->cfg.activation;
    int np = 0, max_n = 0;
    int kdim = -1;
    for (int z = 0; z < 2; ++z) {
      const NetDesc &nd = ctx->net[z];
      if (!use[z] || l >= nd.n_hidden) continue;
      const LayerDesc &L = nd.layer[l];
      if (kdim >= 0 && kdim != L.in) {  // shapes differ: flush what we have
        int rc = gemm_rows_fwd_nk(gb, np, rows, max_n, st);
        if (rc) return rc;
        np = 0;
        max_n = 0;
      }
      kdim = L.in;
      GemmProblem &P = gb.p[np++];
      P.a = (l == 0) ? x : nd.h[l - 1];
      P.lda = (l == 0) ? ldx : nd.layer[l - 1].out;
      P.b = ctx->params + L.w_off;
      P.ldb = L.in;
      P.c = nd.h[l];
      P.ldc = L.out;
      P.bias = L.b_off >= 0 ? ctx->params + L.b_off : nullptr;
      P.m = rows;
      P.n = L.out;
      gb.k = L.in;
      max_n = std::max(max_n, L.out);
    }
    if (np) {
      int rc = gemm_rows_fwd_nk(gb, np, rows, max_n, st);
      if (rc) return rc;
    }
  }
  return 0;
}

int layered_policy_step(ppo_ctx *ctx, const float *state_d, int n, const float *eps_d,
                        uint64_t seed, uint64_t offset, float *action_d, float *logp_d,
                        float *value_d, float *mean_d, hipStream_t st) {
  const bool use[2] = {action_d || logp_d || mean_d, value_d != nullptr};
  if (!use[0] && !use[1]) return 0;
  if (int rc = forward_hidden(ctx, use, state_d, nullptr, n, nullptr, st,
                              ctx->cfg.obs_dim * ctx->cfg.window))
    return rc;
  const NetDesc &A = ctx->net[0], &C = ctx->net[1];
  PolicyHeadArgs q{};
  q.n = n;
  q.act_dim = ctx->cfg.act_dim;
  q.omv = ctx->cfg.output_max_value;
  if (use[0]) {
    const LayerDesc &hl = A.layer[A.n_hidden];
    q.ha = A.h[A.n_hidden - 1];
    q.da = hl.in;
    q.wa = ctx->params + hl.w_off;
    q.ba = hl.b_off >= 0 ? ctx->params + hl.b_off : nullptr;
    q.logstd = ctx->params + A.logstd_off;
  }
  if (use[1]) {
    const LayerDesc &hl = C.layer[C.n_hidden];
    q.hc = C.h[C.n_hidden - 1];
    q.dc = hl.in;
    q.wc = ctx->params + hl.w_off;
    q.bc = ctx->params + hl.b_off;
  }
  q.eps = eps_d;
  q.seed = seed;
  q.offset = offset;
  q.offset_base = ctx->rng_counter;
  q.action = action_d;
  q.logp = logp_d;
  q.value = value_d;
  q.mean = mean_d;
  q.bf16 = ctx->prec == PPO_PREC_BF16;
  const int hpl = hpl_for(std::max(q.da, q.dc));
  const int grid = ceil_div(n, 4);
  const int na = q.act_dim;
  const TimRec rec{KC_POLICY_HEAD,
                   tim_active() ? intern_name("policy_head_kernel<%d>", hpl) : nullptr,
                   2.0 * n * (static_cast<double>(q.da) * na + q.dc),
                   4.0 * n * (q.da + q.dc + (eps_d ? na : 0) + (action_d ? na : 0) +
                              (mean_d ? na : 0) + (logp_d ? 1 : 0) + (value_d ? 1 : 0))};
  if (hpl == 4) launch_k(rec, policy_head_kernel<4>, dim3(grid), dim3(256), 0, st, q);
  else if (hpl == 8) launch_k(rec, policy_head_kernel<8>, dim3(grid), dim3(256), 0, st, q);
  else launch_k(rec, policy_head_kernel<16>, dim3(grid), dim3(256), 0, st, q);
  PPO_LAUNCHED();
  return 0;
}

int layered_minibatch_grad(ppo_ctx *ctx, const float *states_d, const float *actions_d,
                           const float *old_logp_d, const float *adv_d, const float *vtarget_d,
                           const int32_t *rows_d, int b, const int32_t *count_d,
                           const LossCoef &coef, float *grad_d, float *loss_d, hipStream_t st) {
  const bool both[2] = {true, true};
  const int din = ctx->cfg.obs_dim * ctx->cfg.window;
  const int A = ctx->cfg.act_dim;
  launch_k(TimRec{KC_GATHER, "gather_states_kernel", 0.0, 4.0 * b * (2.0 * din + 1)},
           gather_states_kernel, dim3(ceil_div(static_cast<int64_t>(b) * ctx->ldx, 256)),
           dim3(256), 0, st, states_d, rows_d, count_d, b, din, ctx->ldx, ctx->xg);
  PPO_LAUNCHED();
  if (int rc = forward_hidden(ctx, both, ctx->xg, nullptr, b, count_d, st, ctx->ldx)) return rc;

  // ---- heads: loss, dz, dH_L -------------------------------------------------------------
  NetDesc &NA = ctx->net[0], &NC = ctx->net[1];
  const LayerDesc &HA = NA.layer[NA.n_hidden], &HC = NC.layer[NC.n_hidden];
  int head_splits = std::min(kHeadSplits, std::max(1, b / 32));
  UpdateHeadArgs u{};
  u.ha = NA.h[NA.n_hidden - 1];
  u.hc = NC.h[NC.n_hidden - 1];
  u.ga = NA.g;
  u.gc = NC.g;
  u.dza = NA.dz;
  u.dzc = NC.dz;
  u.da = HA.in;
  u.dc = HC.in;
  u.act_dim = A;
  u.act = ctx->cfg.activation;
  u.wa = ctx->params + HA.w_off;
  u.ba = HA.b_off >= 0 ? ctx->params + HA.b_off : nullptr;
  u.logstd = ctx->params + NA.logstd_off;
  u.wc = ctx->params + HC.w_off;
  u.bc = ctx->params + HC.b_off;
  u.omv = ctx->cfg.output_max_value;
  u.rows = rows_d;
  u.rows_max = b;
  u.rows_n = count_d;
  u.actions = actions_d;
  u.old_logp = old_logp_d;
  u.adv = adv_d;
  u.vtarget = vtarget_d;
  u.coef = coef;
  u.logstd_part = ctx->head_part;
  u.loss_part = ctx->head_part + static_cast<int64_t>(kHeadSplits) * A;
  u.splits = head_splits;
  const int hpl = hpl_for(std::max(u.da, u.dc));
  const int nj = (u.da == u.dc && u.da % 16 == 0) ? u.da / 16 : 0;
  const bool aligned = reinterpret_cast<uintptr_t>(u.ha) % 16 == 0 &&
                       reinterpret_cast<uintptr_t>(u.hc) % 16 == 0;
  const bool q4 = aligned && (nj == 2 || nj == 4 || nj == 8 || nj == 16 || nj == 32);
  const bool fused_head_w = q4 && A <= kFusedHeadAct;  // head dW/db inside the head kernel
  u.hw_part = ctx->head_w_part;
  u.hw_stride = ctx->hw_stride;
  u.off_ba = ctx->hw_off_ba;
  u.off_wc = ctx->hw_off_wc;
  u.off_bc = ctx->hw_off_bc;
  u.bf16 = ctx->prec == PPO_PREC_BF16;
  // algorithmic FLOPs: head forward + dH_L (+ head dW when fused); bytes per row: read H_L
  // (actor, critic), action, 4 scalars + row index; write dH_L (actor, critic) and dz (A + 1)
  const TimRec rec{KC_UPDATE_HEAD,
                   !tim_active() ? nullptr
                   : q4 ? intern_name("update_head_q4_kernel<%d, %s>", nj,
                                      fused_head_w ? "true" : "false")
                        : intern_name("update_head_kernel<%d>", hpl),
                   2.0 * b * ((fused_head_w ? 3.0 : 2.0) * (A * u.da + u.dc)),
                   4.0 * b * (2.0 * u.da + 2.0 * u.dc + 2.0 * A + 6.0)};
  if (q4) {
    const size_t shm = sizeof(float) * ((A + 1) * static_cast<size_t>(u.da) + 2 * 4 * 16 * kMaxAct);
    auto launch = [&](auto kernel) -> int {
      if (shm > 64 * 1024)
        PPO_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                        hipFuncAttributeMaxDynamicSharedMemorySize,
                                        static_cast<int>(shm)));
      launch_k(rec, kernel, dim3(head_splits), dim3(256), static_cast<uint32_t>(shm), st, u);
      return 0;
    };
    int rc = 0;
    if (fused_head_w) {
      if (nj == 2) rc = launch(update_head_q4_kernel<2, true>);
      else if (nj == 4) rc = launch(update_head_q4_kernel<4, true>);
      else if (nj == 8) rc = launch(update_head_q4_kernel<8, true>);
      else if (nj == 16) rc = launch(update_head_q4_kernel<16, true>);
      else rc = launch(update_head_q4_kernel<32, true>);
    } else {
      if (nj == 2) rc = launch(update_head_q4_kernel<2, false>);
      else if (nj == 4) rc = launch(update_head_q4_kernel<4, false>);
      else if (nj == 8) rc = launch(update_head_q4_kernel<8, false>);
      else if (nj == 16) rc = launch(update_head_q4_kernel<16, false>);
      else rc = launch(update_head_q4_kernel<32, false>);
    }
    if (rc) return rc;
  } else if (hpl == 4) {
    launch_k(rec, update_head_kernel<4>, dim3(head_splits), dim3(256), 0, st, u);
  } else if (hpl == 8) {
    launch_k(rec, update_head_kernel<8>, dim3(head_splits), dim3(256), 0, st, u);
  } else {
    launch_k(rec, update_head_kernel<16>, dim3(head_splits), dim3(256), 0, st, u);
  }
  PPO_LAUNCHED();

  // ---- weight gradients, split-K over rows, deepest layer first ---------------------------
  const int splits = std::min(kSlabSplits, std::max(1, b / 64));
  const int64_t P = ctx->total_params;
  auto partial = [&](int layer_from_top) -> int {
    // layer index per net: head = n_hidden, then n_hidden-1 ... 0
    GemmBatch gb{};
    gb.prec = ctx->prec;
    gb.k = b;
    gb.rows_n = count_d;
    gb.splits = splits;
    gb.slab_stride = P;
    int np = 0, max_m = 0, max_n = 0;
    for (int z = 0; z < 2; ++z) {
      NetDesc &nd = ctx->net[z];
      const int l = nd.n_hidden - layer_from_top;
      if (l < 0) continue;
      const LayerDesc &L = nd.layer[l];
      GemmProblem &Q = gb.p[np++];
      // dY of layer l: head -> dz, top hidden -> g, lower hidden -> h[l] (overwritten in place)
      Q.a = (l == nd.n_hidden) ? nd.dz : (l == nd.n_hidden - 1 ? nd.g : nd.h[l]);
      Q.lda = L.out;
      Q.b = (l == 0) ? ctx->xg : nd.h[l - 1];
      Q.ldb = (l == 0) ? ctx->ldx : L.in;
      Q.c = ctx->slabs + L.w_off;
      Q.ldc = L.in;
      Q.colsum = L.b_off >= 0 ? ctx->slabs + L.b_off : nullptr;
      Q.m = L.out;
      Q.n = L.in;
      max_m = std::max(max_m, L.out);
      max_n = std::max(max_n, L.in);
    }
    if (!np) return 0;
    if (np == 2 && (gb.p[0].m != gb.p[1].m || gb.p[0].n != gb.p[1].n) &&
        ((gb.p[0].m <= 32) != (gb.p[1].m <= 32) || (gb.p[0].n <= 32) != (gb.p[1].n <= 32))) {
      GemmBatch g1 = gb;
      g1.p[0] = gb.p[1];
      if (int rc = gemm_wgrad_partial(gb, 1, gb.p[0].m, gb.p[0].n, st)) return rc;
      return gemm_wgrad_partial(g1, 1, g1.p[0].m, g1.p[0].n, st);
    }
    return gemm_wgrad_partial(gb, np, max_m, max_n, st);
  };
  auto input_grad = [&](int layer_from_top) -> int {
    // dH_{l-1} = (dY_l W_l) * act'(H_{l-1}), written over H_{l-1}; l = n_hidden - layer_from_top
    GemmBatch gb{};
    gb.prec = ctx->prec;
    gb.rows_n = count_d;
    gb.act = ctx->cfg.activation;
    int np = 0, max_n = 0, kdim = -1;
    for (int z = 0; z < 2; ++z) {
      NetDesc &nd = ctx->net[z];
      const int l = nd.n_hidden - layer_from_top;
      if (l < 1 || l >= nd.n_hidden) continue;  // head handled in the head kernel
      const LayerDesc &L = nd.layer[l];
      if (kdim >= 0 && kdim != L.out) {
        if (int rc = gemm_rows_dx(gb, np, b, max_n, st)) return rc;
        np = 0;
        max_n = 0;
      }
      kdim = L.out;
      GemmProblem &Q = gb.p[np++];
      Q.a = (l == nd.n_hidden - 1) ? nd.g : nd.h[l];
      Q.lda = L.out;
      Q.b = ctx->params + L.w_off;
      Q.ldb = L.in;
      Q.c = nd.h[l - 1];
      Q.aux = nd.h[l - 1];
      Q.ldc = L.in;
      Q.m = b;
      Q.n = L.in;
      gb.k = L.out;
      max_n = std::max(max_n, L.in);
    }
    if (!np) return 0;
    return gemm_rows_dx(gb, np, b, max_n, st);
  };
  const int depth = std::max(NA.n_hidden, NC.n_hidden);
  for (int s = 0; s <= depth; ++s) {
    // dW of layer n_hidden - s (needs its input); the head's is already in head_w_part
    if (!(s == 0 && fused_head_w))
      if (int rc = partial(s)) return rc;
    if (int rc = input_grad(s)) return rc;    // then overwrite that input with its gradient
  }

  // ---- reduce slabs -> grad, loss scalars ---------------------------------------------------
  ReduceArgs r{};
  for (int z = 0; z < 2; ++z) {
    NetDesc &nd = ctx->net[z];
    if (z == 0)
      if (int rc = add_seg(r, nd.logstd_off, A, ctx->head_part, A, head_splits)) return rc;
    for (int l = 0; l <= nd.n_hidden; ++l) {
      const LayerDesc &L = nd.layer[l];
      // the head's dW / db come from the head kernel's own partials when it computed them
      const bool head_fused = fused_head_w && l == nd.n_hidden;
      const float *w_src = head_fused ? ctx->head_w_part + (z == 0 ? 0 : ctx->hw_off_wc)
                                      : ctx->slabs + L.w_off;
      const int64_t stride = head_fused ? ctx->hw_stride : P;
      const int nsplit = head_fused ? head_splits : splits;
      if (int rc = add_seg(r, L.w_off, static_cast<int64_t>(L.out) * L.in, w_src, stride, nsplit))
        return rc;
      if (L.b_off < 0) continue;
      const float *b_src = head_fused
                               ? ctx->head_w_part + (z == 0 ? ctx->hw_off_ba : ctx->hw_off_bc)
                               : ctx->slabs + L.b_off;
      if (int rc = add_seg(r, L.b_off, L.out, b_src, stride, nsplit)) return rc;
    }
  }
  set_loss_tail(r, P, grad_d, u.loss_part, head_splits, coef, ctx->params + NA.logstd_off, A,
                ctx->ent_log_share, loss_d);
  return reduce_slabs_launch(r, TimRec{KC_REDUCE, "reduce_slabs_kernel",
                                       static_cast<double>(splits) * P,
                                       4.0 * (static_cast<double>(splits) + 1) * P}, st);
}

}  // namespace ppo
