// The per-row PPO loss-head arithmetic, written once for every engine (MLP q4 / generic heads, the
// fused kernels, the wide path, CNN, BiLSTM).  Each function is one expression of the reference's
// torch ops, in torch's operation order; the build's -ffp-contract=off keeps every product and sum
// a rounding of its own, so inlining these changes no bit.
//
// Rollout (ppo.py:22-26): action = torch.normal(mean, std) = eps * std + mean, and
//   Normal.log_prob(x) = (-(x - mu)^2) / (2 var) - log(std) - log(sqrt(2 pi)),  var = std * std,
// summed over the actions.  The update (ppo.py:113) recomputes it with the SAME operation order,
// so a row whose parameters did not move has ratio == 1 to the bit.
//
// Update (ppo.py:108-135), with torch's autograd rules:
//   ratio = exp(logp - old_logp);  s1 = ratio * adv;  s2 = clamp(ratio, lo, hi) * adv;
//   actor loss = -mean(min(s1, s2)) - ent_coef * mean(entropy);  critic loss = mean(huber(v - vt)).
//   - torch.min / minimum propagates NaN, and on a tie hands HALF the gradient to each side.  A tie
//     is the common case: every row whose ratio lies inside the clip range has s1 == s2 exactly.
//   - clamp passes the gradient on the CLOSED interval [lo, hi].
//   - huber_loss (delta = 1) is 0.5 d^2 below 1 and |d| - 0.5 above; its backward clips d to +-1.
//   - tanh backward is grad * (1 - y * y) on the output y.
// Callers keep their own masking of padded rows (valid ? ... : 0) and their own reductions.
#pragma once

#include "common.h"

namespace ppo {

constexpr int kMaxAct = 32;  // most actions any head kernel is sized for

// The minibatch's loss coefficients: clip range, entropy coefficient, 1/B and 1/(B*A) (the two
// means' weights), as the C-ABI's minibatch entry points receive them.
struct LossCoef {
  float clip_lo, clip_hi, ent_coef, inv_b, inv_ba;
};

// The entropy coefficient of the LOGGED actor loss (ppo_*_loss_entropy_share: a data-parallel rank
// logs its share of the entropy term; the gradient always uses c.ent_coef itself).
inline float logged_ent_coef(const LossCoef &c, float ent_log_share) { return c.ent_coef * ent_log_share; }

// torch.normal(mean, std): randn * std, then + mean (two roundings, no FMA).
__device__ __forceinline__ float normal_sample(float eps, float sd, float mu) { return eps * sd + mu; }

// One action's Normal.log_prob term, d = x - mu.  The divide form: what torch computes, used by
// every rollout and update head that must agree with each other and the oracle to the bit.
__device__ __forceinline__ float normal_logp_term(float d, float var, float log_sd) {
  return ((-(d * d)) / (2.f * var) - log_sd) - kLogSqrt2Pi;
}

// The same term with the divide replaced by a multiply with half_ivar = 0.5 / var, which the
// caller forms once per action column.  It exists for the fused bf16 kernels (policy_fused_kernel
// and fused_update_kernel), whose rollout and update must agree with EACH OTHER and which keep the
// divide off their per-row path.  It rounds differently from normal_logp_term: never swap one for
// the other.
__device__ __forceinline__ float normal_logp_term_rcp(float d, float half_ivar, float log_sd) {
  return ((-(d * d)) * half_ivar - log_sd) - kLogSqrt2Pi;
}

// min(s1, s2) of one row and d(-inv_b * min) / d(logp), before any padded-row masking.
struct Surrogate {
  float mn, dlogp;
};
__device__ __forceinline__ Surrogate clipped_surrogate(float logp, float old_lp, float adv,
                                                       const LossCoef &c) {
  const float ratio = expf(logp - old_lp);
  const float s1 = ratio * adv;
  const float cl = ratio < c.clip_lo ? c.clip_lo : (ratio > c.clip_hi ? c.clip_hi : ratio);
  const float s2 = cl * adv;
  const float mn = (s1 != s1 || s2 != s2) ? (s1 + s2) : (s2 < s1 ? s2 : s1);
  const float g = -c.inv_b;
  const float g1 = (s1 < s2) ? g : (s1 == s2 ? g * 0.5f : 0.f);
  const float g2 = (s2 < s1) ? g : (s1 == s2 ? g * 0.5f : 0.f);
  const bool inside = (ratio >= c.clip_lo) && (ratio <= c.clip_hi);
  const float dratio = g1 * adv + (inside ? g2 * adv : 0.f);
  return {mn, dratio * ratio};
}

__device__ __forceinline__ float huber(float diff) {
  const float ad = fabsf(diff);
  return (ad < 1.f) ? 0.5f * ad * ad : (ad - 0.5f);
}
__device__ __forceinline__ float huber_grad(float diff, float inv_b) {
  return inv_b * (diff < -1.f ? -1.f : (diff > 1.f ? 1.f : diff));
}

// Backward of the tanh-Gaussian head with a state-independent log-std (mean = omv * y,
// y = tanh(z), d = x - mean): d loss / dz, and one row's term of d loss / d logstd (the entropy
// mean's share included).  The _rcp forms multiply by ivar = 1 / var where the others divide
// (fused_update_kernel); like the two log-prob forms they are not interchangeable.
__device__ __forceinline__ float tanh_mean_grad(float dlogp, float d, float var, float omv, float y) {
  const float dmu = dlogp * (d / var);
  return (dmu * omv) * (1.f - y * y);
}
__device__ __forceinline__ float logstd_grad(float dlogp, float d, float var, const LossCoef &c) {
  return dlogp * ((d * d) / var - 1.f) - c.ent_coef * c.inv_ba;
}
__device__ __forceinline__ float tanh_mean_grad_rcp(float dlogp, float d, float ivar, float omv, float y) {
  const float dmu = dlogp * (d * ivar);
  return (dmu * omv) * (1.f - y * y);
}
__device__ __forceinline__ float logstd_grad_rcp(float dlogp, float d, float ivar, const LossCoef &c) {
  return dlogp * ((d * d) * ivar - 1.f) - c.ent_coef * c.inv_ba;
}

}  // namespace ppo
