// The layered f32 path: the MLP actor-critic as one MFMA GEMM per layer (gemm.h through
// gemm_ops.h) around wave-per-row head kernels, in f32 operands (PPO_PREC_F32: the reference's
// precision, which the oracle tests compare against) or bf16-rounded ones for the shapes no other
// bf16 path covers.  Kernels and host code: layered_engine.hip.  ppo_policy_step /
// ppo_minibatch_grad (mlp_engine.hip) route here when neither fused_active() nor wide_active().
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ctx.h"
#include "ppo_loss.h"

namespace ppo {

// workspace extents of the path, allocated by ppo_ctx_create (ctx.h slabs / head_part / head_w_part)
constexpr int kSlabSplits = 64;   // split-K slabs of the weight gradients (at most)
constexpr int kHeadSplits = 512;  // row blocks of the update head (log-std / loss / head-dW partials)

// Forward through the hidden layers of the requested nets.  x: (rows, in) f32 with row stride
// ldx.  Nets whose layer-l shapes agree share one launch.
int forward_hidden(ppo_ctx *ctx, const bool use[2], const float *x, const int32_t *x_rows, int rows,
                   const int32_t *rows_n, hipStream_t st, int ldx);
int layered_policy_step(ppo_ctx *ctx, const float *state_d, int n, const float *eps_d,
                        uint64_t seed, uint64_t offset, float *action_d, float *logp_d,
                        float *value_d, float *mean_d, hipStream_t st);
int layered_minibatch_grad(ppo_ctx *ctx, const float *states_d, const float *actions_d,
                           const float *old_logp_d, const float *adv_d, const float *vtarget_d,
                           const int32_t *rows_d, int b, const int32_t *count_d,
                           const LossCoef &coef, float *grad_d, float *loss_d, hipStream_t st);

}  // namespace ppo
