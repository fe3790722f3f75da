// Fused bf16 rollout policy step (fused_policy.hip): host-side argument block and launcher.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "fused_update.h"
#include "timing.h"

namespace ppo {

constexpr int kPolicyMaxWindow = 1;  // one net per workgroup: both read the window, W=1 only

struct PolicySlices {  // feature-slice edges of the per-sample standardisation (A1)
  int32_t edge[16];
  int32_t count;
};

struct PolicyFusedArgs {
  FusedNet net[2];               // bf16 W0 / W1 images + f32 biases and heads (w1bt unused)
  const float *logstd;
  int n, obs_dim, window, act_dim, act, hidden;
  float omv;
  // A1: window (N, O, W) f64 updated in place when obs_d != null (push), reset_d / all_reset as
  // ppo_obs_window_push; the standardised state (N, W*O) f32 is written to state_d
  double *window_d;
  const double *obs_d;
  const uint8_t *reset_d;
  int all_reset;
  PolicySlices tab;
  int normalize;
  float *state_d;
  // A2-A4 (each output nullable)
  int do_actor, do_critic;
  const float *eps;
  uint64_t seed, offset;
  const uint64_t *offset_base;
  uint64_t *stamps;              // diagnostics (ReLU only): (2, 128, 11) per-phase cycles, or null
  float *action, *logp, *value, *mean;
};

int policy_fused_launch(const PolicyFusedArgs &q, const TimRec &rec, hipStream_t st);

// All T steps of the synthetic device VecEnv (device_env.h) and the actor in one launch
// (rollout_persistent_kernel): a workgroup owns 32 envs for the whole rollout.  Time-major
// buffers: base_obs (T+1, N, O), base_reward / base_term (T, N), noise (T, N, A); outputs states
// (T+1, N, O), actions (T, N, A), logp (T, N), reward f64 (T, N), terminated (T, N); window_d
// (N, O) f64 holds observation 0 on entry and observation T on exit.
struct RolloutArgs {
  FusedNet net;                  // the actor
  const float *logstd;
  int n, obs_dim, act_dim, act, hidden, t_len;
  float omv;
  double *window_d;
  const float *base_obs, *base_reward;
  const uint8_t *base_term;
  PolicySlices tab;
  int normalize;
  const float *noise;
  float *states, *actions, *logp;
  double *reward;
  uint8_t *terminated;
  uint64_t *stamps;              // diagnostics (ReLU, A in (4, 6]): (2, 128, 11) as the step kernel
};
int rollout_persistent_launch(const RolloutArgs &q, const TimRec &rec, hipStream_t st);

// The critic's forward over ``rows`` rows of standardised f32 states (value_batch_kernel):
// per row bitwise the value the step kernel's critic workgroups compute from the same state.
struct ValueBatchArgs {
  FusedNet net;                  // the critic
  int obs_dim, act, hidden;
  int64_t rows;
  int tiles, tiles_per_wg;       // 32-row tiles in all / per workgroup (contiguous shares)
  const float *states;
  float *values;
};
int value_batch_launch(ValueBatchArgs q, int num_cu, const TimRec &rec, hipStream_t st);

}  // namespace ppo
