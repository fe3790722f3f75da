// The synthetic VecEnv's dynamics (oracle/ppo_ref.py RefSyntheticEnv), one definition for every
// kernel that steps it: synthetic_env_step_kernel, synthetic_test_step_kernel (scan_kernels.hip)
// and rollout_persistent_kernel (fused_policy.hip).  All three are f64 and are compiled with
// -ffp-contract=off, so the multiply and the add below stay two roundings everywhere.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ppo {
namespace denv {

// obs'[f] = base_obs[f] + 0.1 a[f % A]; ``act`` is a[f % A]
__device__ __forceinline__ double next_obs(float base, float act) {
  return static_cast<double>(base) + 0.1 * static_cast<double>(act);
}

// r = base_reward - 0.01 sum_j a_j^2, the sum sequential in j order
template <typename ActionAt>
__device__ __forceinline__ double reward(float base_r, int a, ActionAt action_at) {
  double ctrl = 0.0;
  for (int j = 0; j < a; ++j) {
    const double aj = static_cast<double>(action_at(j));
    ctrl = ctrl + aj * aj;
  }
  return static_cast<double>(base_r) - 0.01 * ctrl;
}

// termination comes from the stream unchanged
__device__ __forceinline__ uint8_t terminated(uint8_t base_t) { return base_t; }

}  // namespace denv
}  // namespace ppo
