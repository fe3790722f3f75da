// The implementation of timing.h for the whole library: the per-thread and ctx-free timing
// targets, the interned kernel names, the shared bodies of every engine's timing entry points and
// the kernel-class names.
#include "timing.h"

#include <cstdarg>
#include <cstdio>
#include <deque>
#include <mutex>
#include <string>

#include "common.h"

namespace ppo {

static const char *const kClassNames[KC_COUNT] = {
    "gemm_fwd",     "gemm_dgrad", "gemm_wgrad", "update_head", "policy_head", "reduce_slabs",
    "gather_states", "gae",       "adam",       "normalize_rows", "obs", "minibatch_rows",
    "env_harness", "fused_update", "lstm", "conv"};

thread_local Timing *g_tim = nullptr;
Timing *g_free_tim = nullptr;

const char *intern_name(const char *fmt, ...) {
  static std::mutex mu;
  static std::deque<std::string> names;
  char buf[160];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  std::lock_guard<std::mutex> lock(mu);
  for (const std::string &s : names)
    if (s == buf) return s.c_str();
  names.emplace_back(buf);
  return names.back().c_str();
}

void timing_release(Timing &t) {
  for (int i = 0; i < 2 * t.capacity; ++i) (void)hipEventDestroy(t.ev[i]);
  delete[] t.ev;
  delete[] t.cls;
  delete[] t.kname;
  delete[] t.flops;
  delete[] t.bytes;
}

int timing_enable(Timing &t, int enable, int capacity) {
  if (enable && capacity > t.capacity) {
    timing_release(t);
    t.ev = new hipEvent_t[2 * capacity];
    t.cls = new int[capacity];
    t.kname = new const char *[capacity];
    t.flops = new double[capacity];
    t.bytes = new double[capacity];
    for (int i = 0; i < 2 * capacity; ++i) PPO_HIP_TRY(hipEventCreate(&t.ev[i]));
    t.capacity = capacity;
  }
  if (enable) {
    t.used = 0;
    for (int c = 0; c < KC_COUNT; ++c) t.ms[c] = t.fl[c] = t.by[c] = 0, t.n[c] = 0;
    t.per_kernel.clear();
  }
  t.on = enable != 0 && t.capacity > 0;
  if (t.on) g_free_tim = &t;
  else if (g_free_tim == &t) g_free_tim = nullptr;
  return 0;
}

// Folds pending records into the per-class and per-kernel totals (host sync on their events).
static int timing_fold(Timing &t) {
  for (int i = 0; i < t.used; ++i) {
    PPO_HIP_TRY(hipEventSynchronize(t.ev[2 * i + 1]));
    float ms = 0.f;
    PPO_HIP_TRY(hipEventElapsedTime(&ms, t.ev[2 * i], t.ev[2 * i + 1]));
    const int c = t.cls[i];
    t.ms[c] += ms;
    t.fl[c] += t.flops[i];
    t.by[c] += t.bytes[i];
    t.n[c] += 1;
    const char *name = t.kname[i] ? t.kname[i] : kClassNames[c];
    KernelTotals *k = nullptr;
    for (KernelTotals &e : t.per_kernel)
      if (e.name == name) k = &e;
    if (!k) {
      t.per_kernel.push_back(KernelTotals{name, c, 0.0, 0.0, 0.0, 0});
      k = &t.per_kernel.back();
    }
    k->ms += ms;
    k->fl += t.flops[i];
    k->by += t.bytes[i];
    k->n += 1;
  }
  t.used = 0;
  return 0;
}

int timing_read_class(Timing &t, int kclass, double *total_ms, int64_t *launches, double *flops,
                      double *bytes) {
  if (kclass < 0) return KC_COUNT;
  PPO_REQUIRE(kclass < KC_COUNT, "timing read: class %d out of range", kclass);
  if (int rc = timing_fold(t)) return rc;
  if (total_ms) *total_ms = t.ms[kclass];
  if (launches) *launches = t.n[kclass];
  if (flops) *flops = t.fl[kclass];
  if (bytes) *bytes = t.by[kclass];
  return 0;
}

int timing_read_kernel(Timing &t, int index, const char **name, int *kclass, double *total_ms,
                       int64_t *launches, double *flops, double *bytes) {
  if (int rc = timing_fold(t)) return rc;
  const int count = static_cast<int>(t.per_kernel.size());
  if (index < 0) return count;
  PPO_REQUIRE(index < count, "timing read: kernel index %d out of range [0, %d)", index, count);
  const KernelTotals &k = t.per_kernel[index];
  if (name) *name = k.name;
  if (kclass) *kclass = k.cls;
  if (total_ms) *total_ms = k.ms;
  if (launches) *launches = k.n;
  if (flops) *flops = k.fl;
  if (bytes) *bytes = k.by;
  return 0;
}
}  // namespace ppo

using namespace ppo;

extern "C" const char *ppo_kernel_class_name(int kclass) {
  return (kclass >= 0 && kclass < KC_COUNT) ? kClassNames[kclass] : "";
}
