// What the pixel (ppo_cnn_ctx) and BiLSTM (ppo_lstm_ctx) contexts share: the flat parameter
// layout, the bound parameters, the workspace arena, precision and timing, and the bodies of the
// entry points that touch nothing else.  `who` is the entry point's name (check_rows: the
// engine's prefix) for the error message.  ppo_ctx keeps its own entry points: its ABI differs.
#pragma once

#include <algorithm>
#include <vector>

#include "common.h"
#include "timing.h"

namespace ppo {

struct EncoderCtx {
  int device;
  int prec;
  float ent_log_share;  // ppo_*_loss_entropy_share (logged actor loss only)
  int64_t total, n_actor;
  std::vector<int64_t> offsets;  // torch parameters() order, actor then critic
  float *params;
  void *ws;      // the workspace arena
  int64_t rows;  // workspace rows
  int maxw;      // widest MLP layer output
  Timing tim;
};

inline int ctx_param_layout(const EncoderCtx *x, const char *who, int64_t *offsets,
                            int max_tensors, int64_t *total, int64_t *n_actor) {
  PPO_REQUIRE(x != nullptr, "%s: null ctx", who);
  const int n = static_cast<int>(x->offsets.size());
  if (offsets)
    for (int i = 0; i < std::min(n, max_tensors); ++i) offsets[i] = x->offsets[i];
  if (total) *total = x->total;
  if (n_actor) *n_actor = x->n_actor;
  return n;
}

inline int ctx_bind_params(EncoderCtx *x, const char *who, float *params_d) {
  PPO_REQUIRE(x != nullptr && params_d != nullptr, "%s: null argument", who);
  PPO_REQUIRE(reinterpret_cast<uintptr_t>(params_d) % 64 == 0,
              "%s: parameter buffer must be 64-B aligned", who);
  x->params = params_d;
  return 0;
}

inline int ctx_loss_entropy_share(EncoderCtx *x, const char *who, float share) {
  PPO_REQUIRE(x != nullptr, "%s: null ctx", who);
  x->ent_log_share = share;
  return 0;
}

inline int ctx_set_precision(EncoderCtx *x, const char *who, int prec) {
  PPO_REQUIRE(x != nullptr, "%s: null ctx", who);
  PPO_REQUIRE(prec == PPO_PREC_F32 || prec == PPO_PREC_BF16, "%s: %d", who, prec);
  x->prec = prec;
  return 0;
}

inline int ctx_timing(EncoderCtx *x, const char *who, int enable, int capacity) {
  PPO_REQUIRE(x != nullptr, "%s: null ctx", who);
  return timing_enable(x->tim, enable, capacity);
}

inline int ctx_timing_kernel(EncoderCtx *x, const char *who, int index, const char **name,
                             int *kclass, double *total_ms, int64_t *launches, double *flops,
                             double *bytes) {
  PPO_REQUIRE(x != nullptr, "%s: null ctx", who);
  return timing_read_kernel(x->tim, index, name, kclass, total_ms, launches, flops, bytes);
}

inline int ctx_check_rows(const EncoderCtx *x, const char *who, int b) {
  PPO_REQUIRE(x != nullptr, "%s: null ctx", who);
  PPO_REQUIRE(b >= 0 && b <= x->rows, "%s: %d rows exceed the workspace (%lld)", who, b,
              static_cast<long long>(x->rows));
  PPO_REQUIRE(x->params != nullptr, "%s: parameters not bound (%s_bind_params)", who, who);
  return 0;
}

// The tail of both destroys: this context stops being the ctx-free timing target, its timing
// records and arena go.
inline void ctx_release(EncoderCtx *x) {
  (void)timing_enable(x->tim, 0, 0);
  timing_release(x->tim);
  if (x->ws) (void)hipFree(x->ws);
}

}  // namespace ppo
