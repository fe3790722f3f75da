// The MLP behind an encoder (the pixel encoder's heads, the BiLSTM's mean / log-std / critic
// MLPs): its layer table and flat parameter offsets, and the forward / WGRAD-partial / DX
// ping-pong over gemm_ops.h.  One or two MLPs of equal depth run as one ladder; at a layer where
// their shapes agree they share a launch sized by problem 0, otherwise each gets its own,
// problem 0 first.  Host code only; the layered f32 path keeps its own ladder.
#pragma once

#include "common.h"
#include "gemm_ops.h"

namespace ppo {

struct MlpLayer {
  int in, out, act;
  int64_t w, b;  // b < 0: no bias
};
struct Mlp {
  int n;  // layers incl. the output layer
  MlpLayer l[PPO_MAX_LAYERS + 1];
};

// Cfg: ppo_cnn_cfg / ppo_lstm_cfg (n_hidden, hidden[], activation)
template <class Cfg>
void add_mlp(Mlp &m, int in, const Cfg &c, int out, int final_act, bool bias, ParamLayout &lay) {
  m.n = c.n_hidden + 1;
  for (int l = 0; l < m.n; ++l) {
    MlpLayer &L = m.l[l];
    L.in = in;
    L.out = l < c.n_hidden ? c.hidden[l] : out;
    L.act = l < c.n_hidden ? c.activation : final_act;
    L.w = lay.add(static_cast<int64_t>(L.in) * L.out);
    L.b = bias ? lay.add(L.out) : -1;
    in = L.out;
  }
}

struct MlpProblem {
  const Mlp *m;
  const float *in;      // layer-0 input [b][in0]
  const __bf16 *in16;   // nullable: the same rows as bf16, read instead of `in` (forward A, WGRAD
                        // B and the DX's activation-derivative operand of layer 0)
  float *const *acts;   // layer outputs [b][out]
  float *const *pp;     // backward: the ping-pong pair; pp[0] holds the output-layer gradient
  float *din;           // backward: where the layer-0 input gradient goes
};

struct MlpLadder {
  int prec;
  const float *params;
  int np;  // 1 or 2 problems
  MlpProblem p[2];
  // backward only
  float *slabs;  // split-K slab base, indexed by the flat parameter offsets
  int splits;
  int64_t slab_stride;
  int64_t ld_din;  // leading dimension of din
  int in_act;      // the activation whose derivative (of the layer-0 input) is applied at din
};

// Whether layer l of every problem goes out as one launch (with_act: the activations agree too).
inline bool mlp_one_launch(const MlpLadder &q, int l, bool with_act) {
  if (q.np == 1) return true;
  const MlpLayer &A = q.p[0].m->l[l], &C = q.p[1].m->l[l];
  return A.in == C.in && A.out == C.out && (!with_act || A.act == C.act);
}

// Forward of every layer: act(A W^T + bias) into acts[l].
inline int mlp_forward(const MlpLadder &q, int b, hipStream_t st) {
  const float *P = q.params;
  for (int l = 0; l < q.p[0].m->n; ++l) {
    GemmProblem p[2] = {};
    for (int k = 0; k < q.np; ++k) {
      const MlpLayer &L = q.p[k].m->l[l];
      p[k].a = l == 0 ? q.p[k].in : q.p[k].acts[l - 1];
      if (l == 0) p[k].a16 = q.p[k].in16;
      p[k].lda = L.in;
      p[k].b = P + L.w;
      p[k].ldb = L.in;
      p[k].c = q.p[k].acts[l];
      p[k].ldc = L.out;
      p[k].bias = L.b >= 0 ? P + L.b : nullptr;
      p[k].m = b;
      p[k].n = L.out;
    }
    const bool one = mlp_one_launch(q, l, true);
    for (int z = 0; z < (one ? 1 : q.np); ++z) {
      const MlpLayer &L0 = q.p[z].m->l[l];
      if (int rc = gemm_fwd(q.prec, p + z, one ? q.np : 1, L0.in, b, L0.out, L0.act, false, st))
        return rc;
    }
  }
  return 0;
}

// Backward from pp[0] (gradient of the output layer's pre-activation, [b][out]): per layer and
// launch group the weight-gradient partials into the slabs, then dX = (dZ W) * act'(X) -- into
// the other ping-pong buffer for l > 0, into din (times in_act'(in)) at layer 0.
inline int mlp_backward(const MlpLadder &q, int b, hipStream_t st) {
  const float *P = q.params;
  float *cur[2] = {q.p[0].pp[0], q.np == 2 ? q.p[1].pp[0] : nullptr};
  for (int l = q.p[0].m->n - 1; l >= 0; --l) {
    GemmProblem pw[2] = {}, px[2] = {};
    float *nxt[2] = {nullptr, nullptr};
    for (int k = 0; k < q.np; ++k) {
      const MlpProblem &m = q.p[k];
      const MlpLayer &L = m.m->l[l];
      pw[k].a = cur[k];
      pw[k].lda = L.out;
      pw[k].b = l == 0 ? m.in : m.acts[l - 1];
      if (l == 0) pw[k].b16 = m.in16;
      pw[k].ldb = L.in;
      pw[k].c = q.slabs + L.w;
      pw[k].ldc = L.in;
      pw[k].colsum = L.b >= 0 ? q.slabs + L.b : nullptr;
      pw[k].m = L.out;
      pw[k].n = L.in;
      px[k].a = cur[k];
      px[k].lda = L.out;
      px[k].b = P + L.w;
      px[k].ldb = L.in;
      if (l > 0) {
        nxt[k] = m.pp[cur[k] == m.pp[0] ? 1 : 0];
        px[k].c = nxt[k];
        px[k].ldc = L.in;
        px[k].aux = m.acts[l - 1];
      } else {
        px[k].c = m.din;
        px[k].ldc = q.ld_din;
        px[k].aux = m.in;
        px[k].aux16 = m.in16;
      }
      px[k].m = b;
      px[k].n = L.in;
    }
    const bool one = mlp_one_launch(q, l, false);
    for (int z = 0; z < (one ? 1 : q.np); ++z) {
      const int n = one ? q.np : 1;
      const MlpLayer &L0 = q.p[z].m->l[l];
      if (int rc = gemm_partial(q.prec, pw + z, n, b, L0.out, L0.in, q.splits, q.slab_stride, st))
        return rc;
      const int act = l > 0 ? q.p[z].m->l[l - 1].act : q.in_act;
      if (int rc = gemm_dx(q.prec, px + z, n, L0.out, b, L0.in, act, st)) return rc;
    }
    cur[0] = nxt[0];
    cur[1] = nxt[1];
  }
  return 0;
}

}  // namespace ppo
