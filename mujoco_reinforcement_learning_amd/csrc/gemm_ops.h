// The layered engine's GEMMs (gemm.h templates) instantiated ONCE, in gemm_ops.hip, and called
// from the MLP engine, the BiLSTM and the pixel encoder's heads through these plain functions:
// every translation unit that instantiated the templates itself paid minutes of compile time.
#pragma once

#include "gemm.h"

namespace ppo {

// C = act(A B^T + bias), A [rows][k], B [n][k] (torch Linear weights)
int gemm_rows_fwd_nk(const GemmBatch &gb, int nprob, int rows, int max_n, hipStream_t st);
// C = act(A B + bias), B [k][n]
int gemm_rows_fwd_kn(const GemmBatch &gb, int nprob, int rows, int max_n, hipStream_t st);
// C = (A B) * act'(aux), B [k][n]
int gemm_rows_dx(const GemmBatch &gb, int nprob, int rows, int max_n, hipStream_t st);
// slab[split] = A^T B over a row range per split (+ column sums of A)
int gemm_wgrad_partial(const GemmBatch &gb, int nprob, int max_m, int max_n, hipStream_t st);

// One batch of np problems through the calls above.
inline GemmBatch gemm_batch(int prec, const GemmProblem *p, int np, int k, int act) {
  GemmBatch gb{};
  for (int i = 0; i < np; ++i) gb.p[i] = p[i];
  gb.k = k;
  gb.act = act;
  gb.prec = prec;
  return gb;
}
inline int gemm_fwd(int prec, const GemmProblem *p, int np, int k, int rows, int max_n, int act,
                    bool b_kn, hipStream_t st) {
  const GemmBatch gb = gemm_batch(prec, p, np, k, act);
  return b_kn ? gemm_rows_fwd_kn(gb, np, rows, max_n, st)
              : gemm_rows_fwd_nk(gb, np, rows, max_n, st);
}
inline int gemm_dx(int prec, const GemmProblem *p, int np, int k, int rows, int max_n, int act,
                   hipStream_t st) {
  return gemm_rows_dx(gemm_batch(prec, p, np, k, act), np, rows, max_n, st);
}
inline int gemm_partial(int prec, const GemmProblem *p, int np, int rows, int max_m, int max_n,
                        int splits, int64_t slab_stride, hipStream_t st) {
  GemmBatch gb = gemm_batch(prec, p, np, rows, 0);
  gb.splits = splits;
  gb.slab_stride = slab_stride;
  return gemm_wgrad_partial(gb, np, max_m, max_n, st);
}

}  // namespace ppo
