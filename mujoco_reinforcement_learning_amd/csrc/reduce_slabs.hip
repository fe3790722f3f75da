// The split-K slab fold as a kernel of its own (reduce_slabs.h): the layered and fused MLP paths,
// the data-parallel fused step, the pixel CNN and the BiLSTM's unaligned case launch it here.
#include "reduce_slabs.h"

namespace ppo {

__global__ __launch_bounds__(kRedThreads) void reduce_slabs_kernel(ReduceArgs q) {
  (void)reduce_slab_block(q, blockIdx.x);
}

int reduce_slabs_launch(const ReduceArgs &r, const TimRec &rec, hipStream_t st) {
  launch_k(rec, reduce_slabs_kernel, dim3(ceil_div(r.total, kRedParams)), dim3(kRedThreads), 0, st,
           r);
  PPO_LAUNCHED();
  return 0;
}

}  // namespace ppo
