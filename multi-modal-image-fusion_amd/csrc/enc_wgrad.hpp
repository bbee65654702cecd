// Reduction of the DenseBlock encoder's weight gradients, shared by csrc/enc_wgrad.hip (tile kernel, round 2) and csrc/enc_bwd.hip (the fused
// chain + weight-gradient kernel, round 5); the partial's layout (EW_*, EwDst, the map enc_wgrad_reduce) is in wgrad_reduce.hpp.
#pragma once
#include "wgrad_reduce.hpp"

namespace mmif {

constexpr int EW_MAXG = 512;

// fixed-order sum of G partials (EW_PER floats each) into the four layers' dW / db for two branches in one launch (same summation order as
// two launches of wgrad_reduce_launch(enc_wgrad_reduce{D}, ...); shared destinations are summed one after the other)
int enc_wgrad_reduce_pair_launch(const float* pa, const EwDst& Da, int acc_a, const float* pb, const EwDst& Db, int acc_b, int G, hipStream_t st);

}  // namespace mmif
