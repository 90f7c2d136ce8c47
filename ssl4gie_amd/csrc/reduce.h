// Sums over one 256-thread workgroup (four waves): the block sum and the 256-entry LDS tree; wave_sum is in common.h.
// THE ORDER OF THE ADDITIONS IS PART OF WHAT A KERNEL PROMISES (bit-equal curves, fp64 bounds with a measured k), so
// every site names it, and it changes only together with the results recorded for that kernel:
//   Pairwise   (r0 + r1) + (r2 + r3): det_ops mapln_stats; metric_ops depth_sums, depth_err (fp64); optim_ops
//              grad_norm_partial, grad_norm_final (fp64); loss_ops nce_finalize, ce_rows, soft_ce_rows
//   Sequential r0 + r1 + r2 + r3: loss_ops ssi_sums, ssi_grad, dice_sums, bt_loss_partial; det_ops mapln_reduce;
//              optim_ops lars_norm_partial; metric_ops seg_counts (integers); color_ops' two stats kernels start
//              from 0.f (a -0 total comes out +0) and keep their loop
// A kernel uses a helper only where its device assembly stays what it was (profiles/reduce_header.md lists the sites
// that stay written out).  Sums over part of a wave (conv_direct, attention, bn_block_reduce) are other operations.
#pragma once
#include "common.h"

enum class SumOrder { Pairwise, Sequential };

// lane 0 of every wave stores the wave's K totals, sh[wave][k]; then a barrier; then block_get adds the four in order O
template <int K, typename T>
DEVI void block_put(const T (&v)[K], T* sh /* [4][K] */) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) sh[wave * K + k] = v[k];
}
template <typename T>
DEVI void block_put(T v, T* sh /* [4] */) {
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
}
template <SumOrder O, int K = 1, typename T>
DEVI T block_get(const T* sh /* [4][K] */, int k = 0) {
    if constexpr (O == SumOrder::Pairwise) return (sh[k] + sh[K + k]) + (sh[2 * K + k] + sh[3 * K + k]);
    else return sh[k] + sh[K + k] + sh[2 * K + k] + sh[3 * K + k];
}
// K sums; v holds them ON THREAD 0 ONLY afterwards
template <SumOrder O, int K, typename T>
DEVI void block_sum(T (&v)[K], T* sh /* [4][K] */) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
    block_put(v, sh);
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = block_get<O, K>(sh, k);
}
// one sum, ON EVERY THREAD after the one barrier: the caller does not write sh again (a second sum, a second slot)
template <SumOrder O, typename T>
DEVI T block_sum_all(T v, T* sh /* [4] */) {
    block_put(wave_sum(v), sh);
    __syncthreads();
    return block_get<O>(sh);
}
// closes a two-stage reduction: thread t has stored sh[k][t]; sh[k][0] is the total after the last barrier
template <int K, typename T>
DEVI void block_tree_sum(T (&sh)[K][256], int t) {
    static_assert(K <= 2, "spelled out, not a loop over k: a loop loads the operands of each addition the other way");
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            sh[0][t] += sh[0][t + o];
            if constexpr (K > 1) sh[1][t] += sh[1][t + o];
        }
        __syncthreads();
    }
}
