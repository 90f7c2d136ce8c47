// The scoring around a FROZEN trunk in the linear probe (Models/mae/main_linprobe.py, Models/moco_v3/main_lincls.py).
// The trunk forward is the bulk of a probe step and is not touched here; the head's SGD step is in optim_ops.hip.
//
// topk_update  the drivers score every batch with accuracy(output, target, topk=(1, 5)) (main_lincls.py:506-520; timm's
//              accuracy in Models/mae/engine_finetune.py:19,119-124) and the criterion's value, and read each meter
//              back with .item(): topk + eq + three reductions + three host synchronisations per batch.  Here one pass
//              per row gives the RANK of the target's logit and the row's cross-entropy; hits per k, rows counted, rows
//              rejected and the loss sum add up in caller-owned device buffers over a whole loader.
//              One wave per row, four rows per workgroup.  A row is walked in 16-byte chunks (4 fp32 / 8 bf16 columns),
//              chunk q by lane q % 64: a chunk that lies inside the row and is 16-byte aligned is ONE load, any other is
//              read column by column — the same columns on the same lane either way, so a row's loss has the same bits
//              whatever `ld` and the row's alignment are.  Integer counts by integer atomics (order-free); the losses
//              go through a per-row fp32 workspace and are added in fp64 by ONE workgroup in a fixed order (thread t:
//              rows t, t + 256, ... in index order, then the 256-entry LDS tree of reduce.h): no floating-point atomics,
//              the same bits from run to run and for any grid.
#include "reduce.h"
#include "ssl4gie_hip.h"

namespace {
constexpr int TOPK_MAX = 8;
struct TopK { int k[TOPK_MAX]; };

template <typename T> struct Chunk;
template <> struct Chunk<float> {
    static constexpr int V = 4;
    static DEVI void ld(const float* p, float (&v)[4]) {
        const f32x4 r = ld4(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = r[j];
    }
};
template <> struct Chunk<bf16_t> {
    static constexpr int V = 8;
    static DEVI void ld(const bf16_t* p, float (&v)[8]) {
        const u32x4 r = *(const u32x4*)p;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[2 * j] = __uint_as_float(r[j] << 16);
            v[2 * j + 1] = __uint_as_float(r[j] & 0xffff0000u);
        }
    }
};
// chunk q of a row: columns [q V, q V + V); n = how many of them lie inside the row (the rest of v is not read)
template <typename T>
DEVI int load_chunk(const T* __restrict__ x, int q, int C, bool aligned, float (&v)[Chunk<T>::V]) {
    constexpr int V = Chunk<T>::V;
    const int c0 = q * V, n = C - c0 < V ? C - c0 : V;
    if (aligned && n == V) {
        Chunk<T>::ld(x + c0, v);
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j)
            if (j < n) v[j] = Elem<T>::ld(x + c0 + j);
    }
    return n;
}

// acc: [0, nk) hits per k | [nk] rows counted | [nk + 1] rows rejected.  ws fp32 [B]: the row's loss, 0 for a rejected row
template <typename T>
__global__ __launch_bounds__(256) void topk_rows_kernel(const T* __restrict__ logits, long long ld,
                                                        const long long* __restrict__ target, TopK ks, int nk,
                                                        unsigned long long* __restrict__ acc, int* __restrict__ rank_out,
                                                        float* __restrict__ row_loss, float* __restrict__ ws, int B, int C) {
    constexpr int V = Chunk<T>::V;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nchunk = (C + V - 1) / V;
    int cnt[TOPK_MAX + 2];  // the wave's totals (the same on every lane)
#pragma unroll
    for (int j = 0; j < TOPK_MAX + 2; ++j) cnt[j] = 0;
    for (long long row = (long long)blockIdx.x * 4 + wave; row < B; row += (long long)gridDim.x * 4) {
        const long long tg = target[row];
        if (tg < 0 || tg >= C) {  // wave-uniform; never used as an index
            ++cnt[TOPK_MAX + 1];
            if (lane == 0) {
                ws[row] = 0.f;
                if (rank_out) rank_out[row] = -1;
                if (row_loss) row_loss[row] = 0.f;
            }
            continue;
        }
        const T* x = logits + (size_t)row * (size_t)ld;
        const bool aligned = ((uintptr_t)x & 15) == 0;
        const float xt = Elem<T>::ld(x + tg);
        const bool tnan = xt != xt;
        // pass 1: the row maximum (NaNs aside) and the columns ordered above the target: a NaN above every number,
        // equal values (and NaNs among themselves) by lower index first
        float m = -INFINITY;
        int above = 0;
        for (int q = lane; q < nchunk; q += 64) {
            float v[V];
            const int n = load_chunk<T>(x, q, C, aligned, v);
#pragma unroll
            for (int j = 0; j < V; ++j)
                if (j < n) {
                    const float a = v[j];
                    const int c = q * V + j;
                    const bool anan = a != a;
                    m = fmaxf(m, a);
                    const bool tie = tnan ? anan : a == xt;
                    const bool over = !tnan && (anan || a > xt);
                    above += (over || (tie && c < tg)) ? 1 : 0;
                }
        }
        m = wave_max(m);
        above = wave_sum(above);
        // pass 2 (the row is in the cache): sum exp(x - max); a NaN in the row makes the sum and the loss NaN
        float s = 0.f;
        for (int q = lane; q < nchunk; q += 64) {
            float v[V];
            const int n = load_chunk<T>(x, q, C, aligned, v);
#pragma unroll
            for (int j = 0; j < V; ++j)
                if (j < n) s += expf(v[j] - m);
        }
        const float loss = logf(wave_sum(s)) + (m - xt);  // (m - xt first: a dominant target loses nothing to the sum's size)
#pragma unroll
        for (int j = 0; j < TOPK_MAX; ++j) cnt[j] += (j < nk && above < ks.k[j]) ? 1 : 0;
        ++cnt[TOPK_MAX];
        if (lane == 0) {
            ws[row] = loss;
            if (rank_out) rank_out[row] = above;
            if (row_loss) row_loss[row] = loss;
        }
    }
    __shared__ int sh[4 * (TOPK_MAX + 2)];
    block_put(cnt, sh);
    __syncthreads();
    const int t = threadIdx.x;
    if (t < TOPK_MAX + 2) {
        const int total = block_get<SumOrder::Sequential, TOPK_MAX + 2>(sh, t);
        const int slot = t < TOPK_MAX ? t : nk + (t - TOPK_MAX);
        if (total != 0 && (t >= TOPK_MAX || t < nk)) atomicAdd(acc + slot, (unsigned long long)total);
    }
}
// one workgroup: loss_sum += the B row losses, thread t adding rows t, t + 256, ... in index order, then the LDS tree
__global__ __launch_bounds__(256) void topk_loss_kernel(const float* __restrict__ ws, double* __restrict__ loss_sum, int B) {
    __shared__ double sh[1][256];
    const int t = threadIdx.x;
    double a = 0.0;
    for (int r = t; r < B; r += 256) a += (double)ws[r];
    sh[0][t] = a;
    block_tree_sum(sh, t);
    if (t == 0) *loss_sum += sh[0][0];
}
}  // namespace

extern "C" size_t ssl4gie_topk_workspace_bytes(int B) { return B > 0 ? align256((size_t)B * sizeof(float)) : 0; }

extern "C" int ssl4gie_topk_update(const void* logits, int dtype, long long ld, const long long* target, const int* ks,
                                   int nk, long long* acc, double* loss_sum, int* rank, float* row_loss, int B, int C,
                                   void* workspace, void* stream) {
    REQUIRE(logits && target && ks && acc && loss_sum && workspace && B > 0 && C > 0 && C <= (1 << 30) && ld >= C);
    REQUIRE(dtype == SSL4GIE_F32 || dtype == SSL4GIE_BF16);
    REQUIRE(nk >= 1 && nk <= TOPK_MAX);
    REQUIRE((uintptr_t)logits % (dtype == SSL4GIE_F32 ? 4 : 2) == 0 && (uintptr_t)loss_sum % 8 == 0 &&
            (uintptr_t)acc % 8 == 0 && (uintptr_t)workspace % 4 == 0);
    TopK k;
    for (int j = 0; j < TOPK_MAX; ++j) {
        k.k[j] = j < nk ? ks[j] : 0;
        if (j < nk) REQUIRE(ks[j] >= 1 && ks[j] <= C && (j == 0 || ks[j] > ks[j - 1]));
    }
    hipStream_t st = (hipStream_t)stream;
    const int nblk = (B + 3) / 4 < 2048 ? (B + 3) / 4 : 2048;
    unsigned long long* a = (unsigned long long*)acc;
    float* ws = (float*)workspace;
    if (dtype == SSL4GIE_F32)
        hipLaunchKernelGGL(topk_rows_kernel<float>, dim3(nblk), dim3(256), 0, st, (const float*)logits, ld, target, k, nk,
                           a, rank, row_loss, ws, B, C);
    else
        hipLaunchKernelGGL(topk_rows_kernel<bf16_t>, dim3(nblk), dim3(256), 0, st, (const bf16_t*)logits, ld, target, k,
                           nk, a, rank, row_loss, ws, B, C);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(topk_loss_kernel, dim3(1), dim3(256), 0, st, (const float*)ws, loss_sum, B);
    LAUNCH_CHECK();
    return 0;
}
