// Optimizer steps over the parameter arena: AdamW as the reference drives it
// (torch.optim.AdamW, Models/mae/main_pretrain.py:179-180, train_depth.py:280) and LARS
// (Models/moco_v3/moco/optimizer.py:18-43) as ONE or THREE launches over the flat fp32 buffers of
// engine.ParamArena instead of a multi-tensor launch chain per step, and the linear probe's SGD
// (Models/moco_v3/main_lincls.py:236-238) as one launch over a sub-range of them.
//
// The arena is a sequence of segments (one per parameter, 64-element aligned, padding belongs to the
// preceding parameter and stays zero); per-segment hyper-parameters come from small device tables:
//   seg_start [S + 1]  element offsets (int64, ascending, seg_start[S] = arena length)
//   seg_lr    [S]      learning rate of the segment's group; < 0: skip the segment (frozen
//                      parameter, or no gradient this step — torch skips p.grad is None too)
//   seg_wd    [S]      weight decay
//   seg_mat   [S]      LARS only: 1 for p.ndim > 1 (trust-ratio scaling + weight decay), else 0
// HBM-bound streaming: 16-byte accesses, no atomics, fixed summation order.
//
// The reference's scaler object (Models/mae/util/misc.py:251-292: unscale_ -> grad norm / clip ->
// scaler.step) is three more kernels over the same tables, around a 4-float device control block
//   ctl[0] global L2 norm of inv_scale * g over the active segments
//   ctl[1] clip coefficient min(1, max_norm / (norm + 1e-6)); exactly 1 when max_norm <= 0
//   ctl[2] found_inf: 1 when any ACTIVE element of g is inf or NaN (decided per element), else 0
//   ctl[3] reserved (0)
// which the scale kernel and the device-counted AdamW read on the device: nothing comes back to the host.
#include "reduce.h"
#include "ssl4gie_hip.h"

namespace {
DEVI int find_seg(const long long* __restrict__ seg_start, int S, long long i) {
    int lo = 0, hi = S;  // invariant: seg_start[lo] <= i < seg_start[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (seg_start[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}
// segment of element i for a whole 256-thread block: ONE binary search (thread 0), then every
// thread walks forward from there — a block's 1024 elements almost always lie in one or two segments
DEVI int block_seg(const long long* __restrict__ seg_start, int S, long long i, long long block_first) {
    __shared__ int s0;
    if (threadIdx.x == 0) s0 = find_seg(seg_start, S, block_first);
    __syncthreads();
    int s = s0;
    while (s + 1 < S && seg_start[s + 1] <= i) ++s;
    return s;
}
// the way into a streaming kernel over the elements [lo, n), 1024 per block: the thread's four elements start at i and
// lie in segment s (slices are 64-element aligned); false for a thread past n
DEVI bool elem_seg(const long long* __restrict__ seg_start, int S, long long lo, long long n, long long& i, int& s) {
    const long long first = lo + (long long)blockIdx.x * blockDim.x * 4;
    i = first + threadIdx.x * 4;
    s = block_seg(seg_start, S, i < n ? i : n - 4, first);
    return i < n;
}
}  // namespace

// torch.optim.AdamW (decoupled decay, bias-corrected): p *= 1 - lr wd; m, v moments;
// p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
// CTL: the gradient is ctl[1] * g, the step count of the bias corrections is *applied + 1 (a device
// counter of the updates really applied), and with `skip` nothing at all is written while ctl[2] is set
template <bool CTL>
__global__ __launch_bounds__(256) void adamw_arena_kernel(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
    const long long* __restrict__ seg_start, const float* __restrict__ seg_lr,
    const float* __restrict__ seg_wd, int S, float b1, float b2, float eps, float bc1, float rsqrt_bc2,
    long long n, bf16_t* __restrict__ lp, long long lo, const float* __restrict__ ctl,
    const int* __restrict__ applied, int skip) {
    __shared__ float bc[2];
    float coef = 1.f;
    if (CTL) {
        if (skip && ctl[2] != 0.f) return;  // uniform over the grid: GradScaler.step's skip
        coef = ctl[1];
        if (threadIdx.x == 0) {  // published by block_seg's barrier
            const float t = (float)(*applied + 1);
            bc[0] = 1.f - powf(b1, t);
            bc[1] = 1.f / sqrtf(1.f - powf(b2, t));
        }
    }
    long long i;
    int s;
    if (!elem_seg(seg_start, S, lo, n, i, s)) return;
    const float lr = seg_lr[s];
    if (lr < 0.f) return;
    if (CTL) { bc1 = bc[0]; rsqrt_bc2 = bc[1]; }
    const float wd = seg_wd[s];
    f32x4 pp = ld4(p + i), mm = ld4(m + i), vv = ld4(v + i);
    f32x4 gg = ld4(g + i);
    if (CTL) gg *= coef;
    const float step = lr / bc1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float x = pp[j] * (1.f - lr * wd);
        const float mj = b1 * mm[j] + (1.f - b1) * gg[j];
        const float vj = b2 * vv[j] + (1.f - b2) * gg[j] * gg[j];
        x -= step * mj / (sqrtf(vj) * rsqrt_bc2 + eps);
        pp[j] = x; mm[j] = mj; vv[j] = vj;
    }
    st4(p + i, pp);
    st4(m + i, mm);
    st4(v + i, vv);
    if (lp) st4(lp + i, pp);  // the bf16 operand copy of the updated weights, while they are in registers
}
// one thread: the update above was applied unless it was skipped
__global__ void adamw_advance_kernel(int* __restrict__ applied, const float* __restrict__ ctl, int skip) {
    if (!(skip && ctl[2] != 0.f)) *applied += 1;
}

// Gradient norm, stage 1: a FIXED grid; block b owns the contiguous elements [b, b + 1) * per_block
// (per_block = the arena split evenly, rounded up to 1024) and walks them 1024 at a time in order, so
// the summation tree depends on nothing but n: the result is bit-identical from run to run and from
// rank to rank.  Each thread keeps four fp32 sums (one per lane of its 16-byte load: per_block / 1024
// terms each, 54 for the 112 M elements of MAE ViT-B), everything from there on is fp64.  A block's
// elements lie in one or two segments: one binary search per thread, then a forward walk.  Inactive
// segments are not loaded at all.  Four trips are taken at a time — masks first, then the four loads
// back to back — so that four 16-byte loads per thread are in flight.
#define GN_BLOCKS 2048
__global__ __launch_bounds__(256) void grad_norm_partial_kernel(
    const float* __restrict__ g, const long long* __restrict__ seg_start,
    const float* __restrict__ seg_mask, int S, float inv_scale, long long n, long long per_block,
    double* __restrict__ part_sum, int* __restrict__ part_bad) {
    __shared__ double red[4];
    __shared__ int redb[4];
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    unsigned bad = 0;
    const long long lo = (long long)blockIdx.x * per_block;
    const long long hi = lo + per_block < n ? lo + per_block : n;
    long long i = lo + threadIdx.x * 4;
    if (i < hi) {
        int s = find_seg(seg_start, S, i);
        long long next = seg_start[s + 1];  // end of the current segment; the tables are read again
        bool active = seg_mask[s] >= 0.f;   // only when it is crossed
        for (; i < hi; i += 4096) {
            bool on[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long long k = i + u * 1024;
                on[u] = false;
                if (k < hi) {
                    while (k >= next && s + 1 < S) {  // (n = seg_start[S]: the bound only guards a wrong n)
                        ++s;
                        next = seg_start[s + 1];
                        active = seg_mask[s] >= 0.f;
                    }
                    on[u] = active;
                }
            }
            f32x4 gg[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                gg[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (on[u]) gg[u] = ld4(g + i + u * 1024);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    bad |= ((__float_as_uint(gg[u][j]) & 0x7f800000u) == 0x7f800000u);
                    const float x = inv_scale * gg[u][j];
                    acc[j] += x * x;
                }
        }
    }
    double a = ((double)acc[0] + (double)acc[1]) + ((double)acc[2] + (double)acc[3]);
#pragma unroll  // written out here and below: see reduce.h
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    const int wbad = __any((int)bad);
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = a; redb[threadIdx.x >> 6] = wbad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        part_sum[blockIdx.x] = block_get<SumOrder::Pairwise>(red);
        part_bad[blockIdx.x] = (redb[0] | redb[1] | redb[2] | redb[3]) != 0;
    }
}
// stage 2, one workgroup: the GN_BLOCKS partials in fp64 in a fixed tree, then the control block
__global__ __launch_bounds__(256) void grad_norm_final_kernel(
    const double* __restrict__ part_sum, const int* __restrict__ part_bad, float max_norm,
    float* __restrict__ ctl) {
    __shared__ double red[4];
    __shared__ int redb[4];
    double a = 0.0;
    int bad = 0;
    for (int k = threadIdx.x; k < GN_BLOCKS; k += 256) {
        a += part_sum[k];
        bad |= part_bad[k];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    bad = __any(bad);
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = a; redb[threadIdx.x >> 6] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(block_get<SumOrder::Pairwise>(red));
        float coef = 1.f;
        if (max_norm > 0.f) {  // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max=1)
            coef = max_norm / (norm + 1e-6f);
            coef = coef > 1.f ? 1.f : coef;  // a NaN norm stays a NaN coefficient, as torch's clamp leaves it
        }
        ctl[0] = norm;
        ctl[1] = coef;
        ctl[2] = (redb[0] | redb[1] | redb[2] | redb[3]) ? 1.f : 0.f;
        ctl[3] = 0.f;
    }
}
// g *= ctl[1] over the active segments; nothing is written when the coefficient is exactly 1
__global__ __launch_bounds__(256) void grad_scale_kernel(
    float* __restrict__ g, const long long* __restrict__ seg_start, const float* __restrict__ seg_mask,
    int S, const float* __restrict__ ctl, long long n) {
    const float coef = ctl[1];
    if (coef == 1.f) return;  // uniform over the grid
    long long i;
    int s;
    if (!elem_seg(seg_start, S, 0, n, i, s)) return;
    if (seg_mask[s] < 0.f) return;
    st4(g + i, ld4(g + i) * coef);
}

// LARS stage 1: partial[(s * parts + part) * 2 + {0, 1}] = sum p^2, sum (g + wd p)^2 over the part
#define LARS_PARTS 32
__global__ __launch_bounds__(256) void lars_norm_partial_kernel(
    const float* __restrict__ p, const float* __restrict__ g, const long long* __restrict__ seg_start,
    const float* __restrict__ seg_lr, const float* __restrict__ seg_wd, const float* __restrict__ seg_mat,
    float* __restrict__ partial) {
    __shared__ float red[2][4];
    const int s = blockIdx.y, part = blockIdx.x;
    float a = 0.f, b = 0.f;
    if (seg_lr[s] >= 0.f && seg_mat[s] != 0.f) {
        const long long lo = seg_start[s], hi = seg_start[s + 1];
        const float wd = seg_wd[s];
        for (long long i = lo + ((long long)part * 256 + threadIdx.x) * 4; i < hi; i += (long long)LARS_PARTS * 1024) {
            const f32x4 pp = ld4(p + i), gg = ld4(g + i);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float d = gg[j] + wd * pp[j];
                a += pp[j] * pp[j];
                b += d * d;
            }
        }
    }
    a = wave_sum(a);
    b = wave_sum(b);
    block_put(a, red[0]); block_put(b, red[1]);
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[((size_t)s * LARS_PARTS + part) * 2] = block_get<SumOrder::Sequential>(red[0]);
        partial[((size_t)s * LARS_PARTS + part) * 2 + 1] = block_get<SumOrder::Sequential>(red[1]);
    }
}
// stage 2: q[s] = trust |p| / |dp| where both norms are > 0, else 1 (matrices); 1 for vectors
__global__ void lars_trust_kernel(const float* __restrict__ partial, const float* __restrict__ seg_mat,
                                  float* __restrict__ q, float trust, int S) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    float a = 0.f, b = 0.f;
    for (int k = 0; k < LARS_PARTS; ++k) {
        a += partial[((size_t)s * LARS_PARTS + k) * 2];
        b += partial[((size_t)s * LARS_PARTS + k) * 2 + 1];
    }
    const float pn = sqrtf(a), un = sqrtf(b);
    q[s] = (seg_mat[s] != 0.f && pn > 0.f && un > 0.f) ? trust * pn / un : 1.f;
}
// stage 3: dp = (g + wd p) q (matrices) or g (vectors); mu = mom mu + dp; p -= lr mu
__global__ __launch_bounds__(256) void lars_apply_kernel(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ mu,
    const long long* __restrict__ seg_start, const float* __restrict__ seg_lr,
    const float* __restrict__ seg_wd, const float* __restrict__ seg_mat, const float* __restrict__ q,
    int S, float momentum, long long n) {
    long long i;
    int s;
    if (!elem_seg(seg_start, S, 0, n, i, s)) return;
    const float lr = seg_lr[s];
    if (lr < 0.f) return;
    const bool mat = seg_mat[s] != 0.f;
    const float wd = mat ? seg_wd[s] : 0.f, qq = mat ? q[s] : 1.f;
    f32x4 pp = ld4(p + i), mm = ld4(mu + i);
    const f32x4 gg = ld4(g + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float dp = (gg[j] + wd * pp[j]) * qq;
        mm[j] = momentum * mm[j] + dp;
        pp[j] -= lr * mm[j];
    }
    st4(p + i, pp);
    st4(mu + i, mm);
}
// torch.optim.SGD(momentum, weight_decay), dampening 0, no Nesterov (Models/moco_v3/main_lincls.py:236-238):
// d = g + wd p; buf = momentum buf + d; p -= lr buf
__global__ __launch_bounds__(256) void sgd_arena_kernel(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
    const long long* __restrict__ seg_start, const float* __restrict__ seg_lr,
    const float* __restrict__ seg_wd, int S, float momentum, long long n) {
    long long i;
    int s;
    if (!elem_seg(seg_start, S, 0, n, i, s)) return;
    const float lr = seg_lr[s];
    if (lr < 0.f) return;
    const float wd = seg_wd[s];
    f32x4 pp = ld4(p + i), bb = ld4(buf + i);
    const f32x4 gg = ld4(g + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float d = gg[j] + wd * pp[j];
        bb[j] = momentum * bb[j] + d;
        pp[j] -= lr * bb[j];
    }
    st4(p + i, pp);
    st4(buf + i, bb);
}

extern "C" int ssl4gie_adamw_arena(float* p, const float* g, float* m, float* v, const long long* seg_start,
                                   const float* seg_lr, const float* seg_wd, int S, float beta1, float beta2,
                                   float eps, int step, int* applied, long long lo, long long hi, void* lp_bf16,
                                   const float* ctl, int skip_nonfinite, int advance, void* stream) {
    REQUIRE(p && g && m && v && seg_start && seg_lr && seg_wd && S > 0 && lo >= 0 && hi >= lo && lo % 4 == 0 &&
            hi % 4 == 0);
    REQUIRE(ctl ? applied != nullptr : step > 0 && !applied && !skip_nonfinite && !advance);
    const dim3 grid((unsigned)(((hi - lo) / 4 + 255) / 256));
    bf16_t* lp = (bf16_t*)lp_bf16;
    if (!ctl) {  // host-counted: the bias corrections come from `step`
        if (hi == lo) return 0;
        const float bc1 = 1.f - powf(beta1, (float)step), bc2 = 1.f - powf(beta2, (float)step);
        hipLaunchKernelGGL(adamw_arena_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, p, g, m, v,
                           seg_start, seg_lr, seg_wd, S, beta1, beta2, eps, bc1, 1.f / sqrtf(bc2), hi, lp, lo,
                           (const float*)nullptr, (const int*)nullptr, 0);
        LAUNCH_CHECK();
        return 0;
    }
    if (hi > lo) {  // device-counted: the kernel derives them from *applied
        hipLaunchKernelGGL(adamw_arena_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, p, g, m, v,
                           seg_start, seg_lr, seg_wd, S, beta1, beta2, eps, 0.f, 0.f, hi, lp, lo, ctl,
                           (const int*)applied, skip_nonfinite != 0);
        LAUNCH_CHECK();
    }
    if (advance) {
        hipLaunchKernelGGL(adamw_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, applied, ctl,
                           skip_nonfinite != 0);
        LAUNCH_CHECK();
    }
    return 0;
}
extern "C" size_t ssl4gie_grad_norm_workspace_bytes(void) {
    return (size_t)GN_BLOCKS * (sizeof(double) + sizeof(int));
}
extern "C" int ssl4gie_grad_norm_arena(const float* g, const long long* seg_start, const float* seg_mask,
                                       int S, float inv_scale, float max_norm, void* workspace,
                                       float* ctl, long long n, void* stream) {
    REQUIRE(g && seg_start && seg_mask && S > 0 && workspace && ctl && n > 0 && n % 4 == 0 &&
            (uintptr_t)workspace % 8 == 0);
    double* part_sum = (double*)workspace;
    int* part_bad = (int*)(part_sum + GN_BLOCKS);
    const long long per_block = ((n + 1023) / 1024 + GN_BLOCKS - 1) / GN_BLOCKS * 1024;
    hipLaunchKernelGGL(grad_norm_partial_kernel, dim3(GN_BLOCKS), dim3(256), 0, (hipStream_t)stream, g,
                       seg_start, seg_mask, S, inv_scale, n, per_block, part_sum, part_bad);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream,
                       (const double*)part_sum, (const int*)part_bad, max_norm, ctl);
    LAUNCH_CHECK();
    return 0;
}
extern "C" int ssl4gie_grad_scale_arena(float* g, const long long* seg_start, const float* seg_mask, int S,
                                        const float* ctl, long long n, void* stream) {
    REQUIRE(g && seg_start && seg_mask && S > 0 && ctl && n > 0 && n % 4 == 0);
    hipLaunchKernelGGL(grad_scale_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, g, seg_start, seg_mask, S, ctl, n);
    LAUNCH_CHECK();
    return 0;
}
extern "C" size_t ssl4gie_lars_workspace_bytes(int S) {
    return ((size_t)S * LARS_PARTS * 2 + S) * sizeof(float);
}
extern "C" int ssl4gie_lars_arena(float* p, const float* g, float* mu, const long long* seg_start,
                                  const float* seg_lr, const float* seg_wd, const float* seg_mat, int S,
                                  float momentum, float trust, float* workspace, long long n,
                                  void* stream) {
    REQUIRE(p && g && mu && seg_start && seg_lr && seg_wd && seg_mat && workspace && S > 0 && S <= 65535 &&
            n >= 0 && n % 4 == 0);
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    float* partial = workspace;
    float* q = workspace + (size_t)S * LARS_PARTS * 2;
    hipLaunchKernelGGL(lars_norm_partial_kernel, dim3(LARS_PARTS, S), dim3(256), 0, st, p, g, seg_start,
                       seg_lr, seg_wd, seg_mat, partial);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(lars_trust_kernel, dim3((S + 255) / 256), dim3(256), 0, st, partial, seg_mat, q,
                       trust, S);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(lars_apply_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, st, p, g, mu,
                       seg_start, seg_lr, seg_wd, seg_mat, q, S, momentum, n);
    LAUNCH_CHECK();
    return 0;
}
extern "C" int ssl4gie_sgd_arena(float* p, const float* g, float* buf, const long long* seg_start, const float* seg_lr,
                                 const float* seg_wd, int S, float momentum, long long n, void* stream) {
    REQUIRE(p && g && buf && seg_start && seg_lr && seg_wd && S > 0 && n >= 0 && n % 4 == 0);
    REQUIRE(((uintptr_t)p | (uintptr_t)g | (uintptr_t)buf) % 16 == 0);
    if (n == 0) return 0;
    hipLaunchKernelGGL(sgd_arena_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p, g,
                       buf, seg_start, seg_lr, seg_wd, S, momentum, n);
    LAUNCH_CHECK();
    return 0;
}
