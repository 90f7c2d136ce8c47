// Evaluation metrics of the three finetune heads as device kernels: the `test()` loops and `eval_*.py` CLIs of the
// reference run them as torch ops with a host read-back per metric and image.
//
//  * Binary_segmentation/Metrics/performance.py:5-92 (DiceScore, IoU, Precision, Recall): the four classes threshold
//    the same two maps and differ only in the closing formula.  seg_counts_kernel counts |m1|, |m2|, |m1 & m2| per image
//    in one pass (the logits resampled on the fly where the target is stored at another size: eval_segmentation.py:36-37),
//    seg_scores_kernel evaluates the four formulas from the counts.
//  * Classification/Metrics/performance.py:4-56 (meanF1Score, meanPrecision, meanRecall): every term of the per-class
//    loops is an entry, a row sum or a column sum of the confusion matrix, which adds up over the batches of a loader
//    (train_classification.py:93-98 re-concatenates and re-scores all predictions at every batch instead).
//  * Depth_estimation/eval_depth.py:19-28, 43-61 (rmse, rel_err, abs_err after the scale-and-shift alignment, the resize
//    to the stored size, the centre crop, the clamp and the mask): depth_sums_kernel / depth_solve_kernel give the
//    alignment, depth_err_kernel evaluates the aligned, resampled, cropped prediction per stored pixel and never stores
//    it, and the median is an exact radix select (sel_hist_kernel / sel_pick_kernel) instead of a sort.
//
// Integer counts use LDS / global integer atomics (the result does not depend on their order); floating sums are
// per-block partials added in a fixed order in fp64.  No float atomics: every result is bit-identical from run to run.
// Products and sums are rounded one by one (no contraction into fused multiply-adds): the per-pixel values are the ones
// the separate torch ops give.
#include <type_traits>

#include "reduce.h"
#include "ssl4gie_hip.h"

#pragma clang fp contract(off)

// uint8 targets beside common.h's fp32 / bf16 element access
DEVI f32x4 ld4(const uint8_t* p) {
    const uint32_t r = *(const uint32_t*)p;
    return f32x4{(float)(r & 255u), (float)((r >> 8) & 255u), (float)((r >> 16) & 255u), (float)(r >> 24)};
}
template <> struct Elem<uint8_t> {
    static DEVI float ld(const uint8_t* p) { return (float)*p; }
};

namespace {

constexpr int MAXBLK = 256;    // blocks per image of the streaming kernels (one per CU)
constexpr int DEPTH_NB = 32;   // blocks per image of the alignment sums (the maps are the model's S x S outputs)
constexpr int SEL_BINS = 2048; // radix of the select: 11 + 11 + 10 bits
constexpr uint32_t SEL_SKIP = 0xFFFFFFFFu;  // bit pattern of a masked-out entry (a negative NaN: never a valid |d / t|)

typedef unsigned long long u64;

// F.interpolate(mode = "bilinear", align_corners = False): source taps and weight of output index `dst`
struct Tap { int i0, i1; float l1; };
DEVI Tap bilinear_tap(float scale, int dst, int in) {
    float s = scale * ((float)dst + 0.5f) - 0.5f;
    s = s < 0.f ? 0.f : s;
    int i0 = (int)s;
    i0 = i0 > in - 1 ? in - 1 : i0;
    Tap t;
    t.i0 = i0;
    t.i1 = i0 + (i0 < in - 1 ? 1 : 0);
    t.l1 = fminf(s - (float)i0, 1.f);
    return t;
}
DEVI float bilinear_mix(float a, float b, float c, float d, float lx, float ly) {
    return (1.f - ly) * ((1.f - lx) * a + lx * b) + ly * ((1.f - lx) * c + lx * d);
}

// ------------------------------------------------------------------ segmentation counts
// counts[b] += (|m1|, |m2|, |m1 & m2|), m1 = logit > thr (thr = 0 stands for sigmoid(logit) > 0.5), m2 = target > 0.5
template <typename LT, typename TT, bool RESIZE>
__global__ __launch_bounds__(256) void seg_counts_kernel(const LT* __restrict__ logits, const TT* __restrict__ target,
                                                         u64* __restrict__ counts, int Hin, int Win, int H, int W,
                                                         float thr, int vec) {
    const int b = blockIdx.y;
    const unsigned HW = (unsigned)H * (unsigned)W;
    const LT* l = logits + (size_t)b * Hin * Win;
    const TT* t = target + (size_t)b * HW;
    const unsigned step = gridDim.x * 256u;
    int c[3] = {0, 0, 0};
    if constexpr (!RESIZE) {
        if (vec) {  // HW % 4 == 0 and both bases aligned to four elements
            for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < HW / 4u; i += step) {
                const f32x4 x = ld4(l + 4u * (size_t)i), y = ld4(t + 4u * (size_t)i);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const bool m1 = x[e] > thr, m2 = y[e] > 0.5f;
                    c[0] += m1; c[1] += m2; c[2] += m1 && m2;
                }
            }
        } else {
            for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < HW; i += step) {
                const bool m1 = Elem<LT>::ld(l + i) > thr, m2 = Elem<TT>::ld(t + i) > 0.5f;
                c[0] += m1; c[1] += m2; c[2] += m1 && m2;
            }
        }
    } else {
        const float sy = (float)Hin / (float)H, sx = (float)Win / (float)W;
        for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < HW; i += step) {
            const unsigned y = i / (unsigned)W, x = i - y * (unsigned)W;
            const Tap ty = bilinear_tap(sy, (int)y, Hin), tx = bilinear_tap(sx, (int)x, Win);
            const LT* r0 = l + (size_t)ty.i0 * Win;
            const LT* r1 = l + (size_t)ty.i1 * Win;
            const float v = bilinear_mix(Elem<LT>::ld(r0 + tx.i0), Elem<LT>::ld(r0 + tx.i1), Elem<LT>::ld(r1 + tx.i0),
                                         Elem<LT>::ld(r1 + tx.i1), tx.l1, ty.l1);
            const bool m1 = v > thr, m2 = Elem<TT>::ld(t + i) > 0.5f;
            c[0] += m1; c[1] += m2; c[2] += m1 && m2;
        }
    }
    __shared__ int sh[4 * 3];
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = wave_sum(c[k]);
    block_put(c, sh);
    __syncthreads();
    if (threadIdx.x < 3) {  // thread k closes count k
        const int k = threadIdx.x;
        const int s = block_get<SumOrder::Sequential, 3>(sh, k);
        if (s) atomicAdd(counts + (size_t)b * 3 + k, (u64)s);  // integer: the order of arrival does not matter
    }
}

// the closing formulas of performance.py:21-26, :46-49, :69-70, :90-91 in fp32, in their operation order; the batch
// sum runs in fp64 in image order
__global__ __launch_bounds__(256) void seg_scores_kernel(const long long* __restrict__ counts, int B, float smooth,
                                                         float* __restrict__ scores, double* __restrict__ accum) {
    __shared__ double sh[4][256];
    double a[4] = {0, 0, 0, 0};
    for (int b = threadIdx.x; b < B; b += 256) {
        const long long m1 = counts[b * 3], m2 = counts[b * 3 + 1], in = counts[b * 3 + 2];
        const float num = (float)in + smooth;
        a[0] += (double)(2.0f * num / ((float)(m1 + m2) + smooth));
        a[1] += (double)(num / ((float)(m1 + m2 - in) + smooth));
        a[2] += (double)(num / ((float)m1 + smooth));
        a[3] += (double)(num / ((float)m2 + smooth));
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) sh[k][threadIdx.x] = a[k];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o)
#pragma unroll
            for (int k = 0; k < 4; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x < 4) {
        const int k = threadIdx.x;
        scores[k] = (float)sh[k][0] / (float)B;
        if (accum) accum[k] += sh[k][0];
    }
    if (threadIdx.x == 4 && accum) accum[4] += (double)B;
}

// ------------------------------------------------------------------ confusion matrix
// KIND 0 fp32 logits, 1 bf16 logits, 2 int64 predictions; conf[target][prediction]
template <int KIND>
__global__ __launch_bounds__(256) void confusion_kernel(const void* __restrict__ in,
                                                        const long long* __restrict__ target, u64* __restrict__ conf,
                                                        u64* __restrict__ rejected, int B, int C) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= B) return;
    long long p;
    if constexpr (KIND == 2) {
        p = ((const long long*)in)[row];
    } else {
        typedef typename std::conditional<KIND == 0, float, bf16_t>::type T;
        const T* x = (const T*)in + (size_t)row * C;
        float best = Elem<T>::ld(x);
        int arg = 0;
        for (int c = 1; c < C; ++c) {  // the first maximum; a NaN counts as the largest value, as torch.argmax has it
            const float v = Elem<T>::ld(x + c);
            if (v > best || (v != v && best == best)) { best = v; arg = c; }
        }
        p = arg;
    }
    const long long t = target[row];
    if (t >= 0 && t < C && p >= 0 && p < C)
        atomicAdd(conf + (size_t)t * C + (size_t)p, (u64)1);
    else
        atomicAdd(rejected, (u64)1);  // never an index
}

// per class i: tp = conf[i][i], |m1| = column sum (predicted i), |m2| = row sum (target i); the terms of
// Classification/Metrics/performance.py:17-21, :38, :55 in fp32, computed side by side (CS_CHUNK classes at a time),
// then added by one thread in class order in fp32 — `score = 0; score += term` of the reference's loops, so the means
// are the reference's bit for bit — and divided by n_class
constexpr int CS_CHUNK = 1024;
__global__ __launch_bounds__(256) void confusion_scores_kernel(const long long* __restrict__ conf, int C, float smooth,
                                                               float* __restrict__ scores) {
    __shared__ float term[3][CS_CHUNK];
    __shared__ long long shi[2][256];
    float run[3] = {0.f, 0.f, 0.f};  // thread 0's running sums
    long long diag = 0, total = 0;
    for (int c0 = 0; c0 < C; c0 += CS_CHUNK) {
        const int nc = C - c0 < CS_CHUNK ? C - c0 : CS_CHUNK;
        for (int u = threadIdx.x; u < nc; u += 256) {
            const int i = c0 + u;
            long long m1 = 0, m2 = 0;
            for (int j = 0; j < C; ++j) {
                m1 += conf[(size_t)j * C + i];
                m2 += conf[(size_t)i * C + j];
            }
            const long long tp = conf[(size_t)i * C + i];
            const float num = (float)tp + smooth;
            term[0][u] = 2.0f * num / ((float)(m1 + m2) + smooth);
            term[1][u] = num / ((float)m1 + smooth);
            term[2][u] = num / ((float)m2 + smooth);
            diag += tp;
            total += m2;
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int u = 0; u < nc; ++u) { run[0] += term[0][u]; run[1] += term[1][u]; run[2] += term[2][u]; }
        __syncthreads();
    }
    shi[0][threadIdx.x] = diag;
    shi[1][threadIdx.x] = total;
    block_tree_sum(shi, threadIdx.x);
    if (threadIdx.x == 0) {
        scores[0] = run[0] / (float)C;
        scores[1] = run[1] / (float)C;
        scores[2] = run[2] / (float)C;
        scores[3] = (float)shi[0][0] / (float)shi[1][0];  // no sample at all: 0 / 0 = NaN
    }
}

// ------------------------------------------------------------------ exact rank select on non-negative fp32
// The bit pattern of a non-negative float is monotone in its value.  Three histogram passes over the digits
// [31:21], [20:10], [9:0]; after each, sel_pick_kernel finds the bin that holds the wanted rank and narrows the prefix.
struct SelState { u64 rank; uint32_t prefix, pad; };
DEVI int sel_digit_shift(int pass) { return pass == 0 ? 21 : (pass == 1 ? 10 : 0); }

__global__ __launch_bounds__(256) void sel_hist_kernel(const float* __restrict__ vals, long long n, long long stride,
                                                       const SelState* __restrict__ st, u64* __restrict__ hist,
                                                       int pass, int skip) {
    __shared__ unsigned h[SEL_BINS];
    const int b = blockIdx.y;
    for (int j = threadIdx.x; j < SEL_BINS; j += 256) h[j] = 0u;
    __syncthreads();
    const uint32_t* v = (const uint32_t*)(vals + (size_t)b * stride);
    const uint32_t prefix = pass ? st[b].prefix : 0u;
    const int hs = pass == 1 ? 21 : 10, ds = sel_digit_shift(pass);
    const uint32_t mask = pass == 2 ? 0x3FFu : 0x7FFu;
    auto add = [&](uint32_t key) {
        if (skip && key == SEL_SKIP) return;
        if (pass && (key >> hs) != (prefix >> hs)) return;
        atomicAdd(&h[(key >> ds) & mask], 1u);
    };
    const long long step = (long long)gridDim.x * 256;
    long long done = 0;
    if (((uintptr_t)v & 15) == 0) {
        const long long n4 = n >> 2;
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += step) {
            const u32x4 k = *(const u32x4*)(v + 4 * i);
            add(k[0]); add(k[1]); add(k[2]); add(k[3]);
        }
        done = n4 << 2;
    }
    for (long long i = done + (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += step) add(v[i]);
    __syncthreads();
    for (int j = threadIdx.x; j < SEL_BINS; j += 256)
        if (h[j]) atomicAdd(hist + (size_t)b * SEL_BINS + j, (u64)h[j]);
}

// one block per array: rank k = (count - 1) / 2 in the first pass (torch.median's lower median), the rank inside the
// chosen bin afterwards.  Leaves the histogram zeroed for the next pass.  The last pass writes the value: NaN for an
// empty array (and for a count that its entries do not bear out).
__global__ __launch_bounds__(256) void sel_pick_kernel(SelState* __restrict__ st, u64* __restrict__ hist,
                                                       const long long* __restrict__ count_dev, long long n, int pass,
                                                       float* __restrict__ out, long long out_stride) {
    __shared__ u64 part[256];
    __shared__ int found;
    const int b = blockIdx.x, t = threadIdx.x;
    u64* H = hist + (size_t)b * SEL_BINS;
    const long long cnt = count_dev ? count_dev[b] : n;
    const u64 k = pass == 0 ? (cnt > 0 ? (u64)((cnt - 1) / 2) : 0) : st[b].rank;
    const uint32_t prefix = pass ? st[b].prefix : 0u;
    constexpr int PER = SEL_BINS / 256;
    u64 loc[PER], s = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) { loc[j] = H[t * PER + j]; s += loc[j]; }
    part[t] = s;
    if (t == 0) found = 0;
    __syncthreads();
    u64 before = 0;
    for (int j = 0; j < t; ++j) before += part[j];
    if (cnt > 0 && k >= before && k < before + s) {  // at most one thread
        int bin = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            if (k >= before + loc[j]) { before += loc[j]; ++bin; } else break;
        }
        const uint32_t np = prefix | ((uint32_t)(t * PER + bin) << sel_digit_shift(pass));
        st[b].prefix = np;
        st[b].rank = k - before;
        found = 1;
        if (pass == 2) out[(size_t)b * out_stride] = __uint_as_float(np);
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) H[t * PER + j] = 0;
    __syncthreads();
    if (pass == 2 && t == 0 && !found) out[(size_t)b * out_stride] = NAN;
}

__global__ void nan_kernel(float* out) { *out = NAN; }

__host__ __device__ inline size_t sel_bytes(int B) { return (size_t)B * (sizeof(SelState) + SEL_BINS * sizeof(u64)); }

// vals [B] arrays of n entries `stride` apart; sel = sel_bytes(B) of ZEROED workspace; out[b * out_stride]
void sel_launch(const float* vals, long long n, long long stride, int B, const long long* count_dev, int skip, void* sel,
                float* out, long long out_stride, hipStream_t st) {
    SelState* state = (SelState*)sel;
    u64* hist = (u64*)(state + B);
    long long nb = (n + 4095) / 4096;  // 16 entries per thread
    nb = nb > MAXBLK ? MAXBLK : (nb < 1 ? 1 : nb);
    for (int pass = 0; pass < 3; ++pass) {
        hipLaunchKernelGGL(sel_hist_kernel, dim3((unsigned)nb, B), dim3(256), 0, st, vals, n, stride,
                           (const SelState*)state, hist, pass, skip);
        hipLaunchKernelGGL(sel_pick_kernel, dim3(B), dim3(256), 0, st, state, hist, count_dev, n, pass, out, out_stride);
    }
}

// ------------------------------------------------------------------ depth errors
// workspace (8-byte units first): partA double [B][DEPTH_NB][5] | sol double [B][2] | partE double [B][MAXBLK][2] |
// cntE int64 [B][MAXBLK] | cnt int64 [B] (+ 1 for an odd B: what follows is 16-byte aligned) | select state +
// histograms | rel float [B][H * W]
struct DepthWs {
    double *partA, *sol, *partE;
    long long *cntE, *cnt;
    void* sel;
    float* rel;
};
__host__ __device__ inline DepthWs depth_ws(void* ws, int B, long long HW) {
    DepthWs w;
    w.partA = (double*)ws;
    w.sol = w.partA + (size_t)B * DEPTH_NB * 5;
    w.partE = w.sol + (size_t)B * 2;
    w.cntE = (long long*)(w.partE + (size_t)B * MAXBLK * 2);
    w.cnt = w.cntE + (size_t)B * MAXBLK;
    w.sel = (void*)(w.cnt + B + (B & 1));
    w.rel = (float*)((char*)w.sel + sel_bytes(B));
    return w;
}
size_t depth_rel_offset(int B) {
    return ((size_t)B * (DEPTH_NB * 5 + 2 + MAXBLK * 2 + MAXBLK + 1) + (size_t)(B & 1)) * 8 + sel_bytes(B);
}

// the five masked sums of compute_scale_and_shift (Depth_estimation/Metrics/losses.py:7-13) over target > 0, in fp64
__global__ __launch_bounds__(256) void depth_sums_kernel(const float* __restrict__ pred,
                                                         const float* __restrict__ target, double* __restrict__ partA,
                                                         int n) {
    const int b = blockIdx.y;
    const float* p = pred + (size_t)b * n;
    const float* t = target + (size_t)b * n;
    double v[5] = {0, 0, 0, 0, 0};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += DEPTH_NB * 256) {
        const float tf = t[i];
        if (tf > 0.f) {
            const double pv = (double)p[i], tv = (double)tf;
            v[0] += pv * pv; v[1] += pv; v[2] += 1.0; v[3] += pv * tv; v[4] += tv;
        }
    }
    __shared__ double sh[4 * 5];
    block_sum<SumOrder::Pairwise>(v, sh);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < 5; ++k) partA[((size_t)b * DEPTH_NB + blockIdx.x) * 5 + k] = v[k];
}
// thread b: the 2 x 2 solve of losses.py:19-23 in fp64; det == 0 leaves scale = shift = 0
__global__ void depth_solve_kernel(const double* __restrict__ partA, double* __restrict__ sol, int B) {
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        double s[5] = {0, 0, 0, 0, 0};
        for (int j = 0; j < DEPTH_NB; ++j)
            for (int k = 0; k < 5; ++k) s[k] += partA[((size_t)b * DEPTH_NB + j) * 5 + k];
        const double a00 = s[0], a01 = s[1], a11 = s[2], b0 = s[3], b1 = s[4];
        const double det = a00 * a11 - a01 * a01;
        double sc = 0.0, shf = 0.0;
        if (det != 0.0) {
            sc = (a11 * b0 - a01 * b1) / det;
            shf = (-a01 * b0 + a00 * b1) / det;
        }
        sol[b * 2] = sc;
        sol[b * 2 + 1] = shf;
    }
}

// one pass over the stored H x W pixels (eval_depth.py:44-58): the aligned prediction, resampled to max(H, W)^2, centre
// cropped at (top, left), clamped to [0, 1], zeroed where target_og == 0; both sides times scale_.  Block partials of
// sum d^2, sum |d| and the valid count; |d / t| of a valid pixel, SEL_SKIP's pattern of any other, to rel.
__global__ __launch_bounds__(256) void depth_err_kernel(const float* __restrict__ pred,
                                                        const float* __restrict__ target_og, void* __restrict__ ws,
                                                        int B, int S, int H, int W, int M, int top, int left,
                                                        float scale_) {
    const int b = blockIdx.y;
    const unsigned HW = (unsigned)H * (unsigned)W;
    const DepthWs w = depth_ws(ws, B, HW);
    const float* p = pred + (size_t)b * S * S;
    const float* tg = target_og + (size_t)b * HW;
    uint32_t* rel = (uint32_t*)(w.rel + (size_t)b * HW);
    const float sc = (float)w.sol[b * 2], shf = (float)w.sol[b * 2 + 1];
    const float rs = (float)S / (float)M;
    double v[2] = {0, 0};
    int cnt = 0;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < HW; i += gridDim.x * 256u) {
        const unsigned y = i / (unsigned)W, x = i - y * (unsigned)W;
        const float t0 = tg[i];
        uint32_t r = SEL_SKIP;
        const float t = t0 * scale_;
        if (t > 0.f) {
            const Tap ty = bilinear_tap(rs, (int)y + top, S), tx = bilinear_tap(rs, (int)x + left, S);
            const float* r0 = p + (size_t)ty.i0 * S;
            const float* r1 = p + (size_t)ty.i1 * S;
            float o = bilinear_mix(sc * r0[tx.i0] + shf, sc * r0[tx.i1] + shf, sc * r1[tx.i0] + shf,
                                   sc * r1[tx.i1] + shf, tx.l1, ty.l1);
            o = o < 0.f ? 0.f : o;   // the reference's two masked assignments: a NaN stays a NaN
            o = o > 1.f ? 1.f : o;
            if (t0 == 0.f) o = 0.f;  // t > 0 with t0 == 0 cannot happen; kept as the reference orders it
            const float d = o * scale_ - t;
            v[0] += (double)(d * d);
            v[1] += (double)fabsf(d);
            ++cnt;
            r = __float_as_uint(fabsf(d / t));
        }
        rel[i] = r;
    }
    __shared__ double sh[4 * 2];
    __shared__ int shc[4];
    block_sum<SumOrder::Pairwise>(v, sh);
    block_put(wave_sum(cnt), shc);
    __syncthreads();
    if (threadIdx.x == 0) {
        const size_t o = (size_t)b * MAXBLK + blockIdx.x;
        w.partE[o * 2] = v[0];
        w.partE[o * 2 + 1] = v[1];
        w.cntE[o] = (long long)shc[0] + shc[1] + shc[2] + shc[3];
    }
}
// thread b: the partials of image b in block order; out[b] = (sqrt(mean d^2), ., mean |d|), NaN without a valid pixel
__global__ void depth_tot_kernel(void* __restrict__ ws, float* __restrict__ out, int B, long long HW, int nblk) {
    const DepthWs w = depth_ws(ws, B, HW);
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        double s2 = 0.0, s1 = 0.0;
        long long c = 0;
        for (int j = 0; j < nblk; ++j) {
            const size_t o = (size_t)b * MAXBLK + j;
            s2 += w.partE[o * 2]; s1 += w.partE[o * 2 + 1]; c += w.cntE[o];
        }
        w.cnt[b] = c;
        out[b * 3] = c > 0 ? (float)sqrt(s2 / (double)c) : NAN;
        out[b * 3 + 2] = c > 0 ? (float)(s1 / (double)c) : NAN;
    }
}

int stream_blocks(long long n) {
    long long nb = (n + 1023) / 1024;  // four entries per thread
    return (int)(nb > MAXBLK ? MAXBLK : (nb < 1 ? 1 : nb));
}
// torchvision's centre-crop offset int(round((M - h) / 2.0)): Python rounds a half to the even neighbour
int crop_offset(int M, int h) {
    const int d = M - h, k = d / 2;
    return (d & 1) ? k + (k & 1) : k;
}

template <typename LT, typename TT>
void seg_launch(const void* logits, const void* target, u64* counts, int B, int Hin, int Win, int H, int W, float thr,
                hipStream_t st) {
    const long long HW = (long long)H * W;
    const dim3 grid(stream_blocks(HW), B);
    if (Hin == H && Win == W) {
        const int vec = (HW & 3) == 0 && ((uintptr_t)logits & (4 * sizeof(LT) - 1)) == 0 &&
                        ((uintptr_t)target & (4 * sizeof(TT) - 1)) == 0;
        hipLaunchKernelGGL((seg_counts_kernel<LT, TT, false>), grid, dim3(256), 0, st, (const LT*)logits,
                           (const TT*)target, counts, Hin, Win, H, W, thr, vec);
    } else {
        hipLaunchKernelGGL((seg_counts_kernel<LT, TT, true>), grid, dim3(256), 0, st, (const LT*)logits,
                           (const TT*)target, counts, Hin, Win, H, W, thr, 0);
    }
}

}  // namespace

extern "C" int ssl4gie_seg_counts(const void* logits, int logits_dtype, const void* target, int target_dtype,
                                  long long* counts, int B, int Hin, int Win, int H, int W, int sigmoid, void* stream) {
    REQUIRE(logits && target && counts && B > 0 && B <= 65535 && Hin > 0 && Win > 0 && H > 0 && W > 0);
    REQUIRE(logits_dtype == SSL4GIE_F32 || logits_dtype == SSL4GIE_BF16);
    REQUIRE(target_dtype == SSL4GIE_TGT_U8 || target_dtype == SSL4GIE_TGT_F32);
    REQUIRE((long long)H * W <= 0x7fffffffLL && (long long)Hin * Win <= 0x7fffffffLL);
    hipStream_t st = (hipStream_t)stream;
    HIP_RET(hipMemsetAsync(counts, 0, (size_t)B * 3 * sizeof(long long), st));
    const float thr = sigmoid ? 0.f : 0.5f;
    u64* c = (u64*)counts;
    const bool f = logits_dtype == SSL4GIE_F32, u8 = target_dtype == SSL4GIE_TGT_U8;
    if (f && u8) seg_launch<float, uint8_t>(logits, target, c, B, Hin, Win, H, W, thr, st);
    else if (f) seg_launch<float, float>(logits, target, c, B, Hin, Win, H, W, thr, st);
    else if (u8) seg_launch<bf16_t, uint8_t>(logits, target, c, B, Hin, Win, H, W, thr, st);
    else seg_launch<bf16_t, float>(logits, target, c, B, Hin, Win, H, W, thr, st);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int ssl4gie_seg_scores(const long long* counts, int B, float smooth, float* scores, double* accum,
                                  void* stream) {
    REQUIRE(counts && scores && B > 0);
    hipLaunchKernelGGL(seg_scores_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, counts, B, smooth, scores, accum);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int ssl4gie_confusion_update(const void* input, int input_kind, const long long* target, long long* conf,
                                        long long* rejected, int B, int C, void* stream) {
    REQUIRE(input && target && conf && rejected && B > 0 && C > 0 && C <= 46340);
    REQUIRE(input_kind == SSL4GIE_F32 || input_kind == SSL4GIE_BF16 || input_kind == SSL4GIE_PRED_I64);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((B + 255) / 256));
    if (input_kind == SSL4GIE_F32)
        hipLaunchKernelGGL(confusion_kernel<0>, grid, dim3(256), 0, st, input, target, (u64*)conf, (u64*)rejected, B, C);
    else if (input_kind == SSL4GIE_BF16)
        hipLaunchKernelGGL(confusion_kernel<1>, grid, dim3(256), 0, st, input, target, (u64*)conf, (u64*)rejected, B, C);
    else
        hipLaunchKernelGGL(confusion_kernel<2>, grid, dim3(256), 0, st, input, target, (u64*)conf, (u64*)rejected, B, C);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int ssl4gie_confusion_scores(const long long* conf, int C, float smooth, float* scores, void* stream) {
    REQUIRE(conf && scores && C > 0 && C <= 46340);
    hipLaunchKernelGGL(confusion_scores_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, conf, C, smooth, scores);
    LAUNCH_CHECK();
    return 0;
}

extern "C" size_t ssl4gie_lower_median_workspace_bytes(void) { return sel_bytes(1); }

extern "C" int ssl4gie_lower_median_f32(const float* x, long long n, float* out, void* workspace, void* stream) {
    REQUIRE(out && n >= 0 && (n == 0 || (x && workspace)));
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        hipLaunchKernelGGL(nan_kernel, dim3(1), dim3(1), 0, st, out);
    } else {
        HIP_RET(hipMemsetAsync(workspace, 0, sel_bytes(1), st));
        sel_launch(x, n, 0, 1, nullptr, 0, workspace, out, 0, st);
    }
    LAUNCH_CHECK();
    return 0;
}

extern "C" size_t ssl4gie_depth_eval_workspace_bytes(int B, int S, int H, int W) {
    if (B <= 0 || S <= 0 || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL) return 0;
    return depth_rel_offset(B) + (size_t)B * H * W * sizeof(float);
}

extern "C" int ssl4gie_depth_eval(const float* pred, const float* target, const float* target_og, float* out, int B,
                                  int Sh, int Sw, int H, int W, float scale_, void* workspace, void* stream) {
    REQUIRE(pred && target && target_og && out && workspace);
    REQUIRE(B > 0 && B <= 65535 && Sh > 0 && Sw > 0 && H > 0 && W > 0 && Sh == Sw);
    REQUIRE((long long)H * W <= 0x7fffffffLL && (long long)Sh * Sw <= 0x7fffffffLL);
    REQUIRE(((uintptr_t)workspace & 15) == 0);
    hipStream_t st = (hipStream_t)stream;
    const int S = Sh, M = H > W ? H : W;
    const long long HW = (long long)H * W;
    const DepthWs w = depth_ws(workspace, B, HW);
    HIP_RET(hipMemsetAsync(w.sel, 0, sel_bytes(B), st));
    hipLaunchKernelGGL(depth_sums_kernel, dim3(DEPTH_NB, B), dim3(256), 0, st, pred, target, w.partA, S * S);
    hipLaunchKernelGGL(depth_solve_kernel, dim3(1), dim3(256), 0, st, (const double*)w.partA, w.sol, B);
    const int nblk = stream_blocks(HW);
    hipLaunchKernelGGL(depth_err_kernel, dim3(nblk, B), dim3(256), 0, st, pred, target_og, workspace, B, S, H, W, M,
                       crop_offset(M, H), crop_offset(M, W), scale_);
    hipLaunchKernelGGL(depth_tot_kernel, dim3(1), dim3(256), 0, st, workspace, out, B, HW, nblk);
    sel_launch(w.rel, HW, HW, B, w.cnt, 1, w.sel, out + 1, 3, st);
    LAUNCH_CHECK();
    return 0;
}
