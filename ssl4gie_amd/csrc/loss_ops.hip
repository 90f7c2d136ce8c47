// Finetune losses as device kernels: value AND gradient w.r.t. the prediction in
// three passes over the map instead of the ~100 small elementwise / reduction launches of the
// host-side torch formulation (which stays available and is the parity reference).
//
//  * ScaleAndShiftInvariantLoss (Depth_estimation/Metrics/losses.py:120-146): per image the closed-form
//    2x2 least squares (scale s, shift h) on the valid pixels m = target > 0 (:5-25), masked MSE /
//    (2 sum M) (:51-57, batch-based reduction :28-38) + alpha x sum over 4 scales of the masked
//    gradient L1 on the subsampled grids (:60-77, :104-117).
//      pass A  per image sums a00 = sum m p^2, a01 = sum m p, a11 = sum m, b0 = sum m p t, b1 = sum m t
//              and the mask counts of the subsampled grids; -> s, h, batch totals M_k
//      pass B  g = dL/d(ssi) per pixel (MSE part + sign terms of the up to 4 x 4 neighbour pairs),
//              loss partials, per image G0 = sum g, G1 = sum g p
//      pass C  dL/dp = g s + G1 ds/dp + G0 dh/dp   (s and h depend on every pixel of the image)
//    Two-stage deterministic reductions (block partials, then one block per image / per batch).
//  * SoftDiceLoss (Binary_segmentation/Metrics/losses.py:5-24): per image sums of sigmoid(l) t,
//    sigmoid(l)^2, t^2; loss = 1 - mean score; gradient in a second pass.
#include "reduce.h"
#include "internal.h"
#include "ssl4gie_hip.h"

namespace {

constexpr int NB = 32;      // blocks per image
constexpr int NSUM_A = 8;   // a00 a01 a11 b0 b1 M1 M2 M3
constexpr int NSUM_B = 7;   // mse reg0 reg1 reg2 reg3 G0 G1

// layout of the fp32 workspace (floats): partA [B][NB][8] | img [B][12] | tot [8] | partB [B][NB][7] | g [B*H*W]
struct SsiWs {
    float *partA, *img, *tot, *partB, *g;
};
DEVI SsiWs ssi_ws(float* ws, int B, long long HW) {
    SsiWs w;
    w.partA = ws;
    w.img = w.partA + (size_t)B * NB * NSUM_A;
    w.tot = w.img + (size_t)B * 12;
    w.partB = w.tot + 8;
    w.g = w.partB + (size_t)B * NB * NSUM_B;
    return w;
}

__global__ __launch_bounds__(256) void ssi_sums_kernel(const float* __restrict__ pred,
                                                       const float* __restrict__ target, float* __restrict__ ws,
                                                       int B, int H, int W) {
    const int b = blockIdx.y;
    const long long HW = (long long)H * W;
    const float* p = pred + (size_t)b * HW;
    const float* t = target + (size_t)b * HW;
    float v[NSUM_A] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < HW; i += (long long)NB * 256) {
        const float tv = t[i], pv = p[i];
        if (tv > 0.f) {
            v[0] += pv * pv; v[1] += pv; v[2] += 1.f; v[3] += pv * tv; v[4] += tv;
            const int y = (int)(i / W), x = (int)(i % W);
            if (!((y | x) & 1)) v[5] += 1.f;
            if (!((y | x) & 3)) v[6] += 1.f;
            if (!((y | x) & 7)) v[7] += 1.f;
        }
    }
    __shared__ float sh[4 * NSUM_A];
    block_sum<SumOrder::Sequential>(v, sh);
    if (threadIdx.x == 0) {
        float* o = ssi_ws(ws, B, HW).partA + ((size_t)b * NB + blockIdx.x) * NSUM_A;
#pragma unroll
        for (int k = 0; k < NSUM_A; ++k) o[k] = v[k];
    }
}

// one block; thread b finishes image b (NB partials in a fixed order), then thread 0 the batch totals
__global__ void ssi_finalize_a_kernel(float* __restrict__ ws, int B, long long HW) {
    const SsiWs w = ssi_ws(ws, B, HW);
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        float s[NSUM_A] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int j = 0; j < NB; ++j)
            for (int k = 0; k < NSUM_A; ++k) s[k] += w.partA[((size_t)b * NB + j) * NSUM_A + k];
        const float a00 = s[0], a01 = s[1], a11 = s[2], b0 = s[3], b1 = s[4];
        const float det = a00 * a11 - a01 * a01;
        float sc = 0.f, shf = 0.f;
        if (det != 0.f) {  // losses.py:18-23: images with a singular system keep scale = shift = 0
            sc = (a11 * b0 - a01 * b1) / det;
            shf = (-a01 * b0 + a00 * b1) / det;
        }
        float* o = w.img + (size_t)b * 12;
        o[0] = a00; o[1] = a01; o[2] = a11; o[3] = b0; o[4] = b1; o[5] = det; o[6] = sc; o[7] = shf;
        o[8] = s[5]; o[9] = s[6]; o[10] = s[7]; o[11] = 0.f;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float m[4] = {0, 0, 0, 0};
        for (int b = 0; b < B; ++b) {
            const float* o = w.img + (size_t)b * 12;
            m[0] += o[2]; m[1] += o[8]; m[2] += o[9]; m[3] += o[10];
        }
        for (int k = 0; k < 4; ++k) w.tot[k] = m[k];
    }
}

DEVI float sgn(float x) { return (x > 0.f) ? 1.f : ((x < 0.f) ? -1.f : 0.f); }

__global__ __launch_bounds__(256) void ssi_grad_kernel(const float* __restrict__ pred,
                                                       const float* __restrict__ target, float* __restrict__ ws,
                                                       int B, int H, int W, float alpha, int scales) {
    const int b = blockIdx.y;
    const long long HW = (long long)H * W;
    const SsiWs w = ssi_ws(ws, B, HW);
    const float* p = pred + (size_t)b * HW;
    const float* t = target + (size_t)b * HW;
    const float sc = w.img[(size_t)b * 12 + 6], shf = w.img[(size_t)b * 12 + 7];
    float inv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) inv[k] = w.tot[k] > 0.f ? 1.f / w.tot[k] : 0.f;
    auto D = [&](int y, int x, float& m) -> float {  // mask * (ssi - target) at (y, x)
        const long long i = (long long)y * W + x;
        const float tv = t[i];
        m = tv > 0.f ? 1.f : 0.f;
        return m * (sc * p[i] + shf - tv);
    };
    float v[NSUM_B] = {0, 0, 0, 0, 0, 0, 0};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < HW; i += (long long)NB * 256) {
        const int y = (int)(i / W), x = (int)(i % W);
        float m;
        const float d = D(y, x, m);
        float g = d * inv[0];          // d/dssi of sum m (ssi - t)^2 / (2 sum M)
        v[0] += d * d;
        if (alpha > 0.f && m > 0.f) {
            for (int k = 0; k < scales && k < 4; ++k) {
                const int s = 1 << k;
                if ((y | x) & (s - 1)) break;  // not on this (or any coarser) grid
                float acc = 0.f, m2;
                if (x + s < W) { const float e = D(y, x + s, m2) - d; v[1 + k] += fabsf(e) * m2; acc -= sgn(e) * m2; }
                if (y + s < H) { const float e = D(y + s, x, m2) - d; v[1 + k] += fabsf(e) * m2; acc -= sgn(e) * m2; }
                if (x - s >= 0) { const float e = d - D(y, x - s, m2); acc += sgn(e) * m2; }
                if (y - s >= 0) { const float e = d - D(y - s, x, m2); acc += sgn(e) * m2; }
                g += alpha * inv[k] * acc;
            }
        }
        w.g[(size_t)b * HW + i] = g;
        v[5] += g;
        v[6] += g * p[i];
    }
    __shared__ float sh[4 * NSUM_B];
    block_sum<SumOrder::Sequential>(v, sh);
    if (threadIdx.x == 0) {
        float* o = w.partB + ((size_t)b * NB + blockIdx.x) * NSUM_B;
#pragma unroll
        for (int k = 0; k < NSUM_B; ++k) o[k] = v[k];
    }
}

__global__ void ssi_finalize_b_kernel(float* __restrict__ ws, float* __restrict__ loss, int B, long long HW,
                                      float alpha, int scales) {
    const SsiWs w = ssi_ws(ws, B, HW);
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        float s[NSUM_B] = {0, 0, 0, 0, 0, 0, 0};
        for (int j = 0; j < NB; ++j)
            for (int k = 0; k < NSUM_B; ++k) s[k] += w.partB[((size_t)b * NB + j) * NSUM_B + k];
        float* o = w.partB + (size_t)b * NB * NSUM_B;  // image totals overwrite the image's first partial
        for (int k = 0; k < NSUM_B; ++k) o[k] = s[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float tot[5] = {0, 0, 0, 0, 0};
        for (int b = 0; b < B; ++b)
            for (int k = 0; k < 5; ++k) tot[k] += w.partB[(size_t)b * NB * NSUM_B + k];
        float l = w.tot[0] > 0.f ? tot[0] / (2.f * w.tot[0]) : 0.f;
        if (alpha > 0.f)
            for (int k = 0; k < scales && k < 4; ++k)
                if (w.tot[k] > 0.f) l += alpha * tot[1 + k] / w.tot[k];
        *loss = l;
    }
}

__global__ __launch_bounds__(256) void ssi_apply_kernel(const float* __restrict__ pred,
                                                        const float* __restrict__ target,
                                                        const float* __restrict__ ws_c, float* __restrict__ dpred,
                                                        int B, long long HW) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)B * HW) return;
    const int b = (int)(idx / HW);
    const SsiWs w = ssi_ws(const_cast<float*>(ws_c), B, HW);
    const float* o = w.img + (size_t)b * 12;
    const float a00 = o[0], a01 = o[1], a11 = o[2], b0 = o[3], b1 = o[4], det = o[5], sc = o[6], shf = o[7];
    const float G0 = w.partB[(size_t)b * NB * NSUM_B + 5], G1 = w.partB[(size_t)b * NB * NSUM_B + 6];
    const float pv = pred[idx], tv = target[idx];
    float d = w.g[idx] * sc;
    if (tv > 0.f && det != 0.f) {
        const float dd = 2.f * a11 * pv - 2.f * a01;  // d det / d p
        const float ds = (a11 * tv - b1 - sc * dd) / det;
        const float dh = (-b0 - a01 * tv + 2.f * pv * b1 - shf * dd) / det;
        d += G1 * ds + G0 * dh;
    }
    (void)a00;
    dpred[idx] = d;
}

// ------------------------------------------------------------------ soft Dice
__global__ __launch_bounds__(256) void dice_sums_kernel(const float* __restrict__ logits,
                                                        const float* __restrict__ target, float* __restrict__ ws,
                                                        long long n) {
    const int b = blockIdx.y;
    const float* l = logits + (size_t)b * n;
    const float* t = target + (size_t)b * n;
    float v[3] = {0, 0, 0};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)NB * 256) {
        const float m1 = 1.f / (1.f + __expf(-l[i])), m2 = t[i];
        v[0] += m1 * m2; v[1] += m1 * m1; v[2] += m2 * m2;
    }
    __shared__ float sh[4 * 3];
    block_sum<SumOrder::Sequential>(v, sh);
    if (threadIdx.x == 0)
        for (int k = 0; k < 3; ++k) ws[((size_t)b * NB + blockIdx.x) * 3 + k] = v[k];
}
__global__ void dice_finalize_kernel(float* __restrict__ ws, float* __restrict__ loss, int B, float smooth) {
    float* img = ws + (size_t)B * NB * 3;  // [B][3]: inter, den, score
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        float s[3] = {0, 0, 0};
        for (int j = 0; j < NB; ++j)
            for (int k = 0; k < 3; ++k) s[k] += ws[((size_t)b * NB + j) * 3 + k];
        const float num = s[0] + smooth, den = s[1] + s[2] + smooth;
        img[b * 3] = num; img[b * 3 + 1] = den; img[b * 3 + 2] = 2.f * num / den;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float sum = 0.f;
        for (int b = 0; b < B; ++b) sum += img[b * 3 + 2];
        *loss = 1.f - sum / (float)B;
    }
}
__global__ __launch_bounds__(256) void dice_apply_kernel(const float* __restrict__ logits,
                                                         const float* __restrict__ target,
                                                         const float* __restrict__ ws, float* __restrict__ dlogits,
                                                         int B, long long n) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)B * n) return;
    const int b = (int)(idx / n);
    const float* img = ws + (size_t)B * NB * 3 + (size_t)b * 3;
    const float num = img[0], den = img[1];
    const float m1 = 1.f / (1.f + __expf(-logits[idx])), m2 = target[idx];
    // score = 2 num / den: d score / d m1 = 2 m2 / den - 2 num 2 m1 / den^2; loss = 1 - mean score
    const float dscore = 2.f * m2 / den - 4.f * num * m1 / (den * den);
    dlogits[idx] = -(dscore / (float)B) * m1 * (1.f - m1);
}

// ------------------------------------------------------------------ InfoNCE (MoCo-v3 builder.py:63-73)
// logits = q^ k^T / T are produced tile by tile from fp32 FMA chains and never stored: pass 1 keeps per
// (row, key chunk) the running maximum, the sum of exp(logit - max) and the positive logit; pass 2 rebuilds the
// same tiles (same code, same bits), forms p = exp(logit - lse) - [j == label] and multiplies it with the keys.
// A workgroup owns NCE_TR query rows x one chunk of keys; the chunks split the keys over the chip.
constexpr int NCE_TR = 32;       // query rows per workgroup (8 per wave)
constexpr int NCE_TK = 64;       // keys per sub-tile (one per lane)
constexpr int NCE_KC = 32;       // features staged in LDS per step
constexpr int NCE_MAXCHUNK = 64; // key chunks (grid.y, and the depth of the finalize sums)
constexpr float NCE_EPS = 1e-12f; // F.normalize's eps

struct NcePlan { int rowtiles, nsub, spc, nchunk; };
static NcePlan nce_plan(int N, int M) {
    NcePlan p;
    p.rowtiles = (N + NCE_TR - 1) / NCE_TR;
    p.nsub = (M + NCE_TK - 1) / NCE_TK;
    int want = (512 + p.rowtiles - 1) / p.rowtiles;  // ~2 workgroups per CU
    want = want > NCE_MAXCHUNK ? NCE_MAXCHUNK : want;
    want = want > p.nsub ? p.nsub : want;
    p.spc = (p.nsub + want - 1) / want;              // sub-tiles per chunk
    p.nchunk = (p.nsub + p.spc - 1) / p.spc;         // every chunk holds at least one key
    return p;
}
// fp32 workspace: qn [N][C] | kn [M][C] | qnorm [N] | part [nchunk][N][3] | dqp [nchunk][N][C]
struct NceWs { float *qn, *kn, *qnorm, *part, *dqp; };
DEVI NceWs nce_ws(float* ws, int N, int M, int C) {
    NceWs w;
    w.qn = ws;
    w.kn = w.qn + (size_t)N * C;
    w.qnorm = w.kn + (size_t)M * C;
    w.part = w.qnorm + N;
    w.dqp = w.part + (size_t)NCE_MAXCHUNK * N * 3;
    return w;
}

// one wave per row of q (rows < N) or k: x / max(||x||, eps), and ||q||
__global__ __launch_bounds__(256) void nce_norm_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                       float* __restrict__ ws, int N, int M, int C) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= (long long)N + M) return;
    const NceWs w = nce_ws(ws, N, M, C);
    const float* src = row < N ? q + (size_t)row * C : k + (size_t)(row - N) * C;
    float* dst = row < N ? w.qn + (size_t)row * C : w.kn + (size_t)(row - N) * C;
    float ss = 0.f;
    for (int c = lane; c < C; c += 64) ss += src[c] * src[c];
    const float nrm = sqrtf(wave_sum(ss));
    const float den = fmaxf(nrm, NCE_EPS);
    for (int c = lane; c < C; c += 64) dst[c] = src[c] / den;
    if (row < N && lane == 0) w.qnorm[row] = nrm;
}

// log-sum-exp of row `row` from the chunk partials (fixed order), and its positive logit
DEVI float nce_row_lse(const float* __restrict__ part, int N, int nchunk, int row, float& pos) {
    float m = -INFINITY;
    for (int ch = 0; ch < nchunk; ++ch) m = fmaxf(m, part[((size_t)ch * N + row) * 3]);
    float s = 0.f, p = 0.f;
    for (int ch = 0; ch < nchunk; ++ch) {
        const float* o = part + ((size_t)ch * N + row) * 3;
        s += o[1] * expf(o[0] - m);
        p += o[2];  // zero in every chunk but the label's
    }
    pos = p;
    return m + logf(s);
}

template <bool GRAD>
__global__ __launch_bounds__(256) void nce_pass_kernel(float* __restrict__ ws, int N, int M, int C, float T,
                                                       int off, int nsub, int spc, int nchunk) {
    __shared__ float qs[NCE_TR][NCE_KC + 1];
    __shared__ float ks[NCE_KC][NCE_TK + 1];
    __shared__ __attribute__((aligned(16))) float pt[GRAD ? NCE_TK : 1][NCE_TR + 4];  // p, [key][row]
    __shared__ float lse_s[NCE_TR];
    const NceWs w = nce_ws(ws, N, M, C);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int r0 = blockIdx.x * NCE_TR, chunk = blockIdx.y;
    const int sub0 = chunk * spc, sub1 = (sub0 + spc < nsub) ? sub0 + spc : nsub;
    float mrun[8], srun[8], prun[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) { mrun[u] = -INFINITY; srun[u] = 0.f; prun[u] = 0.f; }
    if (GRAD) {
        if (t < NCE_TR) {
            float pos;
            lse_s[t] = (r0 + t < N) ? nce_row_lse(w.part, N, nchunk, r0 + t, pos) : 0.f;
        }
        __syncthreads();
    }
    for (int sub = sub0; sub < sub1; ++sub) {
        const int j0 = sub * NCE_TK;
        float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int c0 = 0; c0 < C; c0 += NCE_KC) {
#pragma unroll
            for (int u = 0; u < NCE_TR * NCE_KC / 256; ++u) {
                const int e = t + 256 * u, rr = e >> 5, cc = e & 31;
                qs[rr][cc] = (r0 + rr < N && c0 + cc < C) ? w.qn[(size_t)(r0 + rr) * C + c0 + cc] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < NCE_TK * NCE_KC / 256; ++u) {
                const int e = t + 256 * u, jj = e >> 5, cc = e & 31;
                ks[cc][jj] = (j0 + jj < M && c0 + cc < C) ? w.kn[(size_t)(j0 + jj) * C + c0 + cc] : 0.f;
            }
            __syncthreads();
#pragma unroll 8
            for (int cc = 0; cc < NCE_KC; ++cc) {
                const float kv = ks[cc][lane];
#pragma unroll
                for (int u = 0; u < 8; ++u) acc[u] += qs[wave * 8 + u][cc] * kv;
            }
            __syncthreads();
        }
        const bool valid = j0 + lane < M;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int row = r0 + wave * 8 + u;
            const float l = acc[u] / T;
            const bool hit = valid && row < N && j0 + lane == off + row;
            if constexpr (!GRAD) {
                const float mnew = fmaxf(mrun[u], wave_max(valid ? l : -INFINITY));  // finite: lane 0 is valid
                const float e = valid ? expf(l - mnew) : 0.f;
                srun[u] = srun[u] * expf(mrun[u] - mnew) + wave_sum(e);
                mrun[u] = mnew;
                prun[u] += wave_sum(hit ? l : 0.f);
            } else {
                float p = (valid && row < N) ? expf(l - lse_s[wave * 8 + u]) : 0.f;
                if (hit) p -= 1.f;
                pt[lane][wave * 8 + u] = p;
            }
        }
        if constexpr (GRAD) {
            __syncthreads();
            const int nk = (M - j0 < NCE_TK) ? M - j0 : NCE_TK;
            for (int c = t; c < C; c += 256) {
                float g[NCE_TR];
#pragma unroll
                for (int r = 0; r < NCE_TR; ++r) g[r] = 0.f;
                const float* kcol = w.kn + (size_t)j0 * C + c;
                for (int jj = 0; jj < nk; ++jj) {
                    const float kv = kcol[(size_t)jj * C];
#pragma unroll
                    for (int r4 = 0; r4 < NCE_TR / 4; ++r4) {
                        const f32x4 p4 = *(const f32x4*)&pt[jj][r4 * 4];
                        g[r4 * 4 + 0] += p4[0] * kv; g[r4 * 4 + 1] += p4[1] * kv;
                        g[r4 * 4 + 2] += p4[2] * kv; g[r4 * 4 + 3] += p4[3] * kv;
                    }
                }
#pragma unroll
                for (int r = 0; r < NCE_TR; ++r) {
                    if (r0 + r < N) {  // this workgroup alone owns the slab [chunk][r0 .. r0 + 32)
                        float* o = w.dqp + ((size_t)chunk * N + r0 + r) * C + c;
                        *o = (sub == sub0) ? g[r] : *o + g[r];
                    }
                }
            }
            // the next sub-tile writes pt only after the barriers of its feature loop
        }
    }
    if (!GRAD && lane == 0) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int row = r0 + wave * 8 + u;
            if (row < N) {
                float* o = w.part + ((size_t)chunk * N + row) * 3;
                o[0] = mrun[u]; o[1] = srun[u]; o[2] = prun[u];
            }
        }
    }
}

// block 0: loss = 2T mean_i(lse_i - logit_i,label) from fp32 row terms, summed in fp64 in a fixed order;
// block 1 + i (only with a gradient): dq^_i = (2/N) sum over chunks, then the Jacobian of x / max(||x||, eps)
__global__ __launch_bounds__(256) void nce_finalize_kernel(float* __restrict__ ws, float* __restrict__ loss,
                                                           float* __restrict__ dq, int N, int M, int C, float T,
                                                           int nchunk) {
    const NceWs w = nce_ws(ws, N, M, C);
    const int t = threadIdx.x;
    if (blockIdx.x == 0) {
        __shared__ double sh[256];
        double a = 0.0;
        for (int i = t; i < N; i += 256) {
            float pos;
            const float lse = nce_row_lse(w.part, N, nchunk, i, pos);
            a += (double)(lse - pos);
        }
        sh[t] = a;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (t < o) sh[t] += sh[t + o];
            __syncthreads();
        }
        if (t == 0) *loss = (float)(2.0 * (double)T * sh[0] / (double)N);
        return;
    }
    const int i = blockIdx.x - 1;
    const float scale = 2.f / (float)N;
    float g[4], qh[4], dot = 0.f;  // C <= 1024: at most 4 features per thread
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int c = t + 256 * u;
        g[u] = 0.f; qh[u] = 0.f;
        if (c < C) {
            float s = 0.f;
            for (int ch = 0; ch < nchunk; ++ch) s += w.dqp[((size_t)ch * N + i) * C + c];
            g[u] = s * scale;
            qh[u] = w.qn[(size_t)i * C + c];
            dot += qh[u] * g[u];
        }
    }
    __shared__ float shd[4];
    dot = wave_sum(dot);
    if ((t & 63) == 0) shd[t >> 6] = dot;
    __syncthreads();
    dot = block_get<SumOrder::Pairwise>(shd);
    const float nrm = w.qnorm[i];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int c = t + 256 * u;
        if (c < C) dq[(size_t)i * C + c] = nrm > NCE_EPS ? (g[u] - qh[u] * dot) / nrm : g[u] / NCE_EPS;
    }
}

// ------------------------------------------------------------------ weighted cross-entropy (mean reduction)
constexpr int CE_MAXBLK = 512;
// fp32 workspace: part [CE_MAXBLK][2] (sum w nll, sum w) | lse [B]
__global__ __launch_bounds__(256) void ce_rows_kernel(const float* __restrict__ logits,
                                                      const long long* __restrict__ target,
                                                      const float* __restrict__ weight, float* __restrict__ ws,
                                                      int B, int C) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float v[2] = {0.f, 0.f};  // wave totals, lane 0's copy is the one used
    for (long long row = (long long)blockIdx.x * 4 + wave; row < B; row += (long long)gridDim.x * 4) {
        const float* x = logits + (size_t)row * C;
        float m = -INFINITY;
        for (int c = lane; c < C; c += 64) m = fmaxf(m, x[c]);
        m = wave_max(m);
        float s = 0.f;
        for (int c = lane; c < C; c += 64) s += expf(x[c] - m);
        const float lse = m + logf(wave_sum(s));
        const long long tg = target[row];
        const bool ok = tg >= 0 && tg < C;  // a label outside [0, C) is never used as an index
        const float wt = ok ? (weight ? weight[tg] : 1.f) : 0.f;
        v[0] += ok ? wt * (lse - x[tg]) : NAN;
        v[1] += wt;
        if (lane == 0) ws[2 * CE_MAXBLK + row] = lse;
    }
    __shared__ float sh[4 * 2];
    if (lane == 0) { sh[wave * 2] = v[0]; sh[wave * 2 + 1] = v[1]; }
    __syncthreads();
    if (threadIdx.x == 0) {
        ws[blockIdx.x * 2] = block_get<SumOrder::Pairwise, 2>(sh, 0);
        ws[blockIdx.x * 2 + 1] = block_get<SumOrder::Pairwise, 2>(sh, 1);
    }
}
__global__ __launch_bounds__(256) void ce_apply_kernel(const float* __restrict__ logits,
                                                       const long long* __restrict__ target,
                                                       const float* __restrict__ weight,
                                                       const float* __restrict__ ws, float* __restrict__ loss,
                                                       float* __restrict__ dlogits, int B, int C, int nblk) {
    __shared__ double sh[2][256];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double a = 0.0, b = 0.0;
    for (int p = t; p < nblk; p += 256) { a += (double)ws[p * 2]; b += (double)ws[p * 2 + 1]; }
    sh[0][t] = a; sh[1][t] = b;
    block_tree_sum(sh, t);
    if (blockIdx.x == 0 && t == 0) *loss = (float)(sh[0][0] / sh[1][0]);  // sum w = 0: NaN, as torch
    if (!dlogits) return;
    const float wsum = (float)sh[1][0];
    for (long long row = (long long)blockIdx.x * 4 + wave; row < B; row += (long long)gridDim.x * 4) {
        const float* x = logits + (size_t)row * C;
        float* d = dlogits + (size_t)row * C;
        const float lse = ws[2 * CE_MAXBLK + row];
        const long long tg = target[row];
        const bool ok = tg >= 0 && tg < C;
        const float wt = ok ? (weight ? weight[tg] : 1.f) : 0.f;
        for (int c = lane; c < C; c += 64)
            d[c] = ok ? wt * (expf(x[c] - lse) - (c == tg ? 1.f : 0.f)) / wsum : NAN;
    }
}

// ------------------------------------------------------------------ soft-target / label-smoothing cross-entropy
// loss = mean_b sum_c -t[b, c] log_softmax(x[b])[c] with t either given ([B, C]: Mixup's soft targets, timm's
// SoftTargetCrossEntropy) or built here from a label (timm's LabelSmoothingCrossEntropy: t = conf [c == y] + off).
// One wave per row: max and sum in one online pass, then a second pass over the (cached) row for the loss terms and
// dlogits = (softmax sum_c t - t) / B, which does not assume sum_c t = 1.  fp32 workspace: part [CE_MAXBLK].
__global__ __launch_bounds__(256) void soft_ce_rows_kernel(const float* __restrict__ logits,
                                                           const float* __restrict__ tsoft,
                                                           const long long* __restrict__ label, float conf, float off,
                                                           float* __restrict__ ws, float* __restrict__ dlogits, int B,
                                                           int C) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float total = 0.f;  // wave total, lane 0's copy is the one used
    for (long long row = (long long)blockIdx.x * 4 + wave; row < B; row += (long long)gridDim.x * 4) {
        const float* x = logits + (size_t)row * C;
        float m = -INFINITY, s = 0.f;
        for (int c = lane; c < C; c += 64) {
            const float v = x[c];
            if (v > m) { s = s * expf(m - v) + 1.f; m = v; }
            else s += expf(v - m);
        }
        const float M = wave_max(m);
        s = wave_sum(m == -INFINITY ? 0.f : s * expf(m - M));
        const float logs = logf(s);
        long long tg = 0;
        bool ok = true;
        if (!tsoft) {
            tg = label[row];
            ok = tg >= 0 && tg < C;  // a label outside [0, C) is never used as an index
        }
        const float* t = tsoft ? tsoft + (size_t)row * C : nullptr;
        float tsum = 0.f, nll = 0.f;
        for (int c = lane; c < C; c += 64) {
            const float tc = t ? t[c] : (c == tg ? conf : 0.f) + off;
            tsum += tc;
            nll += tc * (logs - (x[c] - M));  // -t log_softmax
        }
        tsum = wave_sum(tsum);
        nll = wave_sum(nll);
        total += ok ? nll : NAN;
        if (dlogits) {
            float* d = dlogits + (size_t)row * C;
            for (int c = lane; c < C; c += 64) {
                const float tc = t ? t[c] : (c == tg ? conf : 0.f) + off;
                d[c] = ok ? (expf((x[c] - M) - logs) * tsum - tc) / (float)B : NAN;
            }
        }
    }
    __shared__ float sh[4];
    if (lane == 0) sh[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0) ws[blockIdx.x] = block_get<SumOrder::Pairwise>(sh);
}
__global__ __launch_bounds__(256) void soft_ce_finalize_kernel(const float* __restrict__ ws, float* __restrict__ loss,
                                                               int B, int nblk) {
    __shared__ double sh[256];
    const int t = threadIdx.x;
    double a = 0.0;
    for (int p = t; p < nblk; p += 256) a += (double)ws[p];
    sh[t] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) sh[t] += sh[t + o];
        __syncthreads();
    }
    if (t == 0) *loss = (float)(sh[0] / (double)B);
}

// ------------------------------------------------------------------ Barlow Twins loss terms
constexpr int BT_MAXBLK = 1024;
constexpr int BT_TILE = 64;
DEVI void bt_term(float v, bool diag, float& on, float& off) {
    if (diag) on += (v - 1.f) * (v - 1.f);
    else off += v * v;
}
// one read of c: per-block fp32 (sum_i (c_ii - 1)^2, sum_{i != j} c_ij^2), the off-diagonal terms summed directly
__global__ __launch_bounds__(256) void bt_loss_partial_kernel(const float* __restrict__ c, float* __restrict__ ws,
                                                              int D) {
    float v[2] = {0.f, 0.f};
    for (int r = blockIdx.x; r < D; r += gridDim.x) {
        const float* row = c + (size_t)r * D;
        if ((D & 3) == 0 && ((uintptr_t)c & 15) == 0) {
            for (int j = threadIdx.x * 4; j < D; j += 1024) {
                const f32x4 x = ld4(row + j);
#pragma unroll
                for (int e = 0; e < 4; ++e) bt_term(x[e], j + e == r, v[0], v[1]);
            }
        } else {
            for (int j = threadIdx.x; j < D; j += 256) bt_term(row[j], j == r, v[0], v[1]);
        }
    }
    __shared__ float sh[4 * 2];
    block_sum<SumOrder::Sequential>(v, sh);
    if (threadIdx.x == 0) { ws[blockIdx.x * 2] = v[0]; ws[blockIdx.x * 2 + 1] = v[1]; }
}
__global__ __launch_bounds__(256) void bt_loss_final_kernel(const float* __restrict__ ws, float* __restrict__ loss,
                                                            int nblk, float lambd) {
    __shared__ double sh[2][256];
    const int t = threadIdx.x;
    double a = 0.0, b = 0.0;
    for (int p = t; p < nblk; p += 256) { a += (double)ws[p * 2]; b += (double)ws[p * 2 + 1]; }
    sh[0][t] = a; sh[1][t] = b;
    block_tree_sum(sh, t);
    if (t == 0) *loss = (float)(sh[0][0] + (double)lambd * sh[1][0]);
}
// one read of c, both GEMM operands of the backward: w = round(dc s), wt = w^T through an LDS tile so that both
// stores run along rows.  Multiplies only (each rounded to fp32), in the order of the torch ops they replace:
// dc = c (float)(2 lambda) off the diagonal, 2 (c - 1) on it, then dc * s.
DEVI void st2(float* p, float a, float b) { *(f32x2*)p = f32x2{a, b}; }
DEVI void st2(bf16_t* p, float a, float b) { *(uint32_t*)p = pack_bf2(a, b); }
DEVI float bt_dc(float v, bool diag, float two_lambd, float s) {
    const float dc = diag ? 2.f * (v - 1.f) : v * two_lambd;
    return dc * s;
}
// PAIR (D even, pointers aligned to two elements): every thread moves two neighbouring elements per access
template <typename T, bool PAIR>
__global__ __launch_bounds__(256) void bt_grad_kernel(const float* __restrict__ c, const float* __restrict__ scale,
                                                      T* __restrict__ w, T* __restrict__ wt, int D, float two_lambd) {
    __shared__ float tile[BT_TILE][BT_TILE + 1];
    const int i0 = blockIdx.y * BT_TILE, j0 = blockIdx.x * BT_TILE;
    const float s = *scale;
    if constexpr (PAIR) {
        const int tp = threadIdx.x & 31, tr = threadIdx.x >> 5;
        for (int rr = tr; rr < BT_TILE; rr += 8) {
            const int i = i0 + rr, j = j0 + 2 * tp;
            if (i < D && j < D) {  // D even, j even: j + 1 < D as well
                const f32x2 v = *(const f32x2*)(c + (size_t)i * D + j);
                const float o0 = bt_dc(v[0], i == j, two_lambd, s), o1 = bt_dc(v[1], i == j + 1, two_lambd, s);
                st2(w + (size_t)i * D + j, o0, o1);
                tile[rr][2 * tp] = o0;
                tile[rr][2 * tp + 1] = o1;
            }
        }
        __syncthreads();
        for (int rr = tr; rr < BT_TILE; rr += 8) {
            const int j = j0 + rr, i = i0 + 2 * tp;
            if (i < D && j < D) st2(wt + (size_t)j * D + i, tile[2 * tp][rr], tile[2 * tp + 1][rr]);
        }
    } else {
        const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
        for (int rr = ty; rr < BT_TILE; rr += 4) {
            const int i = i0 + rr, j = j0 + tx;
            if (i < D && j < D) {
                const float o = bt_dc(c[(size_t)i * D + j], i == j, two_lambd, s);
                Elem<T>::st(w + (size_t)i * D + j, o);
                tile[rr][tx] = o;
            }
        }
        __syncthreads();
        for (int rr = ty; rr < BT_TILE; rr += 4) {
            const int j = j0 + rr, i = i0 + tx;
            if (i < D && j < D) Elem<T>::st(wt + (size_t)j * D + i, tile[tx][rr]);
        }
    }
}

template <typename T>
static void bt_grad_launch(const float* c, const float* scale, void* w, void* wt, int D, float two_lambd,
                           hipStream_t st) {
    const unsigned nt = (unsigned)((D + BT_TILE - 1) / BT_TILE);
    const bool pair = (D & 1) == 0 && ((uintptr_t)c & 7) == 0 && ((uintptr_t)w & (2 * sizeof(T) - 1)) == 0 &&
                      ((uintptr_t)wt & (2 * sizeof(T) - 1)) == 0;
    if (pair)
        hipLaunchKernelGGL((bt_grad_kernel<T, true>), dim3(nt, nt), dim3(256), 0, st, c, scale, (T*)w, (T*)wt, D,
                           two_lambd);
    else
        hipLaunchKernelGGL((bt_grad_kernel<T, false>), dim3(nt, nt), dim3(256), 0, st, c, scale, (T*)w, (T*)wt, D,
                           two_lambd);
}

}  // namespace

extern "C" size_t ssl4gie_ssi_loss_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    const size_t n = (size_t)B * NB * NSUM_A + (size_t)B * 12 + 8 + (size_t)B * NB * NSUM_B + (size_t)B * H * W;
    return n * sizeof(float);
}

extern "C" int ssl4gie_ssi_loss(const float* pred, const float* target, float* loss, float* dpred, int B, int H,
                                int W, float alpha, int scales, void* workspace, void* stream) {
    REQUIRE(pred && target && loss && dpred && workspace && B > 0 && H > 0 && W > 0 && scales >= 1 && scales <= 4);
    REQUIRE(B <= 65535);
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    const long long HW = (long long)H * W;
    hipLaunchKernelGGL(ssi_sums_kernel, dim3(NB, B), dim3(256), 0, st, pred, target, ws, B, H, W);
    hipLaunchKernelGGL(ssi_finalize_a_kernel, dim3(1), dim3(256), 0, st, ws, B, HW);
    hipLaunchKernelGGL(ssi_grad_kernel, dim3(NB, B), dim3(256), 0, st, pred, target, ws, B, H, W, alpha, scales);
    hipLaunchKernelGGL(ssi_finalize_b_kernel, dim3(1), dim3(256), 0, st, ws, loss, B, HW, alpha, scales);
    const long long total = (long long)B * HW;
    hipLaunchKernelGGL(ssi_apply_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, pred, target,
                       (const float*)ws, dpred, B, HW);
    LAUNCH_CHECK();
    return 0;
}

extern "C" size_t ssl4gie_dice_loss_workspace_bytes(int B) {
    return B > 0 ? ((size_t)B * NB * 3 + (size_t)B * 3) * sizeof(float) : 0;
}

extern "C" int ssl4gie_dice_loss(const float* logits, const float* target, float* loss, float* dlogits, int B,
                                 long long n, float smooth, void* workspace, void* stream) {
    REQUIRE(logits && target && loss && dlogits && workspace && B > 0 && B <= 65535 && n > 0);
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    hipLaunchKernelGGL(dice_sums_kernel, dim3(NB, B), dim3(256), 0, st, logits, target, ws, n);
    hipLaunchKernelGGL(dice_finalize_kernel, dim3(1), dim3(256), 0, st, ws, loss, B, smooth);
    const long long total = (long long)B * n;
    hipLaunchKernelGGL(dice_apply_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, logits, target,
                       (const float*)ws, dlogits, B, n);
    LAUNCH_CHECK();
    return 0;
}

extern "C" size_t ssl4gie_infonce_workspace_bytes(int N, int M, int C) {
    if (N < 1 || M < 1 || C < 1) return 0;
    const NcePlan p = nce_plan(N, M);
    const size_t n = (size_t)N * C + (size_t)M * C + (size_t)N + (size_t)NCE_MAXCHUNK * N * 3 +
                     (size_t)p.nchunk * N * C;
    return n * sizeof(float);
}

extern "C" int ssl4gie_infonce_loss(const float* q, const float* k, float* loss, float* dq, int N, int M, int C,
                                    float T, int label_offset, void* workspace, void* stream) {
    REQUIRE(q && k && loss && workspace);
    REQUIRE(N >= 1 && M >= 1 && C >= 1 && C <= 1024 && T > 0.f && label_offset >= 0);
    REQUIRE((long long)label_offset + N <= (long long)M);
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    const NcePlan p = nce_plan(N, M);
    const long long rows = (long long)N + M;
    hipLaunchKernelGGL(nce_norm_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, q, k, ws, N, M, C);
    const dim3 grid(p.rowtiles, p.nchunk);
    hipLaunchKernelGGL(nce_pass_kernel<false>, grid, dim3(256), 0, st, ws, N, M, C, T, label_offset, p.nsub, p.spc,
                       p.nchunk);
    if (dq)
        hipLaunchKernelGGL(nce_pass_kernel<true>, grid, dim3(256), 0, st, ws, N, M, C, T, label_offset, p.nsub,
                           p.spc, p.nchunk);
    hipLaunchKernelGGL(nce_finalize_kernel, dim3(dq ? N + 1 : 1), dim3(256), 0, st, ws, loss, dq, N, M, C, T,
                       p.nchunk);
    LAUNCH_CHECK();
    return 0;
}

static int ce_blocks(int B) {
    const long long nb = ((long long)B + 3) / 4;
    return nb > CE_MAXBLK ? CE_MAXBLK : (int)nb;
}

extern "C" size_t ssl4gie_cross_entropy_workspace_bytes(int B, int C) {
    if (B < 1 || C < 1) return 0;
    return ((size_t)2 * CE_MAXBLK + (size_t)B) * sizeof(float);
}

extern "C" int ssl4gie_cross_entropy(const float* logits, const long long* target, const float* weight, float* loss,
                                     float* dlogits, int B, int C, void* workspace, void* stream) {
    REQUIRE(logits && target && loss && workspace && B >= 1 && C >= 1);
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    const int nblk = ce_blocks(B);
    hipLaunchKernelGGL(ce_rows_kernel, dim3(nblk), dim3(256), 0, st, logits, target, weight, ws, B, C);
    hipLaunchKernelGGL(ce_apply_kernel, dim3(dlogits ? nblk : 1), dim3(256), 0, st, logits, target, weight,
                       (const float*)ws, loss, dlogits, B, C, nblk);
    LAUNCH_CHECK();
    return 0;
}

extern "C" size_t ssl4gie_soft_cross_entropy_workspace_bytes(int B, int C) {
    if (B < 1 || C < 1) return 0;
    return (size_t)CE_MAXBLK * sizeof(float);
}

extern "C" int ssl4gie_soft_cross_entropy(const float* logits, const float* soft_target, const long long* label,
                                          float conf, float off, float* loss, float* dlogits, int B, int C,
                                          void* workspace, void* stream) {
    REQUIRE(logits && loss && workspace && B >= 1 && C >= 1);
    REQUIRE((soft_target != nullptr) != (label != nullptr));
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    const int nblk = ce_blocks(B);
    hipLaunchKernelGGL(soft_ce_rows_kernel, dim3(nblk), dim3(256), 0, st, logits, soft_target, label, conf, off, ws,
                       dlogits, B, C);
    hipLaunchKernelGGL(soft_ce_finalize_kernel, dim3(1), dim3(256), 0, st, (const float*)ws, loss, B, nblk);
    LAUNCH_CHECK();
    return 0;
}

static int bt_blocks(int D) { return D > BT_MAXBLK ? BT_MAXBLK : D; }

extern "C" size_t ssl4gie_bt_loss_workspace_bytes(int D) {
    return D >= 1 ? (size_t)2 * bt_blocks(D) * sizeof(float) : 0;
}

extern "C" int ssl4gie_bt_loss(const float* c, float* loss, int D, float lambd, void* workspace, void* stream) {
    REQUIRE(c && loss && workspace && D >= 1);
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    const int nblk = bt_blocks(D);
    hipLaunchKernelGGL(bt_loss_partial_kernel, dim3(nblk), dim3(256), 0, st, c, ws, D);
    hipLaunchKernelGGL(bt_loss_final_kernel, dim3(1), dim3(256), 0, st, (const float*)ws, loss, nblk, lambd);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int ssl4gie_bt_loss_grad(const float* c, const float* scale, void* w, void* wt, int dtype, int D,
                                    float lambd, void* stream) {
    REQUIRE(c && scale && w && wt && D >= 1 && (dtype == SSL4GIE_F32 || dtype == SSL4GIE_BF16));
    hipStream_t st = (hipStream_t)stream;
    const unsigned nt = (unsigned)((D + BT_TILE - 1) / BT_TILE);
    REQUIRE(nt <= 65535u);
    const float two_lambd = 2.f * lambd;  // == (float)(2.0 * lambda): doubling is exact
    if (dtype == SSL4GIE_F32)
        bt_grad_launch<float>(c, scale, w, wt, D, two_lambd, st);
    else
        bt_grad_launch<bf16_t>(c, scale, w, wt, D, two_lambd, st);
    LAUNCH_CHECK();
    return 0;
}
