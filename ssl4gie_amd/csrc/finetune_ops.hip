// Element-wise kernels of the MAE fine-tuning recipe (reference Models/mae/main_finetune.py):
//   * stochastic depth beside the block executor's GEMMs (timm's drop_path, per-sample factor s[b] in
//     {0, 1 / keep_prob}): out = res + s[b] t in the forward, dy_s = cast(s[b] dx) in the backward;
//   * Mixup / CutMix on a resident batch, in place (timm.data.Mixup, main_finetune.py:221-226).
// All three are HBM-bound: 16-byte accesses, lanes contiguous along the innermost axis, a few vectors in flight
// per lane, one integer division per vector for the sample index.
#include "common.h"
#include "ssl4gie_hip.h"

namespace {

constexpr int DP_UNROLL = 4;  // 16-byte vectors per lane: 64 B of each operand in flight

// sample of vector `v` when a sample spans `vps` vectors; 32-bit division whenever the count fits (common.h map_index)
DEVI long long sample_of(long long v, long long total, long long vps) {
    if (total <= 0xffffffffLL) return (long long)((unsigned)v / (unsigned)vps);
    return v / vps;
}

// out = res + s[b] t.  A dropped sample (s[b] == 0) is a copy of res and t is NOT read: the row comes out bit-equal
// to its input and a non-finite branch value cannot leak through 0 * inf (timm multiplies).
__global__ __launch_bounds__(256) void drop_path_add_kernel(const float* __restrict__ res, const float* __restrict__ t,
                                                            const float* __restrict__ s, float* __restrict__ out,
                                                            long long nvec, long long vps) {
    const long long base = (long long)blockIdx.x * (256 * DP_UNROLL) + threadIdx.x;
    f32x4 r[DP_UNROLL], b[DP_UNROLL];
    float sc[DP_UNROLL];
#pragma unroll
    for (int u = 0; u < DP_UNROLL; ++u) {
        const long long v = base + u * 256;
        sc[u] = 0.f;
        r[u] = b[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (v < nvec) {
            sc[u] = s[sample_of(v, nvec, vps)];
            r[u] = ld4(res + v * 4);
            if (sc[u] != 0.f) b[u] = ld4(t + v * 4);
        }
    }
#pragma unroll
    for (int u = 0; u < DP_UNROLL; ++u) {
        const long long v = base + u * 256;
        if (v < nvec) st4(out + v * 4, sc[u] != 0.f ? r[u] + sc[u] * b[u] : r[u]);
    }
}

// dy_s = cast(s[b] dx); a dropped sample is written as zeros and dx is not read
template <typename T>
__global__ __launch_bounds__(256) void drop_path_scale_cast_kernel(const float* __restrict__ dx,
                                                                   const float* __restrict__ s, T* __restrict__ out,
                                                                   long long nvec, long long vps) {
    const long long base = (long long)blockIdx.x * (256 * DP_UNROLL) + threadIdx.x;
    f32x4 g[DP_UNROLL];
#pragma unroll
    for (int u = 0; u < DP_UNROLL; ++u) {
        const long long v = base + u * 256;
        g[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (v < nvec) {
            const float sc = s[sample_of(v, nvec, vps)];
            if (sc != 0.f) g[u] = ld4(dx + v * 4) * sc;
        }
    }
#pragma unroll
    for (int u = 0; u < DP_UNROLL; ++u) {
        const long long v = base + u * 256;
        if (v < nvec) st4(out + v * 4, g[u]);
    }
}

unsigned dp_blocks(long long nvec) { return (unsigned)((nvec + 256 * DP_UNROLL - 1) / (256 * DP_UNROLL)); }

// ---------------------------------------------------------------------------------------------- Mixup / CutMix
// One thread owns the same element(s) of samples i and j = B - 1 - i: both originals are loaded before either result
// is written, so the in-place batch never shows a mixed value to its partner (timm's `elem` mode mixes both halves
// from the unmixed batch; `batch` and `pair` mode are the same kernel with tables that repeat / mirror).
// Products are rounded one by one and added once (no fused multiply-add): bit-equal to
// x.mul(lam).add(x.flip(0).mul(1 - lam)) in fp32.
DEVI float mix1(float a, float b, float lam, float oml) { return __fadd_rn(__fmul_rn(a, lam), __fmul_rn(b, oml)); }

struct MixRow {
    float lam, oml;
    int cut, y0, y1, x0, x1;  // cut: 0 mixup, 1 cutmix with box [y0, y1) x [x0, x1); lam = NaN marks a refused row
};
DEVI MixRow mix_row(const float* __restrict__ lam, const int* __restrict__ box,
                    const unsigned char* __restrict__ use_cutmix, int i, int H, int W) {
    MixRow m;
    m.lam = lam[i];
    m.oml = 1.f - m.lam;
    m.cut = use_cutmix[i] != 0;
    m.y0 = box[4 * i]; m.y1 = box[4 * i + 1]; m.x0 = box[4 * i + 2]; m.x1 = box[4 * i + 3];
    // no address is formed from the box: it only gates a select between the two loaded values.  A box outside the
    // image (or a non-finite lambda) is refused all the same: the sample comes out NaN.
    const bool ok = !m.cut ? (m.lam == m.lam)
                           : (m.y0 >= 0 && m.y0 <= m.y1 && m.y1 <= H && m.x0 >= 0 && m.x0 <= m.x1 && m.x1 <= W);
    if (!ok) { m.cut = 0; m.lam = NAN; m.oml = NAN; }
    return m;
}
DEVI float mix_elem(const MixRow& m, float own, float other, int y, int x) {
    if (m.cut) return (y >= m.y0 && y < m.y1 && x >= m.x0 && x < m.x1) ? other : own;
    return mix1(own, other, m.lam, m.oml);
}

// grid (ceil(C H ceil(W / 4) / 256), ceil(B / 2)); VEC: 16-byte accesses (W % 4 == 0 and a 16-byte aligned base)
template <bool VEC>
__global__ __launch_bounds__(256) void mixup_kernel(float* __restrict__ x, const float* __restrict__ lam,
                                                    const int* __restrict__ box,
                                                    const unsigned char* __restrict__ use_cutmix, int B, int C, int H,
                                                    int W) {
    const int i = blockIdx.y, j = B - 1 - i;
    const int wv = VEC ? W / 4 : W;
    const unsigned per = (unsigned)C * H * wv;
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= per) return;
    const unsigned row = idx / (unsigned)wv;           // c * H + y
    const int xv = (int)(idx - row * (unsigned)wv);
    const int y = (int)(row % (unsigned)H);
    const MixRow mi = mix_row(lam, box, use_cutmix, i, H, W);
    const MixRow mj = mix_row(lam, box, use_cutmix, j, H, W);
    const size_t chw = (size_t)C * H * W;
    float* pi = x + (size_t)i * chw + (size_t)row * W;
    float* pj = x + (size_t)j * chw + (size_t)row * W;
    if (VEC) {
        const f32x4 a = ld4(pi + xv * 4), b = ld4(pj + xv * 4);
        f32x4 oi, oj;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            oi[e] = mix_elem(mi, a[e], b[e], y, xv * 4 + e);
            oj[e] = mix_elem(mj, b[e], a[e], y, xv * 4 + e);
        }
        st4(pi + xv * 4, oi);
        if (j != i) st4(pj + xv * 4, oj);
    } else {
        const float a = pi[xv], b = pj[xv];
        pi[xv] = mix_elem(mi, a, b, y, xv);
        if (j != i) pj[xv] = mix_elem(mj, b, a, y, xv);
    }
}

// soft targets [B, C]: off = eps / C, on = 1 - eps + off (rounded by the caller), row i = onehot(y_i) lam_i + onehot(y_j) (1 - lam_i), the
// products rounded one by one as torch's `y1 * lam + y2 * (1. - lam)` rounds them.  A label outside [0, C) is never
// an index: its row is NaN.
__global__ __launch_bounds__(256) void mixup_target_kernel(const long long* __restrict__ target,
                                                           const float* __restrict__ lam, float* __restrict__ out,
                                                           int B, int C, float on, float off) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)B * C) return;
    const int i = (int)(idx / C), c = (int)(idx - (long long)i * C);
    const long long ti = target[i], tj = target[B - 1 - i];
    const float l = lam[i], o = 1.f - l;
    const bool ok = ti >= 0 && ti < C && tj >= 0 && tj < C;
    out[idx] = ok ? mix1(c == ti ? on : off, c == tj ? on : off, l, o) : NAN;
}

}  // namespace

extern "C" int ssl4gie_drop_path_add(const float* res, const float* t, const float* s, float* out, int B,
                                     long long per_sample, void* stream) {
    REQUIRE(res && t && s && out && B > 0 && per_sample > 0 && per_sample % 4 == 0);
    REQUIRE(!(((uintptr_t)res | (uintptr_t)t | (uintptr_t)out) & 15));
    const long long vps = per_sample / 4, nvec = vps * B;
    hipLaunchKernelGGL(drop_path_add_kernel, dim3(dp_blocks(nvec)), dim3(256), 0, (hipStream_t)stream, res, t, s, out,
                       nvec, vps);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int ssl4gie_drop_path_scale_cast(const float* dx, const float* s, void* out, int out_dtype, int B,
                                            long long per_sample, void* stream) {
    REQUIRE(dx && s && out && B > 0 && per_sample > 0 && per_sample % 4 == 0);
    REQUIRE(out_dtype == SSL4GIE_F32 || out_dtype == SSL4GIE_BF16);
    REQUIRE(!(((uintptr_t)dx | (uintptr_t)out) & 15));
    const long long vps = per_sample / 4, nvec = vps * B;
    hipStream_t st = (hipStream_t)stream;
    if (out_dtype == SSL4GIE_BF16)
        hipLaunchKernelGGL(drop_path_scale_cast_kernel<bf16_t>, dim3(dp_blocks(nvec)), dim3(256), 0, st, dx, s,
                           (bf16_t*)out, nvec, vps);
    else
        hipLaunchKernelGGL(drop_path_scale_cast_kernel<float>, dim3(dp_blocks(nvec)), dim3(256), 0, st, dx, s,
                           (float*)out, nvec, vps);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int ssl4gie_mixup(float* x, const float* lam, const int* box, const unsigned char* use_cutmix, int B, int C,
                             int H, int W, void* stream) {
    REQUIRE(x && lam && box && use_cutmix && B > 0 && C > 0 && H > 0 && W > 0);
    REQUIRE((long long)C * H * W <= 0x7fffffffLL);
    const bool vec = W % 4 == 0 && !((uintptr_t)x & 15);
    const long long per = (long long)C * H * (vec ? W / 4 : W);
    const dim3 grid((unsigned)((per + 255) / 256), (unsigned)((B + 1) / 2));
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(mixup_kernel<true>, grid, dim3(256), 0, st, x, lam, box, use_cutmix, B, C, H, W);
    else     hipLaunchKernelGGL(mixup_kernel<false>, grid, dim3(256), 0, st, x, lam, box, use_cutmix, B, C, H, W);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int ssl4gie_mixup_target(const long long* target, const float* lam, float* out, int B, int C,
                                    float on, float off, void* stream) {
    REQUIRE(target && lam && out && B > 0 && C > 0);
    const long long n = (long long)B * C;
    hipLaunchKernelGGL(mixup_target_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       target, lam, out, B, C, on, off);
    LAUNCH_CHECK();
    return 0;
}
