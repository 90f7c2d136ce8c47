// On-device RandAugment and RandomErasing of the MAE fine-tuning loader (Models/mae/util/datasets.py:37-48:
// timm.data.create_transform(auto_augment='rand-m9-mstd0.5-inc1', interpolation='bicubic', re_prob=0.25,
// re_mode='pixel', re_count=1)), on uint8 NHWC images [B, S, S, 3] — the bank's layout.  include/ssl4gie_hip.h states
// every rule; tests/randaug_checks.py restates them in numpy and holds them to PIL bit for bit.
//
//   ssl4gie_quantize_u8         fp32 NCHW crop in 0..255 units -> uint8 NHWC (clamp, + 0.5, truncate)
//   ssl4gie_randaug_layer       one RandAugment layer, one op id per sample: a histogram launch (R, G, B, L; only the
//                               samples whose op reads it) and an apply launch
//   ssl4gie_normalize_erase_u8  ToTensor + Normalize + RandomErasing in one pass, the noise a pure function of
//                               (seed, b, c, y, x)
//
// This object is built with -ffp-contract=off (the Makefile): the fp64 steps of the affine and the fp32 blend are
// rounded one by one, as PIL rounds them.  The one fused multiply-add, Normalize's, is written out.
//
// Work split of the two layer launches: a workgroup of 256 threads owns 256 UNITS of one sample, a unit being 16
// pixels = 48 bytes = three 16-byte chunks (S % 4 == 0, so a sample is a whole number of units).  The table ops walk
// the block's 768 chunks with neighbouring lanes on neighbouring chunks; the pixel ops give thread t unit t.
#include "map_chunk.h"
#include "reduce.h"

#define RA_THREADS 256
#define RA_MAX_S 2048   // 255 S^2 fits an int (the L sum of the contrast mean); grid.y = B <= 65535

enum { RA_AUTOCONTRAST = 0, RA_EQUALIZE, RA_INVERT, RA_ROTATE, RA_POSTERIZE, RA_SOLARIZE, RA_SOLARIZE_ADD, RA_COLOR,
       RA_CONTRAST, RA_BRIGHTNESS, RA_SHARPNESS, RA_SHEAR_X, RA_SHEAR_Y, RA_TRANSLATE_X, RA_TRANSLATE_Y, RA_N_OPS };

DEVI bool ra_needs_hist(int id) { return id == RA_AUTOCONTRAST || id == RA_EQUALIZE || id == RA_CONTRAST; }
DEVI bool ra_is_table(int id) {
    return id == RA_AUTOCONTRAST || id == RA_EQUALIZE || id == RA_INVERT || id == RA_POSTERIZE || id == RA_SOLARIZE ||
           id == RA_SOLARIZE_ADD || id == RA_CONTRAST || id == RA_BRIGHTNESS;
}
DEVI bool ra_is_gather(int id) { return id == RA_ROTATE || (id >= RA_SHEAR_X && id <= RA_TRANSLATE_Y); }

// byte k of 48 (k a constant after unrolling) of three 16-byte chunks
DEVI unsigned ra_get(const u32x4 (&w)[3], int k) { return (w[k >> 4][(k >> 2) & 3] >> (8 * (k & 3))) & 0xffu; }
DEVI void ra_put(u32x4 (&w)[3], int k, unsigned v) { w[k >> 4][(k >> 2) & 3] |= v << (8 * (k & 3)); }
DEVI unsigned ra_lum(unsigned r, unsigned g, unsigned b) { return (19595u * r + 38470u * g + 7471u * b + 0x8000u) >> 16; }
// 0 if t <= 0, 255 if t >= 255, else truncated (PIL's clip8; a NaN converts to 0)
DEVI unsigned ra_clip8(float t) { return t <= 0.f ? 0u : t >= 255.f ? 255u : (unsigned)(int)t; }
DEVI unsigned ra_clip8(double t) { return t <= 0.0 ? 0u : t >= 255.0 ? 255u : (unsigned)(int)t; }
// Image.blend(degenerate d, image v, f): fp32, the product and the sum rounded one by one
DEVI unsigned ra_blend(float d, float v, float f) { return ra_clip8(d + f * (v - d)); }

// ------------------------------------------------------------------ launch 1: R, G, B, L histograms
__global__ __launch_bounds__(RA_THREADS) void randaug_hist_kernel(const unsigned char* __restrict__ in,
                                                                  const unsigned char* __restrict__ op,
                                                                  int* __restrict__ hist, int S, int U) {
    __shared__ int h[4][256];
    const int b = blockIdx.y, t = threadIdx.x;
    if (!ra_needs_hist(op[b])) return;   // (uniform)
#pragma unroll
    for (int k = 0; k < 4; ++k) h[k][t] = 0;
    __syncthreads();
    const int u = blockIdx.x * RA_THREADS + t;
    if (u < U) {
        const u32x4* src = (const u32x4*)(in + (size_t)b * S * S * 3) + (size_t)u * 3;
        const u32x4 w[3] = {src[0], src[1], src[2]};
#pragma unroll
        for (int p = 0; p < 16; ++p) {
            const unsigned r = ra_get(w, 3 * p), g = ra_get(w, 3 * p + 1), bl = ra_get(w, 3 * p + 2);
            atomicAdd(&h[0][r], 1);
            atomicAdd(&h[1][g], 1);
            atomicAdd(&h[2][bl], 1);
            atomicAdd(&h[3][ra_lum(r, g, bl)], 1);
        }
    }
    __syncthreads();
    int* dst = hist + (size_t)b * 1024;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (h[k][t]) atomicAdd(dst + k * 256 + t, h[k][t]);
}

// ------------------------------------------------------------------ launch 2: the op
// PIL's BICUBIC macro, fp64
DEVI double ra_cubic(double v1, double v2, double v3, double v4, double d) {
    const double p1 = v2;
    const double p2 = -v1 + v3;
    const double p3 = 2 * (v1 - v2) + v3 - v4;
    const double p4 = -v1 + v2 - v3 + v4;
    return p1 + d * (p2 + d * (p3 + d * p4));
}

__global__ __launch_bounds__(RA_THREADS) void randaug_apply_kernel(
    const unsigned char* __restrict__ in, unsigned char* __restrict__ out, const unsigned char* __restrict__ op,
    const float* __restrict__ arg, const double* __restrict__ matrix, const int* __restrict__ hist, unsigned fill,
    int S, int U) {
    __shared__ unsigned char lut[3][256];
    __shared__ int hs[3][256];
    __shared__ int lohi[6];
    __shared__ int red[4];
    const int b = blockIdx.y, t = threadIdx.x;
    const int id = op[b];   // uniform over the workgroup: no branch below diverges
    const float a = arg[b];
    const unsigned char* src = in + (size_t)b * S * S * 3;
    unsigned char* dst = out + (size_t)b * S * S * 3;
    const int u = blockIdx.x * RA_THREADS + t;

    if (ra_is_table(id) || !(id == RA_COLOR || id == RA_SHARPNESS || ra_is_gather(id))) {
        const bool table = ra_is_table(id);
        if (table) {   // entry t of the three 256-entry tables
            unsigned e[3] = {(unsigned)t, (unsigned)t, (unsigned)t};
            if (id == RA_AUTOCONTRAST || id == RA_EQUALIZE) {
                const int* hb = hist + (size_t)b * 1024;
                if (t < 6) lohi[t] = t < 3 ? 256 : -1;
#pragma unroll
                for (int c = 0; c < 3; ++c) hs[c][t] = hb[c * 256 + t];
                __syncthreads();
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    if (hs[c][t]) {
                        atomicMin(&lohi[c], t);
                        atomicMax(&lohi[3 + c], t);
                    }
                __syncthreads();
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int lo = lohi[c], hi = lohi[3 + c];
                    if (hi <= lo) continue;   // at most one level: the identity
                    if (id == RA_AUTOCONTRAST) {
                        const double s = 255.0 / (double)(hi - lo);
                        const double o = (double)(-lo) * s;
                        const int v = (int)((double)t * s + o);
                        e[c] = (unsigned)min(255, max(0, v));
                    } else {
                        const int step = (S * S - hs[c][hi]) / 255;
                        if (step == 0) continue;
                        int n = step / 2;
                        for (int j = 0; j < t; ++j) n += hs[c][j];
                        e[c] = (unsigned)min(255, n / step);
                    }
                }
            } else if (id == RA_CONTRAST) {
                const int total = block_sum_all<SumOrder::Sequential>(t * hist[(size_t)b * 1024 + 768 + t], red);
                const int m = (int)((double)total / (double)(S * S) + 0.5);
                e[0] = e[1] = e[2] = ra_blend((float)m, (float)t, a);
            } else {
                unsigned v = (unsigned)t;
                const int n = (int)a;
                if (id == RA_INVERT) v = 255u - v;
                else if (id == RA_POSTERIZE) v = n >= 8 ? v : n <= 0 ? 0u : (v & ~((1u << (8 - n)) - 1u));
                else if (id == RA_SOLARIZE) v = t < n ? v : 255u - v;
                else if (id == RA_SOLARIZE_ADD) v = t < 128 ? (unsigned)min(255, t + n) & 0xffu : v;
                else v = ra_blend(0.f, (float)t, a);   // RA_BRIGHTNESS
                e[0] = e[1] = e[2] = v;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) lut[c][t] = (unsigned char)e[c];
            __syncthreads();
        }
        // the block's 768 chunks; byte j of chunk c is channel (16 c + j) % 3 = (c + j) % 3
        const int C3 = 3 * U;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int c = blockIdx.x * (3 * RA_THREADS) + i * RA_THREADS + t;
            if (c >= C3) continue;
            u32x4 w = ((const u32x4*)src)[c];
            if (table) {
                int ch = c % 3;
                u32x4 o = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    o[j >> 2] |= (unsigned)lut[ch][(w[j >> 2] >> (8 * (j & 3))) & 0xffu] << (8 * (j & 3));
                    ch = ch == 2 ? 0 : ch + 1;
                }
                w = o;
            }
            ((u32x4*)dst)[c] = w;   // not a table op: an id outside the table copies
        }
        return;
    }
    if (u >= U) return;
    const u32x4* s3 = (const u32x4*)src + (size_t)u * 3;
    u32x4 o[3] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
    if (id == RA_COLOR) {
        const u32x4 w[3] = {s3[0], s3[1], s3[2]};
#pragma unroll
        for (int p = 0; p < 16; ++p) {
            const unsigned r = ra_get(w, 3 * p), g = ra_get(w, 3 * p + 1), bl = ra_get(w, 3 * p + 2);
            const float L = (float)ra_lum(r, g, bl);
            ra_put(o, 3 * p, ra_blend(L, (float)r, a));
            ra_put(o, 3 * p + 1, ra_blend(L, (float)g, a));
            ra_put(o, 3 * p + 2, ra_blend(L, (float)bl, a));
        }
    } else if (id == RA_SHARPNESS) {
        // ImageFilter.SMOOTH on interior pixels: fp32 coefficients 1 / 13 and 5 / 13, the sum started at 0.5, the row
        // below first, three products per row added left to right; the one-pixel border is the source
        const float k1 = 1.f / 13.f, k5 = 5.f / 13.f;
        const u32x4 w[3] = {s3[0], s3[1], s3[2]};
        const int p0 = u * 16, y = p0 / S, x0 = p0 - y * S;   // 16 pixels of one unit may cross into the next row
#pragma unroll
        for (int p = 0; p < 16; ++p) {
            int xx = x0 + p, yy = y;
            while (xx >= S) { xx -= S; ++yy; }   // (S >= 4: at most four steps)
            const bool interior = xx >= 1 && xx < S - 1 && yy >= 1 && yy < S - 1;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const unsigned v = ra_get(w, 3 * p + c);
                unsigned d = v;
                if (interior) {
                    const unsigned char* q = src + ((size_t)yy * S + xx) * 3 + c;   // all nine taps lie inside
                    const int r = 3 * S;
                    float ss = 0.5f;
                    ss += ((float)q[r - 3] * k1 + (float)q[r] * k1) + (float)q[r + 3] * k1;
                    ss += ((float)q[-3] * k1 + (float)q[0] * k5) + (float)q[3] * k1;
                    ss += ((float)q[-r - 3] * k1 + (float)q[-r] * k1) + (float)q[-r + 3] * k1;
                    d = ra_clip8(ss);
                }
                ra_put(o, 3 * p + c, ra_blend((float)d, (float)v, a));
            }
        }
    } else {
        // Image.transform(AFFINE, BICUBIC, fillcolor), fp64.  The source coordinate is only COMPARED before it is
        // clamped: !(inside) fills, so a NaN or an enormous coefficient never reaches an address.
        const double* m = matrix + (size_t)b * 6;
        const double m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5];
        const double Sd = (double)S;
        const int p0 = u * 16, y = p0 / S, x0 = p0 - y * S;
        unsigned* d = (unsigned*)dst + (size_t)u * 12;
#pragma unroll 1
        for (int g = 0; g < 4; ++g) {   // 4 pixels = 12 bytes = three words at a time
            unsigned q[12];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                int xx = x0 + 4 * g + p, yy = y;
                while (xx >= S) { xx -= S; ++yy; }
                const double xc = (double)xx + 0.5, yc = (double)yy + 0.5;
                double xin = m0 * xc + m1 * yc + m2;
                double yin = m3 * xc + m4 * yc + m5;
                q[3 * p] = fill & 0xffu;
                q[3 * p + 1] = (fill >> 8) & 0xffu;
                q[3 * p + 2] = (fill >> 16) & 0xffu;
                if (xin >= 0.0 && xin < Sd && yin >= 0.0 && yin < Sd) {
                    xin -= 0.5;
                    yin -= 0.5;
                    const double fx = floor(xin), fy = floor(yin);
                    const double dx = xin - fx, dy = yin - fy;
                    const int ix = (int)fx, iy = (int)fy;   // in [-1, S - 1]
                    int xo[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) xo[k] = min(max(ix - 1 + k, 0), S - 1) * 3;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        double rows[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const unsigned char* r = src + (size_t)min(max(iy - 1 + j, 0), S - 1) * S * 3 + c;
                            rows[j] = ra_cubic((double)r[xo[0]], (double)r[xo[1]], (double)r[xo[2]], (double)r[xo[3]], dx);
                        }
                        q[3 * p + c] = ra_clip8(ra_cubic(rows[0], rows[1], rows[2], rows[3], dy));
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) d[3 * g + k] = q[4 * k] | q[4 * k + 1] << 8 | q[4 * k + 2] << 16 | q[4 * k + 3] << 24;
        }
        return;
    }
    u32x4* d3 = (u32x4*)dst + (size_t)u * 3;
    d3[0] = o[0];
    d3[1] = o[1];
    d3[2] = o[2];
}

extern "C" size_t ssl4gie_randaug_layer_workspace_bytes(int B) {
    return B > 0 ? align256((size_t)B * 4 * 256 * sizeof(int)) : 0;
}

extern "C" int ssl4gie_randaug_layer(const unsigned char* in, unsigned char* out, const unsigned char* op,
                                     const float* arg, const double* matrix, const unsigned char* fill,
                                     void* workspace, int B, int S, void* stream) {
    REQUIRE(in && out && op && arg && matrix && fill && in != out);
    REQUIRE(B >= 0 && B <= 65535 && S >= 4 && S % 4 == 0 && S <= RA_MAX_S);
    REQUIRE(is16(in) && is16(out) && ((uintptr_t)matrix & 7) == 0);
    if (B == 0) return 0;
    REQUIRE(workspace && is16(workspace));
    hipStream_t st = (hipStream_t)stream;
    const int U = S * S / 16;
    const dim3 grid(blocks_of(U), (unsigned)B);
    HIP_RET(hipMemsetAsync(workspace, 0, (size_t)B * 4 * 256 * sizeof(int), st));
    hipLaunchKernelGGL(randaug_hist_kernel, grid, dim3(RA_THREADS), 0, st, in, op, (int*)workspace, S, U);
    LAUNCH_CHECK();
    const unsigned f = (unsigned)fill[0] | (unsigned)fill[1] << 8 | (unsigned)fill[2] << 16;
    hipLaunchKernelGGL(randaug_apply_kernel, grid, dim3(RA_THREADS), 0, st, in, out, op, arg, matrix,
                       (const int*)workspace, f, S, U);
    LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------ quantize
// one thread per 4 pixels: three 16-byte loads (one per channel plane), 12 bytes out
__global__ void quantize_u8_kernel(const float* __restrict__ x, unsigned char* __restrict__ out, int HW,
                                   long long total4) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total4) return;
    const long long b = idx / (HW / 4);
    const int p = (int)(idx - b * (HW / 4)) * 4;
    unsigned q[12];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const f32x4 v = ld4(x + ((size_t)b * 3 + c) * HW + p);
#pragma unroll
        for (int j = 0; j < 4; ++j) q[3 * j + c] = (unsigned)(int)(fminf(fmaxf(v[j], 0.f), 255.f) + 0.5f);   // NaN -> 0
    }
    unsigned* dst = (unsigned*)(out + ((size_t)b * HW + p) * 3);
#pragma unroll
    for (int k = 0; k < 3; ++k) dst[k] = q[4 * k] | q[4 * k + 1] << 8 | q[4 * k + 2] << 16 | q[4 * k + 3] << 24;
}

extern "C" int ssl4gie_quantize_u8(const float* x, unsigned char* out, int B, int S, void* stream) {
    REQUIRE(x && out && B >= 0 && S >= 4 && S % 4 == 0 && S <= 16384 && is16(x) && ((uintptr_t)out & 3) == 0);
    if (B == 0) return 0;
    const int HW = S * S;
    const long long total4 = (long long)B * (HW / 4);
    REQUIRE((total4 + 255) / 256 <= 0x7fffffffLL);
    hipLaunchKernelGGL(quantize_u8_kernel, dim3(blocks_of(total4)), dim3(256), 0, (hipStream_t)stream, x, out, HW,
                       total4);
    LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------ normalize + erase
// Philox4x32-10 (Salmon, Moraes, Dror, Shaw 2011): counter (x, y, c, b), key (seed low word, seed high word).  The
// two uniforms are the top 24 bits of output words 0 and 1: u = (k + 1) 2^-24 in (0, 1], exact in fp32.
DEVI float ra_noise(unsigned k0, unsigned k1, unsigned x, unsigned y, unsigned c, unsigned b) {
    unsigned c0 = x, c1 = y, c2 = c, c3 = b;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const unsigned h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    const float u1 = (float)((c0 >> 8) + 1u) * 5.9604644775390625e-8f;
    const float u2 = (float)((c1 >> 8) + 1u) * 5.9604644775390625e-8f;
    return sqrtf(-2.f * logf(u1)) * cosf(6.2831855f * u2);   // Box-Muller, fp32
}

__global__ void normalize_erase_u8_kernel(const unsigned char* __restrict__ img, float* __restrict__ out, f32x4 scale,
                                          f32x4 shift, const int* __restrict__ box, int mode, unsigned k0, unsigned k1,
                                          int S, long long total4) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total4) return;
    const int HW = S * S;
    const long long b = idx / (HW / 4);
    const int p = (int)(idx - b * (HW / 4)) * 4;
    const int y = p / S, x = p - y * S;   // S % 4 == 0: the 4 pixels share a row
    // the box is compared with coordinates and with S, and used for nothing else
    const int top = box[4 * b], left = box[4 * b + 1], h = box[4 * b + 2], w = box[4 * b + 3];
    const bool ok = top >= 0 && left >= 0 && h >= 0 && w >= 0 && (long long)top + h <= S && (long long)left + w <= S;
    const bool row_in = ok && h > 0 && w > 0 && y >= top && y < top + h;
    const unsigned* src = (const unsigned*)(img + ((size_t)b * HW + p) * 3);  // 12 bytes, 4-B aligned
    const unsigned w0 = src[0], w1 = src[1], w2 = src[2];
    unsigned px[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) { px[j] = (w0 >> (8 * j)) & 0xff; px[4 + j] = (w1 >> (8 * j)) & 0xff; px[8 + j] = (w2 >> (8 * j)) & 0xff; }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = __builtin_fmaf((float)px[3 * j + c], scale[c], shift[c]);   // ssl4gie_normalize_u8's bits
            if (!ok) v[j] = NAN;
            else if (row_in && x + j >= left && x + j < left + w)
                v[j] = mode == SSL4GIE_ERASE_CONST ? 0.f
                     : mode == SSL4GIE_ERASE_RAND ? ra_noise(k0, k1, 0u, 0u, (unsigned)c, (unsigned)b)
                     : ra_noise(k0, k1, (unsigned)(x + j), (unsigned)y, (unsigned)c, (unsigned)b);
        }
        st4(out + ((size_t)b * 3 + c) * HW + p, v);
    }
}

extern "C" int ssl4gie_normalize_erase_u8(const unsigned char* img, float* out, const float* mean, const float* std,
                                          const int* box, int mode, unsigned long long seed, int B, int S,
                                          void* stream) {
    REQUIRE(img && out && mean && std && box && B >= 0 && S >= 4 && S % 4 == 0 && S <= 16384);
    REQUIRE(mode == SSL4GIE_ERASE_CONST || mode == SSL4GIE_ERASE_RAND || mode == SSL4GIE_ERASE_PIXEL);
    REQUIRE(((uintptr_t)img & 3) == 0 && is16(out));
    for (int c = 0; c < 3; ++c) REQUIRE(std[c] > 0.f);
    if (B == 0) return 0;
    const long long total4 = (long long)B * (S * S / 4);
    REQUIRE((total4 + 255) / 256 <= 0x7fffffffLL);
    const f32x4 scale = {1.f / (255.f * std[0]), 1.f / (255.f * std[1]), 1.f / (255.f * std[2]), 0.f};
    const f32x4 shift = {-mean[0] / std[0], -mean[1] / std[1], -mean[2] / std[2], 0.f};
    hipLaunchKernelGGL(normalize_erase_u8_kernel, dim3(blocks_of(total4)), dim3(256), 0, (hipStream_t)stream, img, out,
                       scale, shift, box, mode, (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32), S, total4);
    LAUNCH_CHECK();
    return 0;
}
