// On-device colour augmentation: the colour half of MoCo-v3's two-view recipe (Models/moco_v3/main_moco.py:262-285,
// moco/loader.py:26-42) on fp32 [B, 3, S, S] images in [0, 1], with the per-sample parameters already drawn:
//   RandomApply(ColorJitter) -> RandomGrayscale -> GaussianBlur -> Solarize -> Normalize.
// The reference flips AFTER the colour transforms; here crop and flip have already happened in
// ssl4gie_view_sample_u8.  Every colour op below is pointwise or a symmetric stencil (symmetric weights, symmetric
// edge rule), so it commutes with a left-right mirror: flipping first gives the same image.
//
// The rule, per sample b, on x = clamp(input, 0, 1), three channels per pixel:
//   1. jitter: order[b][0..3] are op ids applied left to right (an id above 3 is a skip; 255 is the skip the host
//      writes; an id appears at most once).  blend(a, d, f) = clamp(f a + (1 - f) d, 0, 1), gray(x) = 0.299 r +
//      0.587 g + 0.114 b (PIL's "L" weights), f = factors[b][id]:
//        0 brightness  blend(x, 0, f)
//        1 contrast    blend(x, m, f), m = mean of gray over the sample's whole image AFTER the ops before contrast
//        2 saturation  blend(x, gray(x), f)
//        3 hue         rgb -> hsv, h <- (h + f) mod 1, hsv -> rgb: the colorsys formulas in floating point as
//                      torchvision's tensor path writes them, p, q, t clamped to [0, 1]; max == min keeps its value
//   2. flags[b] & 1: r, g, b <- gray(x)
//   3. sigma[b] > 0: separable true Gaussian, R = min(ceil(3 sigma), 6) (sigma taken as the fp32 value it is),
//      weights exp(-k^2 / 2 sigma^2), k in [-R, R], over their sum; horizontal pass, then vertical pass; symmetric
//      edges (index -1 - i reads i, S + i reads S - 1 - i)
//   4. flags[b] & 2: x >= 128 / 255 -> 1 - x  (ImageOps.solarize, threshold 128)
//   5. (x - mean[c]) / std[c]
// No rounding to integer levels between the ops.
//
// ssl4gie_color_augment_ft is the colour stage of the finetune loaders (Binary_segmentation/Data/dataloaders.py:62-71,
// Classification/Data/dataloaders.py:62-66: ColorJitter -> GaussianBlur((25, 25), sigma) -> ToTensor -> Normalize):
// the same rule with step 3 replaced by
//   3'. sigma[b] > 0: separable 25-tap Gaussian, k in [-12, 12], weights exp(-k^2 / 2 sigma^2) over the sum of all 25;
//       horizontal pass, then vertical pass; reflect edges (index -i reads i, S - 1 + i reads S - 1 - i) — what
//       transforms.GaussianBlur((25, 25)) computes on its tensor path.  The tap loop stops at R = ceil(6 sigma)
//       rounded up to even, at most 12: a dropped tap weighs less than exp(-18) = 1.6e-8 of the centre's, and all of
//       them together less than 4e-9 of the sum, a fifteenth of an fp32 ulp of the [0, 1] result.  sigma < 1 / 16: every
//       weight but the centre's is 0 in fp32, and the sample takes the no-blur path.
// It is the same two kernels: color_apply_kernel is a template over (largest radius, edge rule, radius rule).
//
// Two launches:
//   color_stats_kernel  sample x chunk of the image.  A sample without a contrast op exits at once; otherwise the
//       workgroup applies the ops that precede contrast, sums gray (per lane, wave shuffles, LDS, one lane in wave
//       order) and writes ONE partial to workspace[b][chunk].  No atomics.
//   color_apply_kernel  sample x tile.  Sums the sample's partials in chunk order (bit-identical from run to run, and
//       independent of the sample's place in the batch: the chunking depends on S alone).
//       sigma == 0: pointwise, registers only: 16-byte loads, the ops, 16-byte stores.
//       sigma > 0: the tile plus a halo of THIS sample's R rows and R (rounded up to 4) columns goes through the
//       jitter and grayscale into LDS — halo pixels are recomputed, pointwise ops cost less than a second pass over
//       HBM —, the horizontal pass writes a second LDS tile, the vertical pass reads it, solarizes, normalises and
//       stores 16 bytes per lane.  The image is read once (the halo out of L2) and written once.
// Tile geometry: CA_TILE_H rows x 56 columns at S = 224 (48 / 56 / 64 columns, whichever pads S least), 512 threads;
// LDS for R = 6 is 3 (CA_TILE_H + 12) (2 W + 16) floats = 67.6 KB at 32 x 56: two workgroups per CU (what it was
// measured against: the note at CA_TILE_H).  The finetune rule's R = 12: 3 (CA_FT_TILE_H + 24) (2 W + 24) floats =
// 91.4 KB at 32 x 56, one workgroup per CU (the note at CA_FT_TILE_H).
#include "common.h"
#include "ssl4gie_hip.h"

#define CA_THREADS 512
#define CA_STAT_THREADS 256
#define CA_RMAX 6
#define CA_RPAD 8  // CA_RMAX rounded up to the 4-column groups the tiles are loaded and read in
// Rows of a tile.  Measured on an MI355X at B = 256, S = 224 (tools/time_color_augment.py, medians of 50): 32 x 56
// tiles (67.6 KB of LDS, 2 workgroups per CU, 12 halo rows on 32 at R = 6) against 16 x 56 (43 KB, 3 per CU, 12 on
// 16): view-1 recipe 246 against 253 us, sigma = 2 on every sample 274 against 281, the pointwise path 97 against
// 104 — the third workgroup per CU does not pay for the doubled halo share; 32 it is.
#ifndef CA_TILE_H
#define CA_TILE_H 32
#endif
#define CA_FT_RMAX 12  // the 25-tap blur of the finetune loaders; a multiple of 4 already
// Rows of a tile of the finetune rule (halo of up to 12 rows).  Measured on an MI355X at B = 128, S = 224
// (tools/time_finetune_augment.py --part ab, medians of 50): 32 x 56 tiles (91.4 KB of LDS, one workgroup per CU, 24
// halo rows on 32 at R = 12) against 16 x 56 (65.3 KB, two per CU, 24 on 16): segmentation recipe 235 against 302 us,
// sigma = 2 on every sample 277 against 378 — the second workgroup per CU does not pay for the doubled halo share
// (the jitter is recomputed on the halo); 32 it is.
#ifndef CA_FT_TILE_H
#define CA_FT_TILE_H 32
#endif
#define CA_SKIP 255

struct CaSample {
    float f[4];  // factor of slot i
    int op[4];   // op id of slot i, CA_SKIP for none
    int flags;
    float sigma;
};

DEVI CaSample ca_sample(const float* __restrict__ factors, const unsigned char* __restrict__ order,
                        const unsigned char* __restrict__ flags, const float* __restrict__ sigma, int b) {
    CaSample s;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int id = order[4 * b + i];
        s.op[i] = id <= 3 ? id : CA_SKIP;
        s.f[i] = id <= 3 ? factors[4 * b + id] : 1.f;
    }
    s.flags = flags[b];
    s.sigma = sigma[b];
    return s;
}
// slot of the contrast op, 4 when there is none
DEVI int ca_contrast_slot(const CaSample& s) {
    int slot = 4;
#pragma unroll
    for (int i = 3; i >= 0; --i) slot = s.op[i] == 1 ? i : slot;
    return slot;
}

DEVI float ca_sat(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
DEVI float ca_gray(float r, float g, float b) { return 0.299f * r + 0.587f * g + 0.114f * b; }
DEVI float ca_blend(float a, float d, float f) { return ca_sat(f * a + (1.f - f) * d); }

DEVI void ca_hue(float& r, float& g, float& b, float shift) {
    const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
    const float cr = maxc - minc;
    const bool flat = cr == 0.f;  // keeps its value (maxc == 0 is flat too: no division by zero below)
    const float s = cr / (flat ? 1.f : maxc);
    const float inv = 1.f / (flat ? 1.f : cr);
    const float rc = (maxc - r) * inv, gc = (maxc - g) * inv, bc = (maxc - b) * inv;
    float h = maxc == r ? bc - gc : maxc == g ? 2.f + rc - bc : 4.f + gc - rc;
    h = h / 6.f + 1.f;
    h -= floorf(h);  // fmod(h, 1), h > 0
    h += shift;
    h -= floorf(h);  // Python's mod: [0, 1]
    const float h6 = h * 6.f, fl = floorf(h6), fr = h6 - fl;
    int i = (int)fl;
    i = i >= 6 ? i - 6 : i;
    const float v = maxc;
    const float p = ca_sat(v * (1.f - s)), q = ca_sat(v * (1.f - fr * s)), t = ca_sat(v * (1.f - (1.f - fr) * s));
    const float nr = i == 0 || i == 5 ? v : i == 1 ? q : i == 4 ? t : p;
    const float ng = i == 0 ? t : i == 1 || i == 2 ? v : i == 3 ? q : p;
    const float nb = i == 0 || i == 1 ? p : i == 2 ? t : i == 5 ? q : v;
    r = flat ? r : nr;
    g = flat ? g : ng;
    b = flat ? b : nb;
}

// slots [0, n) of the sample's order on one pixel (op ids are uniform over the workgroup)
DEVI void ca_jitter(const CaSample& s, int n, float m, float& r, float& g, float& b) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i >= n) break;
        const float f = s.f[i];
        switch (s.op[i]) {
        case 0:
            r = ca_sat(f * r), g = ca_sat(f * g), b = ca_sat(f * b);
            break;
        case 1:
            r = ca_blend(r, m, f), g = ca_blend(g, m, f), b = ca_blend(b, m, f);
            break;
        case 2: {
            const float y = ca_gray(r, g, b);
            r = ca_blend(r, y, f), g = ca_blend(g, y, f), b = ca_blend(b, y, f);
            break;
        }
        case 3:
            ca_hue(r, g, b, f);
            break;
        default:
            break;
        }
    }
}

// steps 1 and 2 of the rule on four neighbouring pixels
DEVI void ca_point4(const CaSample& s, float m, f32x4& r, f32x4& g, f32x4& b) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float pr = ca_sat(r[j]), pg = ca_sat(g[j]), pb = ca_sat(b[j]);
        ca_jitter(s, 4, m, pr, pg, pb);
        if (s.flags & 1) pr = pg = pb = ca_gray(pr, pg, pb);
        r[j] = pr, g[j] = pg, b[j] = pb;
    }
}
// steps 4 and 5
DEVI f32x4 ca_finish4(f32x4 v, bool solarize, float sc, float sh) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float u = solarize && v[j] >= 128.f / 255.f ? 1.f - v[j] : v[j];
        v[j] = u * sc + sh;
    }
    return v;
}
DEVI int ca_mirror(int i, int S) { return i < 0 ? -1 - i : i >= S ? 2 * S - 1 - i : i; }
DEVI int ca_reflect(int i, int S) { return i < 0 ? -i : i >= S ? 2 * S - 2 - i : i; }

static int ca_chunks(int S) {  // of the statistics pass: about a thousand 4-pixel groups each, S alone decides
    const long long G = (long long)S * S / 4;
    long long c = G / 1024;
    return (int)(c < 1 ? 1 : c > 64 ? 64 : c);
}
static int ca_tile_w(int S) {
    if (S <= 64) return S;
    int best = 64;
    for (int w = 64; w >= 48; w -= 8)
        if ((S + w - 1) / w * w - S < (S + best - 1) / best * best - S) best = w;
    return best;
}

__global__ __launch_bounds__(CA_STAT_THREADS) void color_stats_kernel(
    const float* __restrict__ x, const float* __restrict__ factors, const unsigned char* __restrict__ order,
    const unsigned char* __restrict__ flags, const float* __restrict__ sigma, float* __restrict__ partial, int S,
    int chunks, int per_chunk) {
    __shared__ float wsum[CA_STAT_THREADS / 64];
    const int b = blockIdx.x / chunks, c = blockIdx.x - b * chunks, t = threadIdx.x;
    const CaSample s = ca_sample(factors, order, flags, sigma, b);
    const int n = ca_contrast_slot(s);
    if (n == 4) return;  // (uniform) nobody reads this sample's partials
    const int G = S * S / 4, g0 = c * per_chunk, g1 = min(G, g0 + per_chunk);
    const size_t plane = (size_t)S * S;
    const float* src = x + (size_t)b * 3 * plane;
    float sum = 0.f;
    for (int g = g0 + t; g < g1; g += CA_STAT_THREADS) {
        const f32x4 r = ld4(src + 4 * (size_t)g), gg = ld4(src + plane + 4 * (size_t)g),
                    bb = ld4(src + 2 * plane + 4 * (size_t)g);
        float y[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float pr = ca_sat(r[j]), pg = ca_sat(gg[j]), pb = ca_sat(bb[j]);
            ca_jitter(s, n, 0.f, pr, pg, pb);
            y[j] = ca_gray(pr, pg, pb);
        }
        sum += (y[0] + y[1]) + (y[2] + y[3]);
    }
    sum = wave_sum(sum);
    if ((t & 63) == 0) wsum[t >> 6] = sum;
    __syncthreads();
    if (t == 0) {
        float tot = 0.f;
        for (int w = 0; w < CA_STAT_THREADS / 64; ++w) tot += wsum[w];
        partial[(size_t)b * chunks + c] = tot;
    }
}

// The two blur passes of one tile.  A [3][AH][AW]: the tile's pixels after steps 1-2, rows y0 - R .., columns
// x0 - RP .. (RP = R rounded up to 4); T [3][AH][TW]: after the horizontal pass.  nro x nco outputs.
template <int R>
DEVI void ca_blur_store(const float* A, float* T, const float* wl, int AH, int AW, int TW, int nro, int nco,
                        float* dst, int S, bool solarize, f32x4 nscale, f32x4 nshift) {
    constexpr int RP = (R + 3) & ~3, NV = (2 * RP + 4) / 4;
    const int t = threadIdx.x;
    float w[R + 1];
#pragma unroll
    for (int k = 0; k <= R; ++k) w[k] = wl[k];
    const int ng = nco >> 2, nra = nro + 2 * R;
    for (int i = t; i < 3 * nra * ng; i += CA_THREADS) {
        const int g = i % ng, q = i / ng, ar = q % nra, ch = q / nra;
        const float* row = A + ((size_t)ch * AH + ar) * AW + 4 * g;
        float v[4 * NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const f32x4 u = ld4(row + 4 * j);
            v[4 * j] = u[0], v[4 * j + 1] = u[1], v[4 * j + 2] = u[2], v[4 * j + 3] = u[3];
        }
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float acc = 0.f;
#pragma unroll
            for (int k = -R; k <= R; ++k) acc += w[k < 0 ? -k : k] * v[RP + j + k];
            o[j] = acc;
        }
        st4(T + ((size_t)ch * AH + ar) * TW + 4 * g, o);
    }
    __syncthreads();
    for (int i = t; i < 3 * nro * ng; i += CA_THREADS) {
        const int g = i % ng, q = i / ng, orow = q % nro, ch = q / nro;
        const float* col = T + ((size_t)ch * AH + orow) * TW + 4 * g;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = -R; k <= R; ++k) acc += w[k < 0 ? -k : k] * ld4(col + (size_t)(R + k) * TW);
        const float sc = ch == 0 ? nscale[0] : ch == 1 ? nscale[1] : nscale[2];
        const float sh = ch == 0 ? nshift[0] : ch == 1 ? nshift[1] : nshift[2];
        st4(dst + ((size_t)ch * S + orow) * S + 4 * g, ca_finish4(acc, solarize, sc, sh));
    }
}

// FT = false: the MoCo rule (R = ceil(3 sigma) <= 6, weights over the sum of the taps kept, symmetric edges);
// FT = true: the finetune rule (25 taps, weights over the sum of all 25, reflect edges).
template <bool FT>
__global__ __launch_bounds__(CA_THREADS) void color_apply_kernel(
    const float* __restrict__ x, float* __restrict__ out, const float* __restrict__ factors,
    const unsigned char* __restrict__ order, const unsigned char* __restrict__ flags,
    const float* __restrict__ sigma, const float* __restrict__ partial, int S, int chunks, int TW, int TH,
    int tiles_x, int tiles, f32x4 nscale, f32x4 nshift) {
    constexpr int RMAX = FT ? CA_FT_RMAX : CA_RMAX, RPAD = FT ? CA_FT_RMAX : CA_RPAD;
    extern __shared__ __attribute__((aligned(16))) float ca_lds[];
    __shared__ float wl[RMAX + 1];
    const int t = threadIdx.x;
    const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
    const int ty = tile / tiles_x, y0 = ty * TH, x0 = (tile - ty * tiles_x) * TW;
    const int nro = min(TH, S - y0), nco = min(TW, S - x0), ng = nco >> 2;
    const size_t plane = (size_t)S * S;
    const float* src = x + (size_t)b * 3 * plane;
    float* dst = out + (size_t)b * 3 * plane + (size_t)y0 * S + x0;

    const CaSample s = ca_sample(factors, order, flags, sigma, b);
    float m = 0.f;
    if (ca_contrast_slot(s) < 4) {  // (uniform) the partials in chunk order
        for (int c = 0; c < chunks; ++c) m += partial[(size_t)b * chunks + c];
        m /= (float)plane;
    }
    const bool solarize = (s.flags & 2) != 0;

    // (uniform) no halo, no LDS.  Under the finetune rule a sigma below 1 / 16 is no blur either: every weight but the
    // centre's is below exp(-128) of it, 0 in fp32 (the reference's range starts at 0.001)
    if (!(s.sigma > (FT ? 0.0625f : 0.f))) {
        for (int i = t; i < nro * ng; i += CA_THREADS) {
            const int g = i % ng, orow = i / ng;
            const size_t o = (size_t)(y0 + orow) * S + x0 + 4 * g;
            f32x4 r = ld4(src + o), gg = ld4(src + plane + o), bb = ld4(src + 2 * plane + o);
            ca_point4(s, m, r, gg, bb);
            float* d = dst + (size_t)orow * S + 4 * g;
            st4(d, ca_finish4(r, solarize, nscale[0], nshift[0]));
            st4(d + plane, ca_finish4(gg, solarize, nscale[1], nshift[1]));
            st4(d + 2 * plane, ca_finish4(bb, solarize, nscale[2], nshift[2]));
        }
        return;
    }

    // ceil(3 sigma) in fp64: the product is exact there, in fp32 it can round down onto an integer
    const double r3 = ceil((FT ? 6.0 : 3.0) * (double)s.sigma);
    int R = r3 < (double)RMAX ? (int)r3 : RMAX;  // >= 1; +inf clamps
    if (FT) R = (R + 1) & ~1;                    // even radii only: half the instantiations, a tap of weight ~0 more
    const int RP = (R + 3) & ~3;
    if (t <= RMAX) {
        const double inv2 = 0.5 / ((double)s.sigma * (double)s.sigma);
        double sum = 1.0;
        for (int k = 1; k <= (FT ? RMAX : R); ++k) sum += 2.0 * exp(-(double)(k * k) * inv2);
        wl[t] = t <= R ? (float)(exp(-(double)(t * t) * inv2) / sum) : 0.f;
    }
    const int AH = TH + 2 * RMAX, AW = TW + 2 * RPAD;
    float* A = ca_lds;                   // [3][AH][AW]
    float* T = A + (size_t)3 * AH * AW;  // [3][AH][TW]
    const int nra = nro + 2 * R, nga = (nco + 2 * RP) >> 2;
    for (int i = t; i < nra * nga; i += CA_THREADS) {
        const int ag = i % nga, ar = i / nga;
        const int y = FT ? ca_reflect(y0 - R + ar, S) : ca_mirror(y0 - R + ar, S), c0 = x0 - RP + 4 * ag;
        const float* p = src + (size_t)y * S;
        f32x4 r, gg, bb;
        if (c0 >= 0 && c0 < S) {  // S and c0 are multiples of 4: a group is inside the row or outside it
            r = ld4(p + c0), gg = ld4(p + plane + c0), bb = ld4(p + 2 * plane + c0);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                // c0 + j overshoots by at most 8 <= S (symmetric), by at most 12 < S (reflect)
                const int c = FT ? ca_reflect(c0 + j, S) : ca_mirror(c0 + j, S);
                r[j] = p[c], gg[j] = p[plane + c], bb[j] = p[2 * plane + c];
            }
        }
        ca_point4(s, m, r, gg, bb);
        float* a = A + (size_t)ar * AW + 4 * ag;
        st4(a, r);
        st4(a + (size_t)AH * AW, gg);
        st4(a + (size_t)2 * AH * AW, bb);
    }
    __syncthreads();
    if (FT) {
        switch (R) {  // (uniform)
        case 2: ca_blur_store<2>(A, T, wl, AH, AW, TW, nro, nco, dst, S, solarize, nscale, nshift); break;
        case 4: ca_blur_store<4>(A, T, wl, AH, AW, TW, nro, nco, dst, S, solarize, nscale, nshift); break;
        case 6: ca_blur_store<6>(A, T, wl, AH, AW, TW, nro, nco, dst, S, solarize, nscale, nshift); break;
        case 8: ca_blur_store<8>(A, T, wl, AH, AW, TW, nro, nco, dst, S, solarize, nscale, nshift); break;
        case 10: ca_blur_store<10>(A, T, wl, AH, AW, TW, nro, nco, dst, S, solarize, nscale, nshift); break;
        default: ca_blur_store<12>(A, T, wl, AH, AW, TW, nro, nco, dst, S, solarize, nscale, nshift); break;
        }
        return;
    }
    switch (R) {  // (uniform)
    case 1: ca_blur_store<1>(A, T, wl, AH, AW, TW, nro, nco, dst, S, solarize, nscale, nshift); break;
    case 2: ca_blur_store<2>(A, T, wl, AH, AW, TW, nro, nco, dst, S, solarize, nscale, nshift); break;
    case 3: ca_blur_store<3>(A, T, wl, AH, AW, TW, nro, nco, dst, S, solarize, nscale, nshift); break;
    case 4: ca_blur_store<4>(A, T, wl, AH, AW, TW, nro, nco, dst, S, solarize, nscale, nshift); break;
    case 5: ca_blur_store<5>(A, T, wl, AH, AW, TW, nro, nco, dst, S, solarize, nscale, nshift); break;
    default: ca_blur_store<6>(A, T, wl, AH, AW, TW, nro, nco, dst, S, solarize, nscale, nshift); break;
    }
}

static bool ca_shape_ok(int B, int S) { return B >= 1 && S >= 8 && S % 4 == 0; }

extern "C" size_t ssl4gie_color_augment_workspace_bytes(int B, int S) {
    if (!ca_shape_ok(B, S)) return 0;
    return sizeof(float) * (size_t)B * ca_chunks(S);
}

template <bool FT>
static int ca_launch(const float* x, float* out, int B, int S, const float* factors, const unsigned char* order,
                     const unsigned char* flags, const float* sigma, const float* mean, const float* std,
                     void* workspace, size_t workspace_bytes, void* stream) {
    constexpr int RMAX = FT ? CA_FT_RMAX : CA_RMAX, RPAD = FT ? CA_FT_RMAX : CA_RPAD;
    constexpr int TILE_H = FT ? CA_FT_TILE_H : CA_TILE_H;
    REQUIRE(x && out && factors && order && flags && sigma && mean && std && workspace);
    REQUIRE(ca_shape_ok(B, S));
    if (FT) REQUIRE(S >= 16);  // a reflect halo of 12 needs S > 12
    for (int c = 0; c < 3; ++c) REQUIRE(std[c] != 0.f);
    REQUIRE((const void*)x != (const void*)out);  // the stencil reads its neighbours' inputs
    REQUIRE(((uintptr_t)x | (uintptr_t)out) % 16 == 0);  // 16-byte loads and stores
    REQUIRE(workspace_bytes >= ssl4gie_color_augment_workspace_bytes(B, S));
    const int chunks = ca_chunks(S);
    const int G = (int)((long long)S * S / 4), per_chunk = (G + chunks - 1) / chunks;
    const int TW = ca_tile_w(S), TH = S < TILE_H ? S : TILE_H;
    const int tiles_x = (S + TW - 1) / TW, tiles = tiles_x * ((S + TH - 1) / TH);
    REQUIRE((long long)S * S <= 0x7fffffffLL && (long long)B * tiles <= 0x7fffffffLL &&
            (long long)B * chunks <= 0x7fffffffLL);
    const size_t lds = sizeof(float) * 3 * (size_t)(TH + 2 * RMAX) * (size_t)(2 * TW + 2 * RPAD);
    static bool attr = false;  // one per instantiation
    if (!attr) {
        HIP_RET(hipFuncSetAttribute((const void*)color_apply_kernel<FT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(sizeof(float) * 3 * (TILE_H + 2 * RMAX) * (2 * 64 + 2 * RPAD))));
        attr = true;
    }
    hipLaunchKernelGGL(color_stats_kernel, dim3((unsigned)(B * chunks)), dim3(CA_STAT_THREADS), 0,
                       (hipStream_t)stream, x, factors, order, flags, sigma, (float*)workspace, S, chunks, per_chunk);
    LAUNCH_CHECK();
    const f32x4 nscale = {1.f / std[0], 1.f / std[1], 1.f / std[2], 0.f};
    const f32x4 nshift = {-mean[0] / std[0], -mean[1] / std[1], -mean[2] / std[2], 0.f};
    hipLaunchKernelGGL(color_apply_kernel<FT>, dim3((unsigned)(B * tiles)), dim3(CA_THREADS), lds,
                       (hipStream_t)stream, x, out, factors, order, flags, sigma, (const float*)workspace, S, chunks,
                       TW, TH, tiles_x, tiles, nscale, nshift);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int ssl4gie_color_augment(const float* x, float* out, int B, int S, const float* factors,
                                     const unsigned char* order, const unsigned char* flags, const float* sigma,
                                     const float* mean, const float* std, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    return ca_launch<false>(x, out, B, S, factors, order, flags, sigma, mean, std, workspace, workspace_bytes, stream);
}

extern "C" int ssl4gie_color_augment_ft(const float* x, float* out, int B, int S, const float* factors,
                                        const unsigned char* order, const unsigned char* flags, const float* sigma,
                                        const float* mean, const float* std, void* workspace, size_t workspace_bytes,
                                        void* stream) {
    return ca_launch<true>(x, out, B, S, factors, order, flags, sigma, mean, std, workspace, workspace_bytes, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// Detection input pipeline (Object_detection/Data/dataloaders.py:75-112, Data/dataset.py:38-113) over a RAGGED uint8
// bank: images of different sizes in one flat buffer, image i = HWC bytes at pixels + offsets[i], sizes[i] = (H0, W0).
//   det_color_stats_kernel / det_color_apply_kernel   ColorJitter -> GaussianBlur((25, 25)) on the H0 x W0 rectangle of
//       index[b]: steps 1 and 3' of the rule at the top of this file with H0 and W0 in S's place on the two axes, on
//       x = float(v) / 255 (a true division: ToTensor's value), no grayscale, solarize or normalisation.  Reads the
//       bank, writes fp32 planar scratch [B][3][plane_stride], row pitch W0.  The same two-launch shape as the square
//       stage: per-chunk partial sums of the contrast mean in a fixed order, then tiles with a jittered halo in LDS.
//   det_geometry_kernel   rot90 / hflip / vflip (one index map), the antialiased bicubic halving when a side exceeds
//       F, the centre pad to F x F and (x - mean) / std, from the scratch (training) or from the bank itself (eval).
//   det_boxes_kernel      the boxes of the batch through the same decisions, in the reference's order of fp32 operations.
// A sample is refused by ALL kernels on the same test (det_sample): index outside [0, n), a side below 13 or above
// 32768, bytes outside the bank, or — for the scratch — more pixels than plane_stride.  The geometry and box kernels
// also refuse a sample whose image does not fit F x F after the halving.  A refused sample is all NaN; no address is
// formed from a refused value.
#define DC_CHUNKS_MAX 64
#define DC_TH 32
#define DC_TW 64
#define DC_R 12
#define DC_AW (DC_TW + 2 * DC_R)
#define DC_AH (DC_TH + 2 * DC_R)
#define DG_THREADS 256
#define DB_THREADS 64

struct DetSample {
    bool ok;
    int H0, W0;
    long long off;
};
DEVI DetSample det_sample(const long long* __restrict__ offsets, const int* __restrict__ sizes, long long n,
                          long long total, const long long* __restrict__ index, int b, long long plane_limit) {
    DetSample s = {false, 0, 0, 0};
    const long long idx = index[b];
    if (idx < 0 || idx >= n) return s;
    const int H0 = sizes[2 * idx], W0 = sizes[2 * idx + 1];
    if (H0 < 13 || W0 < 13 || H0 > 32768 || W0 > 32768) return s;
    const long long P = (long long)H0 * W0, off = offsets[idx];
    if (off < 0 || off > total || 3 * P > total - off || P > plane_limit) return s;
    s.ok = true, s.H0 = H0, s.W0 = W0, s.off = off;
    return s;
}
// H0 x W0 through the rotation and the halving: the size of the image inside the F x F output
struct DetGeom {
    bool rot, hf, vf, halve, fits;
    int H1, W1, H2, W2, p1, p2;
};
DEVI DetGeom det_geom(int H0, int W0, int bits, int F) {
    DetGeom g;
    g.hf = bits & 1, g.vf = bits & 2, g.rot = bits & 4;
    g.H1 = g.rot ? W0 : H0, g.W1 = g.rot ? H0 : W0;
    g.halve = g.H1 > F || g.W1 > F;
    g.H2 = g.halve ? (g.H1 + 1) >> 1 : g.H1, g.W2 = g.halve ? (g.W1 + 1) >> 1 : g.W1;
    g.fits = g.H2 <= F && g.W2 <= F;
    g.p1 = (F - g.W2) >> 1, g.p2 = (F - g.H2) >> 1;  // floor((F - W2) / 2): never negative where it fits
    return g;
}
static __host__ __device__ inline int det_chunks(long long P) {  // of the statistics pass; the image's size alone decides
    const long long c = P / 4096;
    return (int)(c < 1 ? 1 : c > DC_CHUNKS_MAX ? DC_CHUNKS_MAX : c);
}
DEVI CaSample det_ca_sample(const float* __restrict__ factors, const unsigned char* __restrict__ order,
                            const float* __restrict__ sigma, int b) {
    CaSample s;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int id = order[4 * b + i];
        s.op[i] = id <= 3 ? id : CA_SKIP;
        s.f[i] = id <= 3 ? factors[4 * b + id] : 1.f;
    }
    s.flags = 0;
    s.sigma = sigma[b];
    return s;
}
// ToTensor: float(v) / 255, correctly rounded (v * (1 / 255) is another fp32 number for 126 of the 256 levels)
DEVI float det_u8(unsigned char v) { return (float)v / 255.f; }

__global__ __launch_bounds__(CA_STAT_THREADS) void det_color_stats_kernel(
    const unsigned char* __restrict__ pixels, long long total, const long long* __restrict__ offsets,
    const int* __restrict__ sizes, long long n, const long long* __restrict__ index,
    const float* __restrict__ factors, const unsigned char* __restrict__ order, const float* __restrict__ sigma,
    float* __restrict__ partial, long long plane_limit) {
    __shared__ float wsum[CA_STAT_THREADS / 64];
    const int b = blockIdx.x / DC_CHUNKS_MAX, c = blockIdx.x - b * DC_CHUNKS_MAX, t = threadIdx.x;
    const CaSample s = det_ca_sample(factors, order, sigma, b);
    const int nj = ca_contrast_slot(s);
    if (nj == 4) return;  // (uniform) nobody reads this sample's partials
    const DetSample d = det_sample(offsets, sizes, n, total, index, b, plane_limit);
    if (!d.ok) return;  // (uniform)
    const int P = d.H0 * d.W0, chunks = det_chunks(P);
    if (c >= chunks) return;  // (uniform) a surplus block
    const int per = (P + chunks - 1) / chunks, g0 = c * per, g1 = min(P, g0 + per);
    const unsigned char* src = pixels + d.off;
    float sum = 0.f;
    for (int g = g0 + t; g < g1; g += CA_STAT_THREADS) {
        float pr = det_u8(src[3 * (size_t)g]), pg = det_u8(src[3 * (size_t)g + 1]), pb = det_u8(src[3 * (size_t)g + 2]);
        ca_jitter(s, nj, 0.f, pr, pg, pb);
        sum += ca_gray(pr, pg, pb);
    }
    sum = wave_sum(sum);
    if ((t & 63) == 0) wsum[t >> 6] = sum;
    __syncthreads();
    if (t == 0) {
        float tot = 0.f;
        for (int w = 0; w < CA_STAT_THREADS / 64; ++w) tot += wsum[w];
        partial[(size_t)b * DC_CHUNKS_MAX + c] = tot;
    }
}

// One workgroup walks the tiles `blockIdx.x % tiles_grid`, `+ tiles_grid`, ... of its sample: the host sizes the grid
// for the batch's largest image (it knows the indices and the sizes), a smaller image's surplus workgroups exit, and a
// sample larger than the host said is still covered.
__global__ __launch_bounds__(CA_THREADS) void det_color_apply_kernel(
    const unsigned char* __restrict__ pixels, long long total, const long long* __restrict__ offsets,
    const int* __restrict__ sizes, long long n, const long long* __restrict__ index,
    const float* __restrict__ factors, const unsigned char* __restrict__ order, const float* __restrict__ sigma,
    const float* __restrict__ partial, float* __restrict__ scratch, long long plane_stride, int tiles_grid) {
    extern __shared__ __attribute__((aligned(16))) float ca_lds[];
    __shared__ float wl[DC_R + 1];
    const int t = threadIdx.x;
    const int b = blockIdx.x / tiles_grid, tile0 = blockIdx.x - b * tiles_grid;
    const DetSample d = det_sample(offsets, sizes, n, total, index, b, plane_stride);
    if (!d.ok) return;  // (uniform) the geometry launch makes the same test and never reads this sample's scratch
    const int H0 = d.H0, W0 = d.W0;
    const int tiles_x = (W0 + DC_TW - 1) / DC_TW, tiles = tiles_x * ((H0 + DC_TH - 1) / DC_TH);
    if (tile0 >= tiles) return;  // (uniform)
    const unsigned char* src = pixels + d.off;
    float* dst = scratch + (size_t)b * 3 * (size_t)plane_stride;

    const CaSample s = det_ca_sample(factors, order, sigma, b);
    float m = 0.f;
    if (ca_contrast_slot(s) < 4) {  // (uniform) the partials in chunk order
        const int chunks = det_chunks((long long)H0 * W0);
        for (int c = 0; c < chunks; ++c) m += partial[(size_t)b * DC_CHUNKS_MAX + c];
        m /= (float)(H0 * W0);
    }
    const bool blur = s.sigma > 0.0625f;  // (uniform) below it every weight but the centre's is 0 in fp32
    int R = 0;
    if (blur) {
        const double r6 = ceil(6.0 * (double)s.sigma);
        R = r6 < (double)DC_R ? (int)r6 : DC_R;
        R = (R + 1) & ~1;  // as the square stage: even radii, a tap of weight ~0 more
        if (t <= DC_R) {
            const double inv2 = 0.5 / ((double)s.sigma * (double)s.sigma);
            double sum = 1.0;
            for (int k = 1; k <= DC_R; ++k) sum += 2.0 * exp(-(double)(k * k) * inv2);
            wl[t] = t <= R ? (float)(exp(-(double)(t * t) * inv2) / sum) : 0.f;
        }
    }
    float* A = ca_lds;                         // [3][DC_AH][DC_AW] jittered tile + halo
    float* T = A + (size_t)3 * DC_AH * DC_AW;  // [3][DC_AH][DC_TW] after the horizontal pass
    for (int tile = tile0; tile < tiles; tile += tiles_grid) {
        const int ty = tile / tiles_x, y0 = ty * DC_TH, x0 = (tile - ty * tiles_x) * DC_TW;
        const int nro = min(DC_TH, H0 - y0), nco = min(DC_TW, W0 - x0);
        if (!blur) {
            for (int i = t; i < nro * nco; i += CA_THREADS) {
                const int orow = i / nco, oc = i - orow * nco;
                const size_t o = (size_t)(y0 + orow) * W0 + x0 + oc;
                float pr = det_u8(src[3 * o]), pg = det_u8(src[3 * o + 1]), pb = det_u8(src[3 * o + 2]);
                ca_jitter(s, 4, m, pr, pg, pb);
                dst[o] = pr, dst[(size_t)plane_stride + o] = pg, dst[2 * (size_t)plane_stride + o] = pb;
            }
            continue;
        }
        __syncthreads();  // the previous tile's passes have read A and T; wl is written
        const int nra = nro + 2 * R, nca = nco + 2 * R;
        for (int i = t; i < nra * nca; i += CA_THREADS) {
            const int ar = i / nca, ac = i - ar * nca;
            // overshoot at most 12 < 13 <= H0, W0: one reflection lands inside
            const int y = ca_reflect(y0 - R + ar, H0), x = ca_reflect(x0 - R + ac, W0);
            const size_t o = (size_t)y * W0 + x;
            float pr = det_u8(src[3 * o]), pg = det_u8(src[3 * o + 1]), pb = det_u8(src[3 * o + 2]);
            ca_jitter(s, 4, m, pr, pg, pb);
            float* a = A + (size_t)ar * DC_AW + ac;
            a[0] = pr, a[(size_t)DC_AH * DC_AW] = pg, a[(size_t)2 * DC_AH * DC_AW] = pb;
        }
        __syncthreads();
        for (int i = t; i < 3 * nra * nco; i += CA_THREADS) {
            const int oc = i % nco, q = i / nco, ar = q % nra, ch = q / nra;
            const float* row = A + ((size_t)ch * DC_AH + ar) * DC_AW + oc + R;
            float acc = 0.f;
            for (int k = -R; k <= R; ++k) acc += wl[k < 0 ? -k : k] * row[k];
            T[((size_t)ch * DC_AH + ar) * DC_TW + oc] = acc;
        }
        __syncthreads();
        for (int i = t; i < 3 * nro * nco; i += CA_THREADS) {
            const int oc = i % nco, q = i / nco, orow = q % nro, ch = q / nro;
            const float* col = T + ((size_t)ch * DC_AH + orow + R) * DC_TW + oc;
            float acc = 0.f;
            for (int k = -R; k <= R; ++k) acc += wl[k < 0 ? -k : k] * col[k * DC_TW];
            dst[(size_t)ch * (size_t)plane_stride + (size_t)(y0 + orow) * W0 + x0 + oc] = acc;
        }
    }
}

// 128 w((t - 3.5) / 2), t = 0 .. 7, of Keys' cubic with a = -0.5
DEVI int dg_w8(int t) {
    const int a = t < 4 ? t : 7 - t;
    return a == 0 ? -3 : a == 1 ? -9 : a == 2 ? 29 : 111;
}
// One lane = 4 neighbouring output pixels of a row, all three channels.  The dihedral map is separable: the source
// offset of pixel (i, j) of the turned image is rowterm(i) + colterm(j) (no rotation: i' W0 + j'; rotation:
// (W0 - 1 - i') + j' W0, with i' = H1 - 1 - i under the vertical flip and j' = W1 - 1 - j under the horizontal one).
// Halving: output (ty, tx) = sum over the rows 2 ty - 3 .. 2 ty + 4 of wy * (sum over the columns 2 tx - 3 .. 2 tx + 4
// of wx * pixel), taps outside the zero-padded even-sized image dropped and the weights (-3, -9, 29, 111, 111, 29, -9,
// -3) divided by the sum of those kept (256 in the interior) — F.interpolate(bicubic, antialias=True) at scale 2,
// horizontal pass first.  The lane reads its 8 x 14 source window per channel through the cache, a row at a time.
template <bool U8>
__global__ __launch_bounds__(DG_THREADS) void det_geometry_kernel(
    const float* __restrict__ scratch, long long plane_stride, const unsigned char* __restrict__ pixels,
    long long total, const long long* __restrict__ offsets, const int* __restrict__ sizes, long long n,
    const long long* __restrict__ index, const unsigned char* __restrict__ geom, float* __restrict__ out, int F,
    int blocks_per_sample, f32x4 mean, f32x4 stdv) {
    const int b = blockIdx.x / blocks_per_sample;
    const int g = (blockIdx.x - b * blocks_per_sample) * DG_THREADS + threadIdx.x;
    const int F4 = F >> 2;
    if (g >= F * F4) return;
    const int y = g / F4, x0 = 4 * (g - y * F4);
    const size_t plane = (size_t)F * F;
    float* dst = out + (size_t)b * 3 * plane + (size_t)y * F + x0;

    const DetSample d = det_sample(offsets, sizes, n, total, index, b, U8 ? 0x7fffffffffffffffLL : plane_stride);
    const DetGeom gm = det_geom(d.H0, d.W0, geom ? geom[b] : 0, F);
    if (!(d.ok && gm.fits)) {  // (uniform)
        const f32x4 bad = {NAN, NAN, NAN, NAN};
        st4(dst, bad), st4(dst + plane, bad), st4(dst + 2 * plane, bad);
        return;
    }
    const int W0 = d.W0, ty = y - gm.p2, tx0 = x0 - gm.p1;
    const unsigned char* src8 = pixels + d.off;
    const float* src32 = scratch + (size_t)b * 3 * (size_t)plane_stride;
    auto rowterm = [&](int i) { const int ii = gm.vf ? gm.H1 - 1 - i : i; return gm.rot ? W0 - 1 - ii : ii * W0; };
    auto colterm = [&](int j) { const int jj = gm.hf ? gm.W1 - 1 - j : j; return gm.rot ? jj * W0 : jj; };
    auto fetch = [&](int o, int ch) {
        return U8 ? det_u8(src8[3 * (size_t)o + ch]) : src32[(size_t)ch * (size_t)plane_stride + (size_t)o];
    };
    f32x4 v[3];
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    v[0] = v[1] = v[2] = zero;
    const bool touches = ty >= 0 && ty < gm.H2 && tx0 + 3 >= 0 && tx0 < gm.W2;
    if (touches && !gm.halve) {
        const int ro = rowterm(ty);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int tx = tx0 + k;
            if (tx >= 0 && tx < gm.W2) {
                const int o = ro + colterm(tx);
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) v[ch][k] = fetch(o, ch);
            }
        }
    } else if (touches) {
        const int Hp = gm.H1 + (gm.H1 & 1), Wp = gm.W1 + (gm.W1 & 1);
        int sumy = 0;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int iy = 2 * ty - 3 + t;
            sumy += iy >= 0 && iy < Hp ? dg_w8(t) : 0;
        }
        float wx[4][8];
        int co[14];  // of the columns 2 tx0 - 3 .. 2 tx0 + 10; -1: a tap outside the image or on the zero column
#pragma unroll
        for (int u = 0; u < 14; ++u) {
            const int ix = 2 * tx0 - 3 + u;
            co[u] = ix >= 0 && ix < gm.W1 ? colterm(ix) : -1;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int tx = tx0 + k;
            const bool in = tx >= 0 && tx < gm.W2;
            int sum = 0;
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const int ix = 2 * tx - 3 + t;
                sum += ix >= 0 && ix < Wp ? dg_w8(t) : 0;
            }
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const int ix = 2 * tx - 3 + t;
                wx[k][t] = in && ix >= 0 && ix < Wp ? (float)dg_w8(t) / (float)sum : 0.f;
            }
        }
        // rolled on purpose: unrolled, the 3 x 8 x 14 loads in flight need more registers than a lane has
#pragma unroll 1
        for (int t = 0; t < 8; ++t) {
            const int iy = 2 * ty - 3 + t;
            if (iy < 0 || iy >= gm.H1) continue;  // outside, or the zero row: contributes 0
            const float wy = (float)dg_w8(t) / (float)sumy;
            const int ro = rowterm(iy);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                float px[14];
#pragma unroll
                for (int u = 0; u < 14; ++u) px[u] = co[u] >= 0 ? fetch(ro + co[u], ch) : 0.f;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float hs = 0.f;
#pragma unroll
                    for (int q = 0; q < 8; ++q) hs += wx[k][q] * px[2 * k + q];
                    v[ch][k] += wy * hs;
                }
            }
        }
    }
    // outside the image v is 0: the padding is the normalised value of black
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float mu = ch == 0 ? mean[0] : ch == 1 ? mean[1] : mean[2];
        const float sd = ch == 0 ? stdv[0] : ch == 1 ? stdv[1] : stdv[2];
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = (v[ch][k] - mu) / sd;
        st4(dst + ch * plane, o);
    }
}

// One lane = one box of the batch.  out_start [B + 1] says where sample b's boxes go; a sample whose count there is
// not its bank count is refused like a bad index.  Dataset.__getitem__'s statements, one fp32 operation each.
__global__ __launch_bounds__(DB_THREADS) void det_boxes_kernel(
    const float* __restrict__ boxes, const long long* __restrict__ labels, const long long* __restrict__ box_offsets,
    long long m, const int* __restrict__ sizes, long long n, const long long* __restrict__ index,
    const unsigned char* __restrict__ geom, const long long* __restrict__ out_start, float* __restrict__ out_boxes,
    long long* __restrict__ out_labels, long long m_out, int F, int blocks_per_sample) {
    const int b = blockIdx.x / blocks_per_sample;
    const long long k = (long long)(blockIdx.x - b * blocks_per_sample) * DB_THREADS + threadIdx.x;
    const long long lo = out_start[b], hi = out_start[b + 1];
    if (lo < 0 || hi < lo || hi > m_out) return;  // (uniform) nowhere to write
    if (k >= hi - lo) return;
    const long long idx = index[b];
    bool ok = idx >= 0 && idx < n;
    long long s0 = 0;
    int H0 = 0, W0 = 0;
    if (ok) {
        s0 = box_offsets[idx];
        const long long s1 = box_offsets[idx + 1];
        H0 = sizes[2 * idx], W0 = sizes[2 * idx + 1];
        ok = s0 >= 0 && s1 >= s0 && s1 <= m && s1 - s0 == hi - lo && H0 >= 13 && W0 >= 13 && H0 <= 32768 && W0 <= 32768;
    }
    const DetGeom gm = det_geom(H0, W0, geom ? geom[b] : 0, F);
    f32x4 o = {NAN, NAN, NAN, NAN};
    long long label = -1;
    if (ok && gm.fits) {
        const f32x4 q = ld4(boxes + 4 * (size_t)(s0 + k));
        float x1 = q[0], y1 = q[1], x2 = q[2], y2 = q[3];
        if (gm.rot) {  // dataset.py:53-61
            const float w = (float)W0, nx1 = y1, nx2 = y2, ny1 = w - x2, ny2 = w - x1;
            x1 = nx1, x2 = nx2, y1 = ny1, y2 = ny2;
        }
        if (gm.hf) {  // :67-71
            const float w = (float)gm.W1, nx1 = w - x2, nx2 = w - x1;
            x1 = nx1, x2 = nx2;
        }
        if (gm.vf) {  // :76-80
            const float h = (float)gm.H1, ny1 = h - y2, ny2 = h - y1;
            y1 = ny1, y2 = ny2;
        }
        if (gm.halve) x1 /= 2.f, y1 /= 2.f, x2 /= 2.f, y2 /= 2.f;  // :97
        const float p1 = (float)gm.p1, p2 = (float)gm.p2;          // :103-106
        o[0] = x1 + p1, o[1] = y1 + p2, o[2] = x2 + p1, o[3] = y2 + p2;
        label = labels[s0 + k];
    }
    st4(out_boxes + 4 * (size_t)(lo + k), o);
    out_labels[lo + k] = label;
}

static bool det_bank_ok(const void* pixels, long long total, const void* offsets, const void* sizes, long long n,
                        const void* index, int B) {
    return pixels && offsets && sizes && index && total >= 1 && n >= 1 && B >= 0 && B <= 65535;
}

extern "C" size_t ssl4gie_det_color_workspace_bytes(int B) {
    return B < 1 ? 0 : sizeof(float) * (size_t)B * DC_CHUNKS_MAX;
}

extern "C" int ssl4gie_det_color(const unsigned char* pixels, long long total, const long long* offsets,
                                 const int* sizes, long long n, const long long* index, int B, int max_h, int max_w,
                                 const float* factors, const unsigned char* order, const float* sigma, float* scratch,
                                 long long plane_stride, void* workspace, size_t workspace_bytes, void* stream) {
    REQUIRE(det_bank_ok(pixels, total, offsets, sizes, n, index, B));
    REQUIRE(factors && order && sigma && scratch && workspace);
    REQUIRE(max_h >= 13 && max_w >= 13 && max_h <= 32768 && max_w <= 32768 && plane_stride >= 169);
    REQUIRE(((uintptr_t)scratch | (uintptr_t)workspace) % 16 == 0);
    REQUIRE(workspace_bytes >= ssl4gie_det_color_workspace_bytes(B));
    if (B == 0) return 0;
    const int tiles = ((max_w + DC_TW - 1) / DC_TW) * ((max_h + DC_TH - 1) / DC_TH);
    REQUIRE((long long)B * tiles <= 0x7fffffffLL);
    const size_t lds = sizeof(float) * 3 * DC_AH * (DC_AW + DC_TW);
    static bool attr = false;
    if (!attr) {
        HIP_RET(hipFuncSetAttribute((const void*)det_color_apply_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds));
        attr = true;
    }
    hipLaunchKernelGGL(det_color_stats_kernel, dim3((unsigned)(B * DC_CHUNKS_MAX)), dim3(CA_STAT_THREADS), 0,
                       (hipStream_t)stream, pixels, total, offsets, sizes, n, index, factors, order, sigma,
                       (float*)workspace, plane_stride);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(det_color_apply_kernel, dim3((unsigned)(B * tiles)), dim3(CA_THREADS), lds,
                       (hipStream_t)stream, pixels, total, offsets, sizes, n, index, factors, order, sigma,
                       (const float*)workspace, scratch, plane_stride, tiles);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int ssl4gie_det_geometry(const float* scratch, long long plane_stride, const unsigned char* pixels,
                                    long long total, const long long* offsets, const int* sizes, long long n,
                                    const long long* index, const unsigned char* geom, float* out, int B, int F,
                                    const float* mean, const float* std, void* stream) {
    REQUIRE(det_bank_ok(pixels, total, offsets, sizes, n, index, B));
    REQUIRE(out && mean && std);
    REQUIRE(F >= 4 && F % 4 == 0 && F <= 16384);
    for (int c = 0; c < 3; ++c) REQUIRE(std[c] != 0.f);
    REQUIRE(((uintptr_t)out | (uintptr_t)scratch) % 16 == 0);
    if (scratch) REQUIRE(plane_stride >= 169);
    const int per = F * (F / 4), blocks = (per + DG_THREADS - 1) / DG_THREADS;
    REQUIRE((long long)B * blocks <= 0x7fffffffLL);
    if (B == 0) return 0;
    const f32x4 mu = {mean[0], mean[1], mean[2], 0.f}, sd = {std[0], std[1], std[2], 1.f};
    if (scratch)
        hipLaunchKernelGGL(det_geometry_kernel<false>, dim3((unsigned)(B * blocks)), dim3(DG_THREADS), 0,
                           (hipStream_t)stream, scratch, plane_stride, pixels, total, offsets, sizes, n, index, geom, out,
                           F, blocks, mu, sd);
    else
        hipLaunchKernelGGL(det_geometry_kernel<true>, dim3((unsigned)(B * blocks)), dim3(DG_THREADS), 0,
                           (hipStream_t)stream, scratch, 0LL, pixels, total, offsets, sizes, n, index, geom, out, F,
                           blocks, mu, sd);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int ssl4gie_det_boxes(const float* boxes, const long long* labels, const long long* box_offsets,
                                 long long m, const int* sizes, long long n, const long long* index,
                                 const unsigned char* geom, const long long* out_start, float* out_boxes,
                                 long long* out_labels, long long m_out, int B, int F, int max_boxes, void* stream) {
    REQUIRE(box_offsets && sizes && index && out_start && n >= 1 && m >= 0 && m_out >= 0 && B >= 0 && B <= 65535);
    REQUIRE(F >= 4 && F % 4 == 0 && F <= 16384 && max_boxes >= 0);
    if (m > 0) REQUIRE(boxes && labels);
    if (m_out > 0) REQUIRE(out_boxes && out_labels);
    REQUIRE(((uintptr_t)boxes | (uintptr_t)out_boxes) % 16 == 0);
    if (B == 0 || m_out == 0 || max_boxes == 0) return 0;
    const int blocks = (max_boxes + DB_THREADS - 1) / DB_THREADS;
    REQUIRE((long long)B * blocks <= 0x7fffffffLL);
    hipLaunchKernelGGL(det_boxes_kernel, dim3((unsigned)(B * blocks)), dim3(DB_THREADS), 0, (hipStream_t)stream, boxes,
                       labels, box_offsets, m, sizes, n, index, geom, out_start, out_boxes, out_labels, m_out, F, blocks);
    LAUNCH_CHECK();
    return 0;
}
