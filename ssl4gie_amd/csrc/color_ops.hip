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
