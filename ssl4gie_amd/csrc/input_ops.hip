// On-device input pipeline: random-resized-crop views out of a uint8 image bank resident in HBM.
//
// ssl4gie_view_sample_u8 is transforms.RandomResizedCrop(S, interpolation=BICUBIC | BILINEAR) +
// RandomHorizontalFlip + ToTensor + Normalize (Models/mae/main_pretrain.py:123-127; the geometric part of
// Models/moco_v3/main_moco.py:263,275) with the crop boxes and flips already drawn: bank [n, Hs, Ws, 3] u8,
// one image index + box + flip per sample -> fp32 NCHW [B, 3, S, S].
//
// Resampling rule (PIL's ImagingResample; F.interpolate(antialias=True, align_corners=False) computes the same):
// separable, the crop happens FIRST (taps never leave the box).  Per axis, box length L -> S outputs:
//   scale = L / S, fs = max(scale, 1), support = R fs (R = 2 bicubic, 1 bilinear);
//   output o: c = (o + 0.5) scale, taps k in [max(0, int(c - support + 0.5)), min(L, int(c + support + 0.5))),
//   weight f((k - c + 0.5) / fs) / (sum over the taps).
// Then flip, clamp to [0, 255] (bicubic overshoots; PIL saturates), (v / 255 - mean) / std.  No rounding to
// integer levels between the passes.
//
// One workgroup = one sample x one band of output rows:
//   1. the weights of all S output columns and of the band's rows, evaluated in fp64 (a few thousand cubic
//      evaluations; in fp32 the centre c would carry 1e-5 of a pixel at L = 96 already) and kept as fp32 in LDS;
//   2. horizontal pass over the source rows the band needs: u8 pixels -> fp32 LDS tile [rows][3][S];
//   3. vertical pass out of LDS, 4 output columns per lane, one 16-byte store each.
// fp32 accumulation in a fixed order, no atomics: bit-identical from run to run.
#include "common.h"
#include "ssl4gie_hip.h"

#define VS_THREADS 512  // 8 waves share one LDS plan: bicubic 155 us against 185 with 256 threads, 177 with 1024 (B = 256)
#define VS_LDS_SMALL (48 * 1024)   // several workgroups per CU: the plan of every stored size up to ~400 px
#define VS_LDS_MAX (160 * 1024)    // all of a CU's LDS: what Hs = 1024 -> S = 224 needs

struct ViewPlan {
    int band;  // output rows per workgroup
    int rows;  // capacity of the LDS tile in source rows
    int tx, ty;  // capacity of the per-output tap lists, horizontal / vertical
    size_t bytes;
};

// taps of one output are int(c + s + .5) - int(c - s + .5) <= floor(2 s) + 1; one more for the margin
static int tap_cap(int L, int S, int R) {
    const double sc = (double)L / S;
    return (int)(2.0 * R * (sc > 1.0 ? sc : 1.0)) + 2;
}
// Source rows under a band of nb outputs: from int(c0 - s + .5) to int(c0 + (nb - 1) scale + s + .5), at most
// (nb - 1) scale + 2 s + 1 of them; increasing in scale, so the whole image (scale = Hs / S) is the worst box.
static void view_plan(int Hs, int Ws, int S, int R, int band, ViewPlan* p) {
    const double sy = (double)Hs / S, fsy = sy > 1.0 ? sy : 1.0;
    long long rows = (long long)((band - 1) * sy + 2.0 * R * fsy + 2.0) + 1;
    if (rows > Hs) rows = Hs;
    p->band = band;
    p->rows = (int)rows;
    p->tx = tap_cap(Ws, S, R);
    p->ty = tap_cap(Hs, S, R);
    p->bytes = sizeof(float) * ((size_t)rows * 3 * S + (size_t)p->tx * S + 2 * (size_t)S + (size_t)band * p->ty
                                + 2 * (size_t)band);
}
static bool view_plan_pick(int Hs, int Ws, int S, int R, ViewPlan* p) {
    for (int band = 32; band >= 1; band >>= 1) {  // the tallest band that leaves room for several workgroups
        view_plan(Hs, Ws, S, R, band, p);
        if (p->bytes <= VS_LDS_SMALL) return true;
    }
    for (int band = 8; band >= 1; band >>= 1) {
        view_plan(Hs, Ws, S, R, band, p);
        if (p->bytes <= VS_LDS_MAX) return true;
    }
    return false;
}

DEVI double vs_filter(double x, int filter) {
    x = fabs(x);
    if (filter == SSL4GIE_FILTER_BICUBIC) {
        const double a = -0.5;  // Keys
        if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
        if (x < 2.0) return a * (((x - 5.0) * x + 8.0) * x - 4.0);
        return 0.0;
    }
    return x < 1.0 ? 1.0 - x : 0.0;
}
// tap range [lo, hi) of output o on an axis of box length L
DEVI void vs_range(int o, double scale, double support, int L, int& lo, int& hi) {
    const double c = (o + 0.5) * scale;
    lo = max(0, (int)(c - support + 0.5));
    hi = min(L, (int)(c + support + 0.5));
}
// normalised fp32 weights of output o into w[k * stride], k < n = min(hi - lo, cap); returns lo, n
DEVI void vs_weights(int o, double scale, double fs, double support, int L, int filter, int cap, float* w,
                     int stride, int& lo, int& n) {
    int hi;
    vs_range(o, scale, support, L, lo, hi);
    n = min(hi - lo, cap);
    const double c = (o + 0.5) * scale, inv_fs = 1.0 / fs;
    double sum = 0.0;
    for (int k = 0; k < n; ++k) sum += vs_filter((lo + k - c + 0.5) * inv_fs, filter);
    const double inv = 1.0 / sum;
    for (int k = 0; k < n; ++k) w[k * stride] = (float)(vs_filter((lo + k - c + 0.5) * inv_fs, filter) * inv);
}

__global__ __launch_bounds__(VS_THREADS) void view_sample_kernel(
    const unsigned char* __restrict__ bank, long long n, int Hs, int Ws, const long long* __restrict__ index,
    const int* __restrict__ box, const unsigned char* __restrict__ flip, float* __restrict__ out, int S,
    int filter, int band, int rows_cap, int TX, int TY, int nbands, f32x4 nscale, f32x4 nshift) {
    extern __shared__ __attribute__((aligned(16))) float vs_lds[];
    float* tile = vs_lds;                            // [rows_cap][3][S]
    float* wx = tile + (size_t)rows_cap * 3 * S;     // [TX][S]: tap k of column x at wx[k S + x]
    int* xlo = (int*)(wx + (size_t)TX * S);          // [S]
    int* xn = xlo + S;                               // [S]
    float* wy = (float*)(xn + S);                    // [band][TY]
    int* ylo = (int*)(wy + band * TY);               // [band]
    int* yn = ylo + band;                            // [band]

    const int t = threadIdx.x;
    const int b = blockIdx.x / nbands, o0 = (blockIdx.x - b * nbands) * band;
    const int nb = min(band, S - o0);
    const int S4 = S >> 2;
    float* dst = out + (size_t)b * 3 * S * S;

    const long long img = index[b];
    const int top = box[4 * b], left = box[4 * b + 1], h = box[4 * b + 2], w = box[4 * b + 3];
    const bool ok = img >= 0 && img < n && h >= 1 && w >= 1 && top >= 0 && left >= 0 &&
                    (long long)top + h <= Hs && (long long)left + w <= Ws;
    if (!ok) {  // (uniform) the sample is all NaN and no address is formed from its index or box
        const f32x4 nan4 = {NAN, NAN, NAN, NAN};
        for (int i = t; i < nb * 3 * S4; i += VS_THREADS) {
            const int xq = i % S4, q = i / S4, ch = q % 3, orow = q / 3;
            st4(dst + ((size_t)ch * S + o0 + orow) * S + 4 * xq, nan4);
        }
        return;
    }

    const double R = filter == SSL4GIE_FILTER_BICUBIC ? 2.0 : 1.0;
    const double sclx = (double)w / S, fsx = sclx > 1.0 ? sclx : 1.0;
    const double scly = (double)h / S, fsy = scly > 1.0 ? scly : 1.0;
    for (int x = t; x < S; x += VS_THREADS) {
        int lo, cnt;
        vs_weights(x, sclx, fsx, R * fsx, w, filter, TX, wx + x, S, lo, cnt);
        xlo[x] = lo;
        xn[x] = cnt;
    }
    for (int j = t; j < nb; j += VS_THREADS) {
        int lo, cnt;
        vs_weights(o0 + j, scly, fsy, R * fsy, h, filter, TY, wy + j * TY, 1, lo, cnt);
        ylo[j] = lo;
        yn[j] = cnt;
    }
    __syncthreads();
    // the band's source rows, from the tap lists themselves (lo and hi do not decrease with o)
    const int r_lo = ylo[0];
    const int nrows = min(ylo[nb - 1] + yn[nb - 1] - r_lo, rows_cap);

    // horizontal pass: source rows r_lo .. r_lo + nrows of the box.  Rows are 3 Ws bytes with no alignment to
    // speak of (Ws = 81: 243), so pixels are read byte by byte; neighbouring lanes read neighbouring pixels.
    const unsigned char* src = bank + (((size_t)img * Hs + top + r_lo) * Ws + left) * 3;
    for (int i = t; i < nrows * S; i += VS_THREADS) {
        const int r = i / S, x = i - r * S;
        const unsigned char* p = src + ((size_t)r * Ws + xlo[x]) * 3;
        const int cnt = xn[x];
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        for (int k = 0; k < cnt; ++k, p += 3) {
            const float wv = wx[k * S + x];
            a0 += wv * (float)p[0];
            a1 += wv * (float)p[1];
            a2 += wv * (float)p[2];
        }
        float* d = tile + (size_t)r * 3 * S + x;
        d[0] = a0;
        d[S] = a1;
        d[2 * S] = a2;
    }
    __syncthreads();

    // vertical pass + flip + clamp + normalise: 4 output columns per lane
    const bool fl = flip != nullptr && flip[b] != 0;
    for (int i = t; i < nb * 3 * S4; i += VS_THREADS) {
        const int xq = i % S4, q = i / S4, ch = q % 3, orow = q / 3;
        const int cnt = yn[orow], r0 = ylo[orow] - r_lo;
        const float* wv = wy + orow * TY;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < cnt; ++k) {
            const int r = min(r0 + k, rows_cap - 1);  // (never binds: see view_plan)
            acc += wv[k] * ld4(tile + ((size_t)r * 3 + ch) * S + 4 * xq);
        }
        const float sc = ch == 0 ? nscale[0] : ch == 1 ? nscale[1] : nscale[2];
        const float sh = ch == 0 ? nshift[0] : ch == 1 ? nshift[1] : nshift[2];
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = fminf(fmaxf(acc[j], 0.f), 255.f) * sc + sh;
        float* o = dst + ((size_t)ch * S + o0 + orow) * S;
        if (fl) {
            const f32x4 rv = {v[3], v[2], v[1], v[0]};
            st4(o + (S - 4 - 4 * xq), rv);
        } else {
            st4(o + 4 * xq, v);
        }
    }
}

extern "C" int ssl4gie_view_sample_u8(const unsigned char* bank, long long n, int Hs, int Ws,
                                      const long long* index, const int* box, const unsigned char* flip,
                                      float* out, int B, int S, int filter, const float* mean, const float* std,
                                      void* stream) {
    REQUIRE(bank && index && box && out && mean && std);
    REQUIRE(n >= 1 && Hs >= 1 && Ws >= 1 && B >= 0 && S >= 4 && S % 4 == 0);
    REQUIRE(filter == SSL4GIE_FILTER_BILINEAR || filter == SSL4GIE_FILTER_BICUBIC);
    for (int c = 0; c < 3; ++c) REQUIRE(std[c] > 0.f);
    ViewPlan p;
    REQUIRE(view_plan_pick(Hs, Ws, S, filter == SSL4GIE_FILTER_BICUBIC ? 2 : 1, &p));
    const int nbands = (S + p.band - 1) / p.band;
    REQUIRE((long long)B * nbands <= 0x7fffffffLL);
    if (B == 0) return 0;
    static bool attr = false;
    if (!attr) {
        HIP_RET(hipFuncSetAttribute((const void*)view_sample_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    VS_LDS_MAX));
        attr = true;
    }
    const f32x4 nscale = {1.f / (255.f * std[0]), 1.f / (255.f * std[1]), 1.f / (255.f * std[2]), 0.f};
    const f32x4 nshift = {-mean[0] / std[0], -mean[1] / std[1], -mean[2] / std[2], 0.f};
    hipLaunchKernelGGL(view_sample_kernel, dim3((unsigned)(B * nbands)), dim3(VS_THREADS), p.bytes,
                       (hipStream_t)stream, bank, n, Hs, Ws, index, box, flip, out, S, filter, p.band, p.rows,
                       p.tx, p.ty, nbands, nscale, nshift);
    LAUNCH_CHECK();
    return 0;
}
