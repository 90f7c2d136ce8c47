// Atrous (dilated) convolution glue of DeepLabV3+ for gfx950: what segmentation_models_pytorch
// 0.3.2 runs around its 1x1 convolutions — the dilated dense 3x3 of a ResNet layer4 at output stride 16
// (encoders/_utils.py replace_strides_with_dilation), the depthwise 3x3 of SeparableConv2d (deeplabv3/decoder.py:
// ASPPSeparableConv, aspp.1, block2), nn.UpsamplingBilinear2d(scale_factor=4) (decoder.up, SegmentationHead) and
// torch.cat along channels (ASPP.forward, DeepLabV3PlusDecoder.forward).
//
// Channels-last maps [B, H, W, C] in the operand type, fp32 accumulation, no float atomics: every reduction is
// per-thread partials + a fixed-order second pass, so results are bit-identical from run to run.  A tap outside the
// map is decided on its (row, column) integers BEFORE an address is formed from them.  All kernels are HBM-bound byte
// movers: 16-byte accesses along channels, the neighbour taps come from L2 / the vector cache.
#include "common.h"
#include "ssl4gie_hip.h"
#include "internal.h"
#include "map_chunk.h"

namespace {

// ------------------------------------------------------------------ dilated 3x3 patch matrix (stride 1, pad = d)
// cols[(b, y, x), (ky*3 + kx)*C + c] = x[b, y + (ky-1) d, x + (kx-1) d, c] (0 outside); columns [9C, ld) are zeros:
// the layout of im2col3x3 (dpt_ops.hip), so the weight images of conv3x3_weight_pack and the plain GEMMs apply.
template <typename T>
__global__ __launch_bounds__(256) void im2col3x3_dil_kernel(const T* __restrict__ x, T* __restrict__ cols, int H,
                                                            int W, int C, int dil, long long ld, long long total) {
    constexpr int V = V16<T>::N;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int cpr = (int)(ld / V);
    const long long m = idx / cpr;
    const int col = (int)(idx - m * cpr) * V;
    float f[V];
#pragma unroll
    for (int j = 0; j < V; ++j) f[j] = 0.f;
    if (col < 9 * C) {
        const int tap = col / C, c = col - tap * C;
        const int ky = tap / 3, kx = tap - ky * 3;
        const int ox = (int)(m % W), oy = (int)((m / W) % H);
        const long long b = m / ((long long)W * H);
        const long long iy = (long long)oy + (long long)(ky - 1) * dil, ix = (long long)ox + (long long)(kx - 1) * dil;
        if (iy >= 0 && iy < H && ix >= 0 && ix < W)
            Chunk<T, V>::ld(x + ((size_t)(b * H + iy) * W + (size_t)ix) * C + c, f);
    }
    Chunk<T, V>::st(cols + (size_t)m * ld + col, f);
}

// ------------------------------------------------------------------ depthwise 3x3 (stride 1, pad = d)
// y[b, y, x, c] = sum_{ky,kx} w[c, ky, kx] x[b, y + (ky-1) d, x + (kx-1) d, c]; flip: w[c, 2-ky, 2-kx] (the data
// gradient).  A thread owns one (column, V-channel chunk) and DW_ROWS consecutive rows; its 9 V weights stay in
// registers over the rows.  Row taps are uniform over the block (blockIdx.y picks the rows), column taps per thread.
constexpr int DW_ROWS = 4;
template <typename T>
__global__ __launch_bounds__(256) void dwconv3x3_fwd_kernel(const T* __restrict__ x, const float* __restrict__ w,
                                                            T* __restrict__ y, int H, int W, int C, int dil,
                                                            int flip) {
    constexpr int V = V16<T>::N;
    const unsigned cpr = (unsigned)(C / V);
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    const unsigned ux = t / cpr;
    if (ux >= (unsigned)W) return;
    const int ox = (int)ux, c = (int)(t - ux * cpr) * V;
    const int b = blockIdx.z;
    // the chunk's 9 V weights are contiguous ([C][9], c % V == 0: 16-byte aligned): 16-byte loads, then a register shuffle
    float wl[9 * V], wr[9][V];
#pragma unroll
    for (int q = 0; q < 9 * V / 4; ++q) {
        const f32x4 r = *(const f32x4*)(w + (size_t)c * 9 + 4 * q);
#pragma unroll
        for (int j = 0; j < 4; ++j) wl[4 * q + j] = r[j];
    }
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int j = 0; j < V; ++j) wr[tap][j] = flip ? wl[j * 9 + 8 - tap] : wl[j * 9 + tap];
    // dil can exceed the map: compare in 64 bits, never form ox +- dil as an index first
    const bool left = (long long)ox - dil >= 0, right = (long long)ox + dil < W;
    const int y_end = min((int)(blockIdx.y + 1) * DW_ROWS, H);
    for (int oy = blockIdx.y * DW_ROWS; oy < y_end; ++oy) {
        float acc[V];
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = 0.f;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const long long iy = (long long)oy + (long long)(ky - 1) * dil;
            if (iy < 0 || iy >= H) continue;   // uniform over the block: the whole tap row is skipped
            const T* row = x + ((size_t)b * H + (size_t)iy) * W * C + c;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                if ((kx == 0 && !left) || (kx == 2 && !right)) continue;
                const int ix = ox + (kx - 1) * dil;   // in [0, W) by the test above
                float f[V];
                Chunk<T, V>::ld(row + (size_t)ix * C, f);
#pragma unroll
                for (int j = 0; j < V; ++j) acc[j] = __builtin_fmaf(wr[ky * 3 + kx][j], f[j], acc[j]);
            }
        }
        Chunk<T, V>::st(y + (((size_t)b * H + oy) * W + ox) * C + c, acc);
    }
}

// dW[c, ky, kx] = sum_{b,y,x} dy[b, y, x, c] x[b, y + (ky-1) d, x + (kx-1) d, c].
// Block = cpb channel chunks x (256 / cpb) pixel lanes, cpb = min(C / V, 256) chosen at launch (304 channels: 38 chunks
// x 6 lanes; 2048: 256 x 1); lane l of block (gx, gy) is pixel slice gy * lanes + l and walks the pixels slice,
// slice + slices, ...; every thread writes its own fp32 partial row [slice][9][C] (a workgroup's `lanes` rows), the
// second kernel sums the slices in index order.
template <typename T>
__global__ __launch_bounds__(256) void dwconv3x3_wgrad_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                              float* __restrict__ part, int H, int W, int C, int dil,
                                                              long long pixels, int cpb) {
    constexpr int V = V16<T>::N;
    const int lanes = 256 / cpb, lane = (int)threadIdx.x / cpb;
    const int chunk = blockIdx.x * cpb + (int)threadIdx.x % cpb;
    if (lane >= lanes || chunk >= C / V) return;
    const int c = chunk * V;
    const long long slice = (long long)blockIdx.y * lanes + lane;
    const long long slices = (long long)gridDim.y * lanes;
    float acc[9][V];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int j = 0; j < V; ++j) acc[tap][j] = 0.f;
    for (long long p = slice; p < pixels; p += slices) {
        const int ox = (int)(p % W), oy = (int)((p / W) % H);
        const long long b = p / ((long long)W * H);
        float g[V];
        Chunk<T, V>::ld(dy + (size_t)p * C + c, g);
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const long long iy = (long long)oy + (long long)(ky - 1) * dil;
            if (iy < 0 || iy >= H) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const long long ix = (long long)ox + (long long)(kx - 1) * dil;
                if (ix < 0 || ix >= W) continue;
                float f[V];
                Chunk<T, V>::ld(x + ((size_t)(b * H + iy) * W + (size_t)ix) * C + c, f);
#pragma unroll
                for (int j = 0; j < V; ++j) acc[ky * 3 + kx][j] = __builtin_fmaf(g[j], f[j], acc[ky * 3 + kx][j]);
            }
        }
    }
    float* out = part + (size_t)slice * 9 * C + c;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
#pragma unroll
        for (int j = 0; j < V; ++j) out[(size_t)tap * C + j] = acc[tap][j];
    }
}
// dW[c][tap] (+)= sum over slices.  Block = 16 consecutive (tap, c) entries x 16 groups of consecutive slices: a thread
// sums its group in slice order, thread 0 of a column sums the 16 group totals in group order — a fixed order for a
// given shape, with enough loads in flight to stream tens of MB of partials.
__global__ __launch_bounds__(256) void dwconv3x3_wgrad_reduce_kernel(const float* __restrict__ part,
                                                                     float* __restrict__ dw, int C, int slices,
                                                                     int accumulate) {
    __shared__ float sh[16][17];
    const int il = threadIdx.x & 15, kg = threadIdx.x >> 4;
    const int idx = blockIdx.x * 16 + il;   // tap * C + c
    const int per = (slices + 15) / 16;
    const int k0 = kg * per, k1 = min(k0 + per, slices);
    float s = 0.f;
    if (idx < 9 * C) {
#pragma unroll 8
        for (int k = k0; k < k1; ++k) s += part[(size_t)k * 9 * C + idx];
    }
    sh[kg][il] = s;
    __syncthreads();
    if (kg != 0 || idx >= 9 * C) return;
    float t = 0.f;
#pragma unroll
    for (int g = 0; g < 16; ++g) t += sh[g][il];
    const int tap = idx / C, c = idx - tap * C;
    float* o = dw + (size_t)c * 9 + tap;
    *o = accumulate ? *o + t : t;
}

// ------------------------------------------------------------------ bilinear x s, align_corners=True
// the taps and weights of an output index: ac_src (map_chunk.h)
template <typename T, int V>
__global__ __launch_bounds__(256) void bilinear_up_ac_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, int H,
                                                                 int W, int C, int s) {
    const unsigned cpr = (unsigned)(C / V);
    const int Ho = s * H, Wo = s * W;
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    const unsigned uox = t / cpr;
    if (uox >= (unsigned)Wo) return;
    const int ox = (int)uox, c = (int)(t - uox * cpr) * V;
    const int oy = blockIdx.y, b = blockIdx.z;
    int y0, y1, x0, x1;
    float wy, wx;
    ac_src(oy, H, Ho, y0, y1, wy);
    ac_src(ox, W, Wo, x0, x1, wx);
    const T* base = x + (size_t)b * H * W * C + c;
    float f00[V], f01[V], f10[V], f11[V], o[V];
    Chunk<T, V>::ld(base + ((size_t)y0 * W + x0) * C, f00);
    Chunk<T, V>::ld(base + ((size_t)y0 * W + x1) * C, f01);
    Chunk<T, V>::ld(base + ((size_t)y1 * W + x0) * C, f10);
    Chunk<T, V>::ld(base + ((size_t)y1 * W + x1) * C, f11);
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const float top = __builtin_fmaf(1.f - wx, f00[j], f01[j] * wx);
        const float bot = __builtin_fmaf(1.f - wx, f10[j], f11[j] * wx);
        o[j] = __builtin_fmaf(1.f - wy, top, bot * wy);
    }
    Chunk<T, V>::st(y + (((size_t)b * Ho + oy) * Wo + ox) * C + c, o);
}
// candidate outputs of input index i: src in [i - 1, i + 1)  ->  o in [(i-1)(n_out-1)/(n_in-1), (i+1)(n_out-1)/(n_in-1)],
// widened by one on each side (the exact membership test is ac_src itself); a one-pixel input takes every output
DEVI void ac_candidates(int i, int n_in, int n_out, int& lo, int& hi) {
    if (n_in == 1) {
        lo = 0;
        hi = n_out - 1;
        return;
    }
    const long long num = n_out - 1, den = n_in - 1;
    const long long l = (long long)(i - 1) * num / den - 1, h = ((long long)(i + 1) * num + den - 1) / den + 1;
    lo = l > 0 ? (int)l : 0;
    hi = h < n_out - 1 ? (int)h : n_out - 1;
}
// gather form: an input pixel collects from every output pixel one of whose taps it is, in (row, column) order
template <typename T, int V>
__global__ __launch_bounds__(256) void bilinear_up_ac_bwd_kernel(const T* __restrict__ dy, T* __restrict__ dx, int H,
                                                                 int W, int C, int s) {
    const unsigned cpr = (unsigned)(C / V);
    const int Ho = s * H, Wo = s * W;
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    const unsigned uix = t / cpr;
    if (uix >= (unsigned)W) return;
    const int ix = (int)uix, c = (int)(t - uix * cpr) * V;
    const int iy = blockIdx.y, b = blockIdx.z;
    float acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.f;
    int oy_lo, oy_hi, ox_lo, ox_hi;
    ac_candidates(iy, H, Ho, oy_lo, oy_hi);
    ac_candidates(ix, W, Wo, ox_lo, ox_hi);
    for (int oy = oy_lo; oy <= oy_hi; ++oy) {
        int y0, y1;
        float wy;
        ac_src(oy, H, Ho, y0, y1, wy);
        float cy = 0.f;
        if (y0 == iy) cy += 1.f - wy;
        if (y1 == iy) cy += wy;
        if (cy == 0.f) continue;
        const T* row = dy + ((size_t)b * Ho + oy) * Wo * C + c;
        for (int ox = ox_lo; ox <= ox_hi; ++ox) {
            int x0, x1;
            float wx;
            ac_src(ox, W, Wo, x0, x1, wx);
            float cx = 0.f;
            if (x0 == ix) cx += 1.f - wx;
            if (x1 == ix) cx += wx;
            if (cx == 0.f) continue;
            float f[V];
            Chunk<T, V>::ld(row + (size_t)ox * C, f);
            const float wgt = cy * cx;
#pragma unroll
            for (int j = 0; j < V; ++j) acc[j] = __builtin_fmaf(wgt, f[j], acc[j]);
        }
    }
    Chunk<T, V>::st(dx + (((size_t)b * H + iy) * W + ix) * C + c, acc);
}

// ------------------------------------------------------------------ channel-slice copy (torch.cat / its gradient)
// dst[r, 0:C) = src[r / rep, 0:C) with row strides ldd / lds (elements): writes a branch into its channel slice of a
// concatenated map (rep = 1), broadcasts a per-image row over its rep = H W pixels (F.interpolate from 1x1), or reads
// a slice back into a dense map.
template <typename T, int V>
__global__ __launch_bounds__(256) void chan_copy_kernel(const T* __restrict__ src, long long lds, T* __restrict__ dst,
                                                        long long ldd, int C, long long rep, long long total) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int cpr = C / V;
    const long long r = idx / cpr;
    const int c = (int)(idx - r * cpr) * V;
    float f[V];
    Chunk<T, V>::ld(src + (size_t)(r / rep) * lds + c, f);
    Chunk<T, V>::st(dst + (size_t)r * ldd + c, f);
}

struct WgradGrid {
    unsigned gx, gy;
    int cpb;
    long long slices;
};
WgradGrid wgrad_grid(int dtype, long long pixels, int C) {
    WgradGrid g;
    const int cpr = C / vecn(dtype);
    g.cpb = cpr < 256 ? cpr : 256;
    g.gx = (unsigned)((cpr + g.cpb - 1) / g.cpb);
    const int lanes = 256 / g.cpb;
    const long long want = (pixels + 16LL * lanes - 1) / (16LL * lanes);   // >= 16 pixels per slice
    long long cap = 512 / g.gx > 0 ? 512 / g.gx : 1;                        // about two workgroups per CU ...
    const long long by_bytes = (64LL << 20) / (36LL * C * lanes);           // ... and at most 64 MiB of partials
    if (by_bytes < cap) cap = by_bytes > 0 ? by_bytes : 1;
    g.gy = (unsigned)(want < 1 ? 1 : (want > cap ? cap : want));
    g.slices = (long long)g.gy * lanes;
    return g;
}

}  // namespace

extern "C" int ssl4gie_im2col3x3_dil(const void* x, void* cols, int dtype, int B, int H, int W, int C, int dilation,
                                     long long ld, void* stream) {
    REQUIRE(x && cols && dt_ok(dtype) && B > 0 && H > 0 && W > 0 && C > 0 && dilation >= 1);
    REQUIRE(C % vecn(dtype) == 0 && ld >= 9LL * C && ld % vecn(dtype) == 0 && is16(x) && is16(cols));
    const long long total = (long long)B * H * W * (ld / vecn(dtype));
    REQUIRE((total + 255) / 256 <= 0x7fffffffLL);
    hipStream_t st = (hipStream_t)stream;
    MAP_LAUNCH(dtype, im2col3x3_dil_kernel, blocks_of(total), 256, (const T*)x, (T*)cols, H, W, C, dilation, ld, total);
    return 0;
}

extern "C" int ssl4gie_dwconv3x3_fwd(const void* x, const float* w, void* y, int dtype, int B, int H, int W, int C,
                                     int dilation, int flip, void* stream) {
    REQUIRE(x && w && y && x != y && dt_ok(dtype) && B > 0 && H > 0 && W > 0 && C > 0 && dilation >= 1);
    REQUIRE(C % 8 == 0 && is16(x) && is16(y) && (flip == 0 || flip == 1));
    const unsigned per_row = (unsigned)W * (unsigned)(C / vecn(dtype));
    const unsigned gy = (unsigned)((H + DW_ROWS - 1) / DW_ROWS);
    REQUIRE((long long)W * (C / vecn(dtype)) < (1LL << 31) && gy <= 65535 && B <= 65535);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((per_row + 255) / 256, gy, B), block(256);
    MAP_LAUNCH(dtype, dwconv3x3_fwd_kernel, grid, block, (const T*)x, w, (T*)y, H, W, C, dilation, flip);
    return 0;
}

extern "C" size_t ssl4gie_dwconv3x3_wgrad_workspace_bytes(int dtype, int B, int H, int W, int C) {
    if (!dt_ok(dtype) || B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 != 0) return 0;
    return (size_t)wgrad_grid(dtype, (long long)B * H * W, C).slices * 9 * (size_t)C * sizeof(float);
}
extern "C" int ssl4gie_dwconv3x3_wgrad(const void* dy, const void* x, float* dweight, void* workspace,
                                       size_t workspace_bytes, int dtype, int B, int H, int W, int C, int dilation,
                                       int accumulate, void* stream) {
    REQUIRE(dy && x && dweight && workspace && dt_ok(dtype) && B > 0 && H > 0 && W > 0 && C > 0 && dilation >= 1);
    REQUIRE(C % 8 == 0 && is16(dy) && is16(x) && is16(workspace));
    REQUIRE(workspace_bytes >= ssl4gie_dwconv3x3_wgrad_workspace_bytes(dtype, B, H, W, C));
    const long long pixels = (long long)B * H * W;
    const WgradGrid g = wgrad_grid(dtype, pixels, C);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(g.gx, g.gy), block(256);
    MAP_LAUNCH(dtype, dwconv3x3_wgrad_kernel, grid, block, (const T*)dy, (const T*)x, (float*)workspace, H, W, C,
               dilation, pixels, g.cpb);
    hipLaunchKernelGGL(dwconv3x3_wgrad_reduce_kernel, dim3((unsigned)((9LL * C + 15) / 16)), dim3(256), 0, st,
                       (const float*)workspace, dweight, C, (int)g.slices, accumulate ? 1 : 0);
    LAUNCH_CHECK();
    return 0;
}

static bool up_args_ok(const void* a, const void* b, int dtype, int B, int H, int W, int C, int scale) {
    return a && b && a != b && dt_ok(dtype) && B > 0 && H > 0 && W > 0 && C > 0 && scale >= 2 && B <= 65535 &&
           (long long)H * scale <= 65535 && (long long)W * scale * C < (1LL << 31);
}
extern "C" int ssl4gie_bilinear_up_ac_fwd(const void* x, void* y, int dtype, int B, int H, int W, int C, int scale,
                                          void* stream) {
    REQUIRE(up_args_ok(x, y, dtype, B, H, W, C, scale));
    const bool wide = C % vecn(dtype) == 0 && is16(x) && is16(y);
    const unsigned per_row = (unsigned)(W * scale) * (unsigned)(wide ? C / vecn(dtype) : C);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((per_row + 255) / 256, H * scale, B);
    MAP_LAUNCH_V(dtype, wide, bilinear_up_ac_fwd_kernel, grid, 256, (const T*)x, (T*)y, H, W, C, scale);
    return 0;
}
extern "C" int ssl4gie_bilinear_up_ac_bwd(const void* dy, void* dx, int dtype, int B, int H, int W, int C, int scale,
                                          void* stream) {
    REQUIRE(up_args_ok(dy, dx, dtype, B, H, W, C, scale));
    const bool wide = C % vecn(dtype) == 0 && is16(dy) && is16(dx);
    const unsigned per_row = (unsigned)W * (unsigned)(wide ? C / vecn(dtype) : C);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((per_row + 255) / 256, H, B);
    MAP_LAUNCH_V(dtype, wide, bilinear_up_ac_bwd_kernel, grid, 256, (const T*)dy, (T*)dx, H, W, C, scale);
    return 0;
}

extern "C" int ssl4gie_chan_copy(const void* src, long long lds, void* dst, long long ldd, int dtype, long long rows,
                                 int C, long long rep, void* stream) {
    REQUIRE(src && dst && dt_ok(dtype) && rows > 0 && C > 0 && rep >= 1 && lds >= C && ldd >= C);
    const int v = vecn(dtype);
    const bool wide = C % v == 0 && lds % v == 0 && ldd % v == 0 && is16(src) && is16(dst);
    const long long total = rows * (wide ? C / v : C);
    REQUIRE((total + 255) / 256 <= 0x7fffffffLL);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(blocks_of(total)), block(256);
    MAP_LAUNCH_V(dtype, wide, chan_copy_kernel, grid, block, (const T*)src, lds, (T*)dst, ldd, C, rep, total);
    return 0;
}
