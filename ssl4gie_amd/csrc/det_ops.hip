// Channels-last glue of the detection backbone's feature pyramid (reference
// ViTDet_FPN, Models/models.py:213-259): MaxPool2d(2), nn.LayerNorm((C, H, W)) — a per-image
// normalisation over the WHOLE map with a per-element affine — and nn.GELU on a map.  The 1x1 / 3x3
// convolutions and ConvTranspose2d(2, 2) of the pyramid are the GEMM paths of gemm*.hip.
//
// All of it is HBM-bound streaming: 16-byte accesses, two-stage deterministic reductions.
#include "reduce.h"
#include "internal.h"
#include "ssl4gie_hip.h"
#include "map_chunk.h"

// ------------------------------------------------------------------ MaxPool2d(kernel 2, stride 2)
// x [B, H, W, C] -> y [B, H/2, W/2, C]; backward routes dy to the FIRST maximum of the window in
// scan order (ATen's tie rule), recomputed from x (no index tensor); the selection is ATen's
// `v > best || isnan(v)`: a NaN anywhere in the window is the output and receives the gradient
template <typename T>
__global__ void maxpool2_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, int H, int W, int C,
                                    long long total) {
    constexpr int V = V16<T>::N;
    typedef typename V16<T>::raw raw_t;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int cpr = C / V, Ho = H / 2, Wo = W / 2;
    const int c = (int)(idx % cpr) * V;
    const long long p = idx / cpr;
    const int ox = (int)(p % Wo), oy = (int)((p / Wo) % Ho);
    const long long b = p / ((long long)Wo * Ho);
    float best[V];
#pragma unroll
    for (int j = 0; j < V; ++j) best[j] = -INFINITY;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        float v[V];
        un<T>(*(const raw_t*)(x + ((b * H + 2 * oy + (t >> 1)) * W + 2 * ox + (t & 1)) * C + c), v);
#pragma unroll
        for (int j = 0; j < V; ++j) best[j] = (v[j] > best[j] || v[j] != v[j]) ? v[j] : best[j];
    }
    *(raw_t*)(y + (size_t)p * C + c) = pk<T>(best);
}
template <typename T>
__global__ void maxpool2_bwd_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                    T* __restrict__ dx, int H, int W, int C, long long total) {
    constexpr int V = V16<T>::N;
    typedef typename V16<T>::raw raw_t;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;  // one output window
    if (idx >= total) return;
    const int cpr = C / V, Ho = H / 2, Wo = W / 2;
    const int c = (int)(idx % cpr) * V;
    const long long p = idx / cpr;
    const int ox = (int)(p % Wo), oy = (int)((p / Wo) % Ho);
    const long long b = p / ((long long)Wo * Ho);
    float v[4][V], g[V];
    un<T>(*(const raw_t*)(dy + (size_t)p * C + c), g);
#pragma unroll
    for (int t = 0; t < 4; ++t)
        un<T>(*(const raw_t*)(x + ((b * H + 2 * oy + (t >> 1)) * W + 2 * ox + (t & 1)) * C + c), v[t]);
    int win[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        win[j] = 0;
        float best = v[0][j];
#pragma unroll
        for (int t = 1; t < 4; ++t)
            if (v[t][j] > best || v[t][j] != v[t][j]) { best = v[t][j]; win[j] = t; }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        float o[V];
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = win[j] == t ? g[j] : 0.f;
        *(raw_t*)(dx + ((b * H + 2 * oy + (t >> 1)) * W + 2 * ox + (t & 1)) * C + c) = pk<T>(o);
    }
}

// ------------------------------------------------------------------ GELU on a map
template <typename T>
__global__ void gelu_map_kernel(const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ out,
                                long long total) {
    constexpr int V = V16<T>::N;
    typedef typename V16<T>::raw raw_t;
    const long long idx = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * V;
    if (idx >= total) return;
    float f[V];
    un<T>(*(const raw_t*)(x + idx), f);
    if (dy) {
        float g[V];
        un<T>(*(const raw_t*)(dy + idx), g);
#pragma unroll
        for (int j = 0; j < V; ++j) f[j] = g[j] * dgelu_f(f[j]);
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) f[j] = gelu_f(f[j]);
    }
    *(raw_t*)(out + idx) = pk<T>(f);
}

// ------------------------------------------------------------------ LayerNorm over whole maps
// x [B, M] (M = H*W*C elements of one image, channels-last), weight / bias fp32 [M] in the SAME
// element order.
//
// Forward statistics.  Block p of image b owns the 16-byte vectors p * 256 + t + k * 65536 (t: thread) and goes
// over them twice (the second time out of L2): their sum about 0 gives the part's first mean m0, the sums of
// d = x - m0 and d^2 its (mean, M2 = sum (x - mean)^2): partial[(b * parts + p) * 2 + {0, 1}].  The finalize
// kernel combines the 256 (count, mean, M2) triples (Chan et al.).  Every sum of squares is taken about a mean of
// the data it covers, so the variance does not depend on where an outlier sits; sums about the image's first
// element, as this kernel once took, lose var entirely when that element is the outlier
// (var = E[d^2] - E[d]^2 with both ~ (500 sigma)^2).
#define MLN_PARTS 256
__host__ __device__ inline long long mapln_part_vectors(long long nvec, int p) {  // vectors part p owns
    const long long rem = nvec % (MLN_PARTS * 256) - (long long)p * 256;
    return nvec / (MLN_PARTS * 256) * 256 + (rem < 0 ? 0 : rem > 256 ? 256 : rem);
}
template <typename T>
__global__ __launch_bounds__(256) void mapln_stats_kernel(const T* __restrict__ x, float* __restrict__ partial,
                                                          long long M) {
    constexpr int V = V16<T>::N;
    typedef typename V16<T>::raw raw_t;
    __shared__ float red[3][4];
    const int b = blockIdx.y, p = blockIdx.x;
    const T* xb = x + (size_t)b * M;
    const long long first = ((long long)p * 256 + threadIdx.x) * V, step = (long long)MLN_PARTS * 256 * V;
    const float n = (float)(mapln_part_vectors(M / V, p) * V);
    float s = 0.f;
    for (long long i = first; i < M; i += step) {
        float f[V];
        un<T>(*(const raw_t*)(xb + i), f);
#pragma unroll
        for (int j = 0; j < V; ++j) s += f[j];
    }
    const float m0 = n > 0.f ? block_sum_all<SumOrder::Pairwise>(s, red[0]) / n : 0.f;  // n is the same for the whole block
    s = 0.f;
    float q = 0.f;
    for (long long i = first; i < M; i += step) {
        float f[V];
        un<T>(*(const raw_t*)(xb + i), f);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float d = f[j] - m0;
            s += d;
            q += d * d;
        }
    }
    s = block_sum_all<SumOrder::Pairwise>(s, red[1]);
    q = block_sum_all<SumOrder::Pairwise>(q, red[2]);
    if (threadIdx.x == 0) {
        float* o = partial + ((size_t)b * MLN_PARTS + p) * 2;
        const float d = n > 0.f ? s / n : 0.f;
        const float m2 = q - s * d;
        o[0] = m0 + d;
        o[1] = m2 > 0.f ? m2 : 0.f;
    }
}
// one wave per image: mean = sum n_p mean_p / M, taken about 0 and then corrected about itself;
// M2 = sum (M2_p + n_p (mean_p - mean)^2)
__global__ __launch_bounds__(64) void mapln_stats_finalize_kernel(const float* __restrict__ partial,
                                                                  float* __restrict__ mean,
                                                                  float* __restrict__ rstd, long long M, int V,
                                                                  float eps) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const float n = (float)M;
    float np[MLN_PARTS / 64], mp[MLN_PARTS / 64], a = 0.f;
#pragma unroll
    for (int k = 0; k < MLN_PARTS / 64; ++k) {
        const int p = lane + 64 * k;
        np[k] = (float)(mapln_part_vectors(M / V, p) * V);
        mp[k] = partial[((size_t)b * MLN_PARTS + p) * 2];
        a += np[k] * mp[k];
    }
    const float m0 = wave_sum(a) / n;
    a = 0.f;
#pragma unroll
    for (int k = 0; k < MLN_PARTS / 64; ++k) a += np[k] * (mp[k] - m0);
    const float mu = m0 + wave_sum(a) / n;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < MLN_PARTS / 64; ++k) {
        const float e = mp[k] - mu;
        q += partial[((size_t)b * MLN_PARTS + lane + 64 * k) * 2 + 1] + np[k] * e * e;
    }
    q = wave_sum(q);
    if (lane != 0) return;
    mean[b] = mu;
    rstd[b] = rsqrtf(q / n + eps);
}
// backward sums: partial[(b * parts + p) * 2 + {0, 1}] = sum g, sum g xhat with g = dy * w
template <typename T>
__global__ __launch_bounds__(256) void mapln_reduce_kernel(
    const T* __restrict__ x, const T* __restrict__ dy, const float* __restrict__ w,
    const float* __restrict__ mean, const float* __restrict__ rstd, float* __restrict__ partial,
    long long M) {
    constexpr int V = V16<T>::N;
    typedef typename V16<T>::raw raw_t;
    __shared__ float red[2][4];
    const int b = blockIdx.y, p = blockIdx.x;
    const T* xb = x + (size_t)b * M;
    const float mu = mean[b], rs = rstd[b];
    float s = 0.f, q = 0.f;
    for (long long i = ((long long)p * 256 + threadIdx.x) * V; i < M; i += (long long)MLN_PARTS * 256 * V) {
        float f[V], g[V];
        un<T>(*(const raw_t*)(xb + i), f);
        un<T>(*(const raw_t*)(dy + (size_t)b * M + i), g);
#pragma unroll
        for (int j = 0; j < V; j += 4) {
            const f32x4 ww = ld4(w + i + j);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float gg = g[j + k] * ww[k];
                s += gg;
                q += gg * ((f[j + k] - mu) * rs);
            }
        }
    }
    s = wave_sum(s);
    q = wave_sum(q);
    block_put(s, red[0]); block_put(q, red[1]);
    __syncthreads();
    if (threadIdx.x == 0) {
        float* o = partial + ((size_t)b * MLN_PARTS + p) * 2;
        o[0] = block_get<SumOrder::Sequential>(red[0]);
        o[1] = block_get<SumOrder::Sequential>(red[1]);
    }
}
// one wave per image: fold the partials into the two means of dx
__global__ __launch_bounds__(64) void mapln_finalize_kernel(const float* __restrict__ partial,
                                                            float* __restrict__ o0, float* __restrict__ o1,
                                                            long long M) {
    const int b = blockIdx.x, lane = threadIdx.x;
    float s = 0.f, q = 0.f;
    for (int p = lane; p < MLN_PARTS; p += 64) {
        s += partial[((size_t)b * MLN_PARTS + p) * 2];
        q += partial[((size_t)b * MLN_PARTS + p) * 2 + 1];
    }
    s = wave_sum(s);
    q = wave_sum(q);
    if (lane != 0) return;
    const float n = (float)M;
    o0[b] = s / n;  // mean(g)
    o1[b] = q / n;  // mean(g xhat)
}
template <typename T>
__global__ void mapln_apply_kernel(const T* __restrict__ x, const float* __restrict__ w,
                                   const float* __restrict__ bias, const float* __restrict__ mean,
                                   const float* __restrict__ rstd, T* __restrict__ y, long long M,
                                   long long total) {
    constexpr int V = V16<T>::N;
    typedef typename V16<T>::raw raw_t;
    const long long idx = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * V;
    if (idx >= total) return;
    const int b = (int)(idx / M);
    const long long i = idx - (long long)b * M;
    const float mu = mean[b], rs = rstd[b];
    float f[V];
    un<T>(*(const raw_t*)(x + idx), f);
#pragma unroll
    for (int j = 0; j < V; j += 4) {
        const f32x4 ww = ld4(w + i + j), bb = ld4(bias + i + j);
#pragma unroll
        for (int k = 0; k < 4; ++k) f[j + k] = (f[j + k] - mu) * rs * ww[k] + bb[k];
    }
    *(raw_t*)(y + idx) = pk<T>(f);
}
// a thread owns V elements of the map for ALL images: dx for each image and the per-element
// dweight = sum_b dy xhat, dbias = sum_b dy in one pass
template <typename T>
__global__ void mapln_bwd_apply_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                       const float* __restrict__ w, const float* __restrict__ mean,
                                       const float* __restrict__ rstd, const float* __restrict__ mg,
                                       const float* __restrict__ mgx, T* __restrict__ dx,
                                       float* __restrict__ dw, float* __restrict__ db, int accumulate,
                                       int B, long long M) {
    constexpr int V = V16<T>::N;
    typedef typename V16<T>::raw raw_t;
    const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * V;
    if (i >= M) return;
    float ww[V], aw[V], ab[V];
#pragma unroll
    for (int j = 0; j < V; j += 4) {
        const f32x4 t = ld4(w + i + j);
#pragma unroll
        for (int k = 0; k < 4; ++k) { ww[j + k] = t[k]; aw[j + k] = 0.f; ab[j + k] = 0.f; }
    }
    for (int b = 0; b < B; ++b) {
        const float mu = mean[b], rs = rstd[b], m1 = mg[b], m2 = mgx[b];
        float f[V], g[V], o[V];
        un<T>(*(const raw_t*)(x + (size_t)b * M + i), f);
        un<T>(*(const raw_t*)(dy + (size_t)b * M + i), g);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float xh = (f[j] - mu) * rs;
            aw[j] += g[j] * xh;
            ab[j] += g[j];
            o[j] = rs * (g[j] * ww[j] - m1 - xh * m2);
        }
        *(raw_t*)(dx + (size_t)b * M + i) = pk<T>(o);
    }
#pragma unroll
    for (int j = 0; j < V; j += 4) {
        f32x4 tw = {aw[j], aw[j + 1], aw[j + 2], aw[j + 3]}, tb = {ab[j], ab[j + 1], ab[j + 2], ab[j + 3]};
        if (dw) { if (accumulate) tw += ld4(dw + i + j); st4(dw + i + j, tw); }
        if (db) { if (accumulate) tb += ld4(db + i + j); st4(db + i + j, tb); }
    }
}

// =====================================================================================
extern "C" int ssl4gie_maxpool2x2_fwd(const void* x, void* y, int dtype, int B, int H, int W, int C,
                                      void* stream) {
    REQUIRE(x && y && dt_ok(dtype) && B > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0 &&
            C % vecn(dtype) == 0);
    hipStream_t st = (hipStream_t)stream;
    const long long total = (long long)B * (H / 2) * (W / 2) * (C / vecn(dtype));
    MAP_LAUNCH(dtype, maxpool2_fwd_kernel, blocks_of(total), 256, (const T*)x, (T*)y, H, W, C, total);
    return 0;
}
extern "C" int ssl4gie_maxpool2x2_bwd(const void* x, const void* dy, void* dx, int dtype, int B, int H,
                                      int W, int C, void* stream) {
    REQUIRE(x && dy && dx && dt_ok(dtype) && B > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0 &&
            C % vecn(dtype) == 0);
    hipStream_t st = (hipStream_t)stream;
    const long long total = (long long)B * (H / 2) * (W / 2) * (C / vecn(dtype));
    MAP_LAUNCH(dtype, maxpool2_bwd_kernel, blocks_of(total), 256, (const T*)x, (const T*)dy, (T*)dx, H, W, C, total);
    return 0;
}
// dy == NULL: out = gelu(x) (exact erf form, nn.GELU);  dy != NULL: out = dy * gelu'(x)
extern "C" int ssl4gie_gelu_map(const void* x, const void* dy, void* out, int dtype, long long n,
                                void* stream) {
    REQUIRE(x && out && dt_ok(dtype) && n >= 0 && n % vecn(dtype) == 0);
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    MAP_LAUNCH(dtype, gelu_map_kernel, blocks_of(n / vecn(dtype)), 256, (const T*)x, (const T*)dy, (T*)out, n);
    return 0;
}
extern "C" size_t ssl4gie_map_layernorm_workspace_bytes(int B) {
    return ((size_t)B * MLN_PARTS * 2 + 2 * (size_t)B) * sizeof(float);  // partials, two means
}
// y[b, i] = (x[b, i] - mean_b) rstd_b w[i] + bias[i]; mean / rstd [B] are outputs kept for backward
extern "C" int ssl4gie_map_layernorm_fwd(const void* x, const float* w, const float* bias, void* y,
                                         float* mean, float* rstd, float eps, float* workspace,
                                         int dtype, int B, long long M, void* stream) {
    REQUIRE(x && w && bias && y && mean && rstd && workspace && dt_ok(dtype) && B > 0 && M > 0 &&
            M % 8 == 0 && B <= 65535);
    hipStream_t st = (hipStream_t)stream;
    dim3 grid(MLN_PARTS, B), block(256);
    MAP_LAUNCH(dtype, mapln_stats_kernel, grid, block, (const T*)x, workspace, M);
    hipLaunchKernelGGL(mapln_stats_finalize_kernel, dim3(B), dim3(64), 0, st, workspace, mean, rstd, M, vecn(dtype),
                       eps);
    LAUNCH_CHECK();
    const long long total = (long long)B * M;
    MAP_LAUNCH(dtype, mapln_apply_kernel, blocks_of(total / vecn(dtype)), 256, (const T*)x, w, bias, mean, rstd, (T*)y,
               M, total);
    return 0;
}
// dx, and dw / db [M] overwritten (accumulate = 0) or accumulated (either may be NULL)
extern "C" int ssl4gie_map_layernorm_bwd(const void* x, const void* dy, const float* w,
                                         const float* mean, const float* rstd, void* dx, float* dw,
                                         float* db, int accumulate, float* workspace, int dtype, int B,
                                         long long M, void* stream) {
    REQUIRE(x && dy && w && mean && rstd && dx && workspace && dt_ok(dtype) && B > 0 && M > 0 &&
            M % 8 == 0 && B <= 65535);
    hipStream_t st = (hipStream_t)stream;
    dim3 grid(MLN_PARTS, B), block(256);
    float* mg = workspace + (size_t)B * MLN_PARTS * 2;
    float* mgx = mg + B;
    MAP_LAUNCH(dtype, mapln_reduce_kernel, grid, block, (const T*)x, (const T*)dy, w, mean, rstd, workspace, M);
    hipLaunchKernelGGL(mapln_finalize_kernel, dim3(B), dim3(64), 0, st, workspace, mg, mgx, M);
    LAUNCH_CHECK();
    MAP_LAUNCH(dtype, mapln_bwd_apply_kernel, blocks_of(M / vecn(dtype)), 256, (const T*)x, (const T*)dy, w, mean, rstd,
               mg, mgx, (T*)dx, dw, db, accumulate, B, M);
    return 0;
}
