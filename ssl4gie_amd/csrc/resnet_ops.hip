// ResNet50 glue for gfx950: everything around the convolution GEMMs of
// torchvision's ResNet(Bottleneck, [3, 4, 6, 3]) as the reference uses it (Models/models.py:63-152,
// Models/moco_v3/main_moco.py:185-187).  Maps are channels-last [B, H, W, C] in the operand type, so
// a 1x1 convolution is a token-major GEMM and BatchNorm2d statistics are column sums over M = B*H*W
// rows.  All HBM-bound: 16-byte accesses, two-stage deterministic reductions (no atomics).
//
//   stem_im2col7x7   fp32 NCHW image -> patch matrix of conv1 (7x7, stride 2, pad 3), K = 147 (+pad)
//   subsample2       rows of a stride-2 1x1 convolution (downsample.0) and its gradient
//   bn_stats         per-channel sum / sum of squares partials  (+ tail: mean, rstd, coefficients)
//   bn_apply         y = act((x - mean) rstd gamma + beta (+ residual))     act = ReLU | id
//   bn_bwd_reduce    partials of sum(dy) and sum(dy * xhat) over the rows (dy already ReLU-masked)
//   bn_bwd_apply     dx = gamma rstd (g - mean(g) - xhat mean(g xhat)); optional dres = g
//   bn_bwd_frozen    fixed statistics (evaluation mode, FrozenBatchNorm2d): dx = gamma rstd g in one pass
//   maxpool3x3s2     forward with argmax byte, backward in gather form
//   avgpool          global average per image and its gradient
#include "common.h"
#include "prof.h"
#include "ssl4gie_hip.h"
#include "internal.h"
#include "map_chunk.h"

// ------------------------------------------------------------------ stem patch matrix
// cols[(b, oy, ox), (dy*7 + dx)*3 + c] = img[b, c, 2 oy + dy - 3, 2 ox + dx - 3]; [147, ld) zero
template <typename T>
__global__ void stem_im2col_kernel(const float* __restrict__ img, T* __restrict__ cols, int B, int H,
                                   int W, int Ho, int Wo, long long ld, long long total) {
    // one thread = 8 consecutive columns of one output row (ld % 8 == 0): a 16-B (bf16) store
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int cpr = (int)(ld >> 3);
    const long long m = idx / cpr;
    const int col0 = (int)(idx % cpr) * 8;
    const int ox = (int)(m % Wo), oy = (int)((m / Wo) % Ho), b = (int)(m / ((long long)Wo * Ho));
    const float* base = img + (size_t)b * 3 * H * W;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int col = col0 + j;
        v[j] = 0.f;
        if (col < 147) {
            const int tap = col / 3, c = col - tap * 3, dy = tap / 7, dx = tap - dy * 7;
            const int iy = 2 * oy + dy - 3, ix = 2 * ox + dx - 3;
            if (iy >= 0 && iy < H && ix >= 0 && ix < W) v[j] = base[((size_t)c * H + iy) * W + ix];
        }
    }
    T* dst = cols + (size_t)m * ld + col0;
#pragma unroll
    for (int j = 0; j < 8; j += 4) st4(dst + j, f32x4{v[j], v[j + 1], v[j + 2], v[j + 3]});
}

// ------------------------------------------------------------------ stride-2 row subsampling
template <typename T>
__global__ void subsample2_kernel(const T* __restrict__ x, T* __restrict__ y, int H, int W, int C,
                                  int Ho, int Wo, long long total) {
    constexpr int V = V16<T>::N;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int cpr = C / V;
    const long long p = idx / cpr;
    const int c = (int)(idx % cpr) * V;
    const int ox = (int)(p % Wo), oy = (int)((p / Wo) % Ho);
    const long long b = p / ((long long)Wo * Ho);
    *(typename V16<T>::raw*)(y + (size_t)p * C + c) =
        *(const typename V16<T>::raw*)(x + ((b * H + 2 * oy) * W + 2 * ox) * C + c);
}
template <typename T>
__global__ void subsample2_bwd_kernel(const T* __restrict__ dy, T* __restrict__ dx, int H, int W,
                                      int C, int Ho, int Wo, long long total) {
    constexpr int V = V16<T>::N;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int cpr = C / V;
    const long long p = idx / cpr;
    const int c = (int)(idx % cpr) * V;
    const int x = (int)(p % W), y = (int)((p / W) % H);
    const long long b = p / ((long long)W * H);
    typename V16<T>::raw v = {};
    if (!(x & 1) && !(y & 1))
        v = *(const typename V16<T>::raw*)(dy + ((b * Ho + (y >> 1)) * Wo + (x >> 1)) * C + c);
    *(typename V16<T>::raw*)(dx + (size_t)p * C + c) = v;
}

// ------------------------------------------------------------------ BatchNorm (training mode)
// partial[blockIdx.y][0][c] = sum_r x[r, c], partial[..][1][c] = sum_r x^2 over this block's rows
// (sums are taken about the pivot x[0, c] — written to `pivot` — so that E[d^2] - E[d]^2 does not
// cancel catastrophically when |mean| >> std).
// Lane mapping (both reductions): a lane owns V = 16 B / sizeof(T) channels (one dwordx4 load).  With
// C / V >= 64 a wave spans 64 V channels of one row and gridDim.x strips cover C; with fewer
// (power-of-two) channel groups a wave folds 64 / (C / V) rows per step and lanes of equal channel
// group are combined by shuffles at the end.  A wave step therefore reads 1 KiB of contiguous
// memory, and four steps are in flight per lane (the pass is pure HBM streaming: ~4 KiB per wave
// outstanding x 16 waves per CU is what it takes to cover the latency).
struct BnLanes {
    int lpr, rpw, c, rsub;
};
template <int V>
DEVI BnLanes bn_lanes(int C, int lane) {
    BnLanes m;
    const int cg = C / V;
    m.lpr = (cg < 64 && !(cg & (cg - 1))) ? cg : 64;  // fold only powers of two
    m.rpw = 64 / m.lpr;
    m.c = (blockIdx.x * 64 + (lane % m.lpr)) * V;
    m.rsub = lane / m.lpr;
    return m;
}
// combine the folded rows of a wave, then the 4 waves of the block; result in wave 0, rsub == 0
template <int V>
DEVI void bn_block_reduce(float (&s)[V], float (&q)[V], float (*red)[2][64][V], int lpr, int lane,
                          int wave) {
    for (int o = lpr; o < 64; o <<= 1) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            s[j] += __shfl_xor(s[j], o, 64);
            q[j] += __shfl_xor(q[j], o, 64);
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int j = 0; j < V; ++j) { red[wave - 1][0][lane][j] = s[j]; red[wave - 1][1][lane][j] = q[j]; }
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int w = 0; w < 3; ++w)
#pragma unroll
            for (int j = 0; j < V; ++j) { s[j] += red[w][0][lane][j]; q[j] += red[w][1][lane][j]; }
    }
}
template <typename T>
__global__ __launch_bounds__(256) void bn_stats_kernel(const T* __restrict__ x,
                                                       float* __restrict__ partial,
                                                       float* __restrict__ pivot, long long rows,
                                                       int C) {
    constexpr int V = V16<T>::N;
    typedef typename V16<T>::raw raw_t;
    __shared__ float red[3][2][64][V];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const BnLanes m = bn_lanes<V>(C, lane);
    float s[V], q[V];
#pragma unroll
    for (int j = 0; j < V; ++j) s[j] = q[j] = 0.f;
    if (m.c < C) {
        float piv[V];
        un<T>(*(const raw_t*)(x + m.c), piv);
        if (blockIdx.y == 0 && wave == 0 && m.rsub == 0) {
#pragma unroll
            for (int j = 0; j < V; ++j) pivot[m.c + j] = piv[j];
        }
        auto acc = [&](const raw_t& v) {
            float f[V];
            un<T>(v, f);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float d = f[j] - piv[j];
                s[j] += d;
                q[j] += d * d;
            }
        };
        const long long step = (long long)gridDim.y * 4 * m.rpw;
        long long r = ((long long)blockIdx.y * 4 + wave) * m.rpw + m.rsub;
        const T* px = x + m.c;
        for (; r + 3 * step < rows; r += 4 * step) {
            const raw_t v0 = *(const raw_t*)(px + (size_t)r * C);
            const raw_t v1 = *(const raw_t*)(px + (size_t)(r + step) * C);
            const raw_t v2 = *(const raw_t*)(px + (size_t)(r + 2 * step) * C);
            const raw_t v3 = *(const raw_t*)(px + (size_t)(r + 3 * step) * C);
            acc(v0); acc(v1); acc(v2); acc(v3);
        }
        for (; r < rows; r += step) acc(*(const raw_t*)(px + (size_t)r * C));
    }
    bn_block_reduce<V>(s, q, red, m.lpr, lane, wave);
    if (wave == 0 && m.c < C && m.rsub == 0) {
        float* p = partial + (size_t)blockIdx.y * 2 * C;
#pragma unroll
        for (int j = 0; j < V; j += 4) {
            st4(p + m.c + j, f32x4{s[j], s[j + 1], s[j + 2], s[j + 3]});
            st4(p + C + m.c + j, f32x4{q[j], q[j + 1], q[j + 2], q[j + 3]});
        }
    }
}
// per-channel affine of the normalisation: y = x * coef[c] + coef[C + c]
// the forward's normalisation coefficients y = x a + b; ONE definition, because the backward kernels that rebuild
// the ReLU mask from x (xmask) must reproduce the forward's sign decisions
DEVI void bn_affine(float gamma, float beta, float mean, float rstd, float& a, float& b) {
    a = rstd * gamma;
    b = beta - mean * a;
}
__global__ void bn_fwd_coef_kernel(const float* __restrict__ mean, const float* __restrict__ rstd,
                                   const float* __restrict__ gamma, const float* __restrict__ beta,
                                   float* __restrict__ coef, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float a, b;
    bn_affine(gamma ? gamma[c] : 1.f, beta ? beta[c] : 0.f, mean[c], rstd[c], a, b);
    coef[c] = a;
    coef[C + c] = b;
}
// dx = coef[c] g + coef[C+c] (x - mu[c]) + coef[2C+c]   (gamma rstd (g - s1/n - xhat s2/n) with xhat = (x - mean) rstd)
// x is centred BEFORE the product: folding mean into the constant term (coef[C+c] x + const) cancels two numbers of
// size |mean| rstd |s2/n| and loses |mean| rstd bits of dx — unbounded when a small batch sits far from 0.
// mu: a 16-byte-aligned copy of mean for the apply kernel's vector loads (callers' mean may be a slice)
__global__ void bn_bwd_coef_kernel(const float* __restrict__ mean, const float* __restrict__ rstd,
                                   const float* __restrict__ gamma, const float* __restrict__ sums,
                                   float inv_n, float* __restrict__ coef, int C, float* __restrict__ mu) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float r = rstd[c], a = r * (gamma ? gamma[c] : 1.f);
    const float s1 = sums[c] * inv_n, s2 = sums[C + c] * inv_n;
    coef[c] = a;
    coef[C + c] = -a * r * s2;
    coef[2 * C + c] = -a * s1;
    mu[c] = mean[c];
}
// Tails of the single-GPU BatchNorm: the partition partials are summed by 4 waves x 64 channels per
// block (a fixed order: deterministic), and the per-channel results are finished in the same
// launch — forward: mean / rstd / running statistics / normalisation coefficients; backward:
// dx coefficients and dgamma / dbeta.  One launch instead of three (four) ~5 us ones per layer.
DEVI bool bn_sum_partials(const float* __restrict__ partial, int parts, int C, float& s, float& q,
                          float (*red)[2][64]) {
    // 4 waves per block, or 16 (BN_TAIL_WIDE: a few hundred to two thousand partial rows summed in ONE launch,
    // without the 64-way fold in front — two ~5 us launches become one)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    s = 0.f; q = 0.f;
    if (c < C) {
        // eight rows' loads in flight, then the adds in row order (the sums are those of the plain loop; a
        // dependent load per row cost up to 64 L2 round trips in this kernel's one wave per 64 channels)
        int p = wave;
        for (; p + 7 * nw < parts; p += 8 * nw) {
            float a[8], b[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                a[u] = partial[(size_t)(p + nw * u) * 2 * C + c];
                b[u] = partial[(size_t)(p + nw * u) * 2 * C + C + c];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) { s += a[u]; q += b[u]; }
        }
        for (; p < parts; p += nw) {
            s += partial[(size_t)p * 2 * C + c];
            q += partial[(size_t)p * 2 * C + C + c];
        }
    }
    if (wave > 0) { red[wave - 1][0][lane] = s; red[wave - 1][1][lane] = q; }
    __syncthreads();
    if (wave != 0 || c >= C) return false;
    for (int w = 0; w < nw - 1; ++w) { s += red[w][0][lane]; q += red[w][1][lane]; }
    return true;
}
__global__ __launch_bounds__(1024) void bn_fwd_tail_kernel(
    const float* __restrict__ partial, int parts, const float* __restrict__ pivot,
    const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ mean,
    float* __restrict__ rstd, float* __restrict__ running_mean, float* __restrict__ running_var,
    float* __restrict__ coef, float count, float eps, float momentum, int C) {
    __shared__ float red[15][2][64];
    float s, q;
    if (!bn_sum_partials(partial, parts, C, s, q, red)) return;
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    const float d = s / count;
    float var = q / count - d * d;
    var = var > 0.f ? var : 0.f;
    const float m = (pivot ? pivot[c] : 0.f) + d, r = rsqrtf(var + eps);
    mean[c] = m;
    rstd[c] = r;
    if (running_mean) {
        const float unbiased = count > 1.f ? var * count / (count - 1.f) : var;
        running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * m;
        running_var[c] = (1.f - momentum) * running_var[c] + momentum * unbiased;
    }
    float a, b;
    bn_affine(gamma ? gamma[c] : 1.f, beta ? beta[c] : 0.f, m, r, a, b);
    coef[c] = a;
    coef[C + c] = b;
}
__global__ __launch_bounds__(1024) void bn_bwd_tail_kernel(
    const float* __restrict__ partial, int parts, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ gamma, float inv_n,
    float* __restrict__ coef, float* __restrict__ dgamma, float* __restrict__ dbeta,
    int accumulate, int C, const float* __restrict__ beta, float* __restrict__ mcoef, float* __restrict__ mu) {
    __shared__ float red[15][2][64];
    float s, q;
    if (!bn_sum_partials(partial, parts, C, s, q, red)) return;
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    if (mcoef) {  // the forward's y = x a + b, for the apply pass's ReLU mask
        float ma, mb;
        bn_affine(gamma ? gamma[c] : 1.f, beta ? beta[c] : 0.f, mean[c], rstd[c], ma, mb);
        mcoef[c] = ma;
        mcoef[C + c] = mb;
    }
    const float r = rstd[c], a = r * (gamma ? gamma[c] : 1.f);
    const float s1 = s * inv_n, s2 = q * inv_n;
    coef[c] = a;
    coef[C + c] = -a * r * s2;
    coef[2 * C + c] = -a * s1;
    mu[c] = mean[c];
    if (dbeta) dbeta[c] = accumulate ? dbeta[c] + s : s;
    if (dgamma) dgamma[c] = accumulate ? dgamma[c] + q : q;
}
// y = act(x coef[c] + coef[C + c] (+ res));  bits (optional, bf16 only: 8 elements per thread = one byte):
// bit j of bits[idx / 8] = (y[idx + j] > 0) — the ReLU mask the backward needs, at 1/16 of y's bytes
template <typename T>
__global__ void bn_apply_kernel(const T* __restrict__ x, const float* __restrict__ coef,
                                const T* __restrict__ res, T* __restrict__ y, int relu, int C,
                                long long total, unsigned char* __restrict__ bits) {
    constexpr int V = V16<T>::N;
    const long long idx = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * V;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    float f[V], r[V], a[V], b[V];
    un<T>(*(const typename V16<T>::raw*)(x + idx), f);
    if (res) un<T>(*(const typename V16<T>::raw*)(res + idx), r);
#pragma unroll
    for (int j = 0; j < V; j += 4) {
        *(f32x4*)(a + j) = ld4(coef + c + j);
        *(f32x4*)(b + j) = ld4(coef + C + c + j);
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
        float v = f[j] * a[j] + b[j];
        if (res) v += r[j];
        f[j] = (relu && v < 0.f) ? 0.f : v;
    }
    const typename V16<T>::raw out = pk<T>(f);
    *(typename V16<T>::raw*)(y + idx) = out;
    if constexpr (V == 8) {
        if (bits) {  // of the ROUNDED outputs: what `y > 0` reads back
            float r2[V];
            un<T>(out, r2);
            unsigned m = 0;
#pragma unroll
            for (int j = 0; j < V; ++j) m |= (r2[j] > 0.f ? 1u : 0u) << j;
            bits[idx >> 3] = (unsigned char)m;
        }
    }
}
// g = relu ? (y > 0 ? dy : 0) : dy;  partial[blk][0][c] = sum g, [1][c] = sum g * xhat; when the block
// had a residual input its gradient is g itself (dres, optional).  Lane mapping as bn_stats_kernel,
// two rows (x 2-3 streams) in flight per lane.
// XMASK (BatchNorm + ReLU without a residual input): the mask is rebuilt as x a + b > 0 from the forward's own
// coefficients instead of read from the ReLU output — two streams instead of three.
// XMASK == 2 (BITS): the mask comes from the forward's bit map (`y` points at it): one byte per 8 elements.
template <typename T, int XMASK>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(
    const T* __restrict__ dy, const T* __restrict__ y, const T* __restrict__ x,
    const float* __restrict__ mean, const float* __restrict__ rstd, T* __restrict__ dres,
    float* __restrict__ partial, int relu, long long rows, int C,
    const float* __restrict__ gamma, const float* __restrict__ beta) {
    constexpr int V = V16<T>::N;
    typedef typename V16<T>::raw raw_t;
    __shared__ float red[3][2][64][V];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const BnLanes m = bn_lanes<V>(C, lane);
    float s[V], q[V];
#pragma unroll
    for (int j = 0; j < V; ++j) s[j] = q[j] = 0.f;
    if (m.c < C) {
        float mu[V], rs[V];
        [[maybe_unused]] float ma[V], mb[V];
#pragma unroll
        for (int j = 0; j < V; ++j) { mu[j] = mean[m.c + j]; rs[j] = rstd[m.c + j]; }
        if constexpr (XMASK == 1) {
#pragma unroll
            for (int j = 0; j < V; ++j)
                bn_affine(gamma ? gamma[m.c + j] : 1.f, beta ? beta[m.c + j] : 0.f, mu[j], rs[j], ma[j], mb[j]);
        }
        [[maybe_unused]] const unsigned char* bits = (const unsigned char*)y;
        auto acc = [&](const raw_t& gv, const raw_t& yv, const raw_t& xv, size_t o) {
            float g[V], xx[V];
            un<T>(gv, g);
            un<T>(xv, xx);
            if constexpr (XMASK == 1) {
#pragma unroll
                for (int j = 0; j < V; ++j) g[j] = xx[j] * ma[j] + mb[j] > 0.f ? g[j] : 0.f;
            } else if constexpr (XMASK == 2) {
                const unsigned mk = (unsigned)yv[0];  // the byte, carried in the first word of `yv`
#pragma unroll
                for (int j = 0; j < V; ++j) g[j] = ((mk >> j) & 1u) ? g[j] : 0.f;
            } else if (relu) {
                float yy[V];
                un<T>(yv, yy);
#pragma unroll
                for (int j = 0; j < V; ++j) g[j] = yy[j] > 0.f ? g[j] : 0.f;
            }
            if (dres) *(raw_t*)(dres + o) = relu ? pk<T>(g) : gv;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                s[j] += g[j];
                q[j] += g[j] * ((xx[j] - mu[j]) * rs[j]);
            }
        };
        const long long step = (long long)gridDim.y * 4 * m.rpw;
        long long r = ((long long)blockIdx.y * 4 + wave) * m.rpw + m.rsub;
        constexpr int NR = XMASK ? 4 : 2;  // rows in flight per lane: ~8 16-B loads outstanding either way
        auto mask_of = [&](size_t o) -> raw_t {  // XMASK == 2: this row's byte of the bit map, in word 0
            raw_t r = {};
            if constexpr (XMASK == 2 && V == 8) r[0] = bits[o >> 3];
            return r;
        };
        for (; r + (NR - 1) * step < rows; r += NR * step) {
            size_t o[NR];
            raw_t gv[NR], xv[NR], yv[NR];
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                o[i] = (size_t)(r + i * step) * C + m.c;
                gv[i] = *(const raw_t*)(dy + o[i]);
                xv[i] = *(const raw_t*)(x + o[i]);
                yv[i] = gv[i];
                if (XMASK == 2) yv[i] = mask_of(o[i]);
                if (!XMASK && relu) yv[i] = *(const raw_t*)(y + o[i]);
            }
#pragma unroll
            for (int i = 0; i < NR; ++i) acc(gv[i], yv[i], xv[i], o[i]);
        }
        for (; r < rows; r += step) {
            const size_t o0 = (size_t)r * C + m.c;
            const raw_t g0 = *(const raw_t*)(dy + o0), x0 = *(const raw_t*)(x + o0);
            raw_t y0 = g0;
            if (XMASK == 2) y0 = mask_of(o0);
            if (!XMASK && relu) y0 = *(const raw_t*)(y + o0);
            acc(g0, y0, x0, o0);
        }
    }
    bn_block_reduce<V>(s, q, red, m.lpr, lane, wave);
    if (wave == 0 && m.c < C && m.rsub == 0) {
        float* p = partial + (size_t)blockIdx.y * 2 * C;
#pragma unroll
        for (int j = 0; j < V; j += 4) {
            st4(p + m.c + j, f32x4{s[j], s[j + 1], s[j + 2], s[j + 3]});
            st4(p + C + m.c + j, f32x4{q[j], q[j + 1], q[j + 2], q[j + 3]});
        }
    }
}
// dx = coef[c] g + coef[C + c] (x - mu[c]) + coef[2C + c];  mcoef (optional, [2][C]): g = x mcoef[c] + mcoef[C + c] > 0 ? dy : 0
template <typename T>
__global__ void bn_bwd_apply_kernel(const T* __restrict__ dy, const T* __restrict__ y,
                                    const T* __restrict__ x, const float* __restrict__ coef,
                                    T* __restrict__ dx, int relu, int C, long long total,
                                    const float* __restrict__ mcoef, const float* __restrict__ mu) {
    constexpr int V = V16<T>::N;
    const long long idx = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * V;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    float g[V], xv[V], yy[V], a[V], b[V], d[V], m[V];
    un<T>(*(const typename V16<T>::raw*)(dy + idx), g);
    un<T>(*(const typename V16<T>::raw*)(x + idx), xv);
    if (mcoef) {  // the forward's pre-activation, sign only
#pragma unroll
        for (int j = 0; j < V; j += 4) {
            const f32x4 ma = ld4(mcoef + c + j), mb = ld4(mcoef + C + c + j);
#pragma unroll
            for (int i = 0; i < 4; ++i) yy[j + i] = xv[j + i] * ma[i] + mb[i];
        }
    } else if (relu) {
        un<T>(*(const typename V16<T>::raw*)(y + idx), yy);
    }
#pragma unroll
    for (int j = 0; j < V; j += 4) {
        *(f32x4*)(a + j) = ld4(coef + c + j);
        *(f32x4*)(b + j) = ld4(coef + C + c + j);
        *(f32x4*)(d + j) = ld4(coef + 2 * C + c + j);
        *(f32x4*)(m + j) = ld4(mu + c + j);
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const float gg = (relu && !(yy[j] > 0.f)) ? 0.f : g[j];
        g[j] = a[j] * gg + b[j] * (xv[j] - m[j]) + d[j];
    }
    *(typename V16<T>::raw*)(dx + idx) = pk<T>(g);
}
// ---- frozen statistics (evaluation mode, torchvision's FrozenBatchNorm2d): y = x a + b with a = rstd gamma FIXED, so
// dx = a g and no term depends on a sum over the batch.  MASK is the mask kind of the C ABI (0 none, 1 the ReLU output,
// 2 rebuilt as x a + b > 0 by bn_affine, as the forward decided it, 3 the forward's bit map).
// four of the caller's per-channel floats: one 16-byte load where the pointer allows it (a caller may pass a slice)
template <bool AL>
DEVI f32x4 bn_ld_channels(const float* p) {
    if constexpr (AL) return ld4(p);
    return f32x4{p[0], p[1], p[2], p[3]};
}
// without parameter gradients: a flat map, one 16-byte vector per thread.  dy (+ the ReLU output | 1/16 of a bit map
// | x) -> dx (+ dres = the masked dy)
template <typename T, int MASK, bool AL>
__global__ void bn_bwd_frozen_kernel(const T* __restrict__ dy, const void* __restrict__ mask,
                                     const T* __restrict__ x, const float* __restrict__ gamma,
                                     const float* __restrict__ beta, const float* __restrict__ mean,
                                     const float* __restrict__ rstd, T* __restrict__ dx, T* __restrict__ dres,
                                     int C, long long total) {
    constexpr int V = V16<T>::N;
    typedef typename V16<T>::raw raw_t;
    const long long idx = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * V;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    const raw_t gv = *(const raw_t*)(dy + idx);
    float g[V], a[V];
    [[maybe_unused]] float t[V];  // what the sign is taken of: the ReLU output, or x and then the pre-activation
    [[maybe_unused]] unsigned mk = 0;
    if constexpr (MASK == SSL4GIE_BN_MASK_Y) un<T>(*(const raw_t*)((const T*)mask + idx), t);
    if constexpr (MASK == SSL4GIE_BN_MASK_X) un<T>(*(const raw_t*)(x + idx), t);
    if constexpr (MASK == SSL4GIE_BN_MASK_BITS) mk = ((const unsigned char*)mask)[idx >> 3];  // V == 8: one byte
    un<T>(gv, g);
#pragma unroll
    for (int j = 0; j < V; j += 4) {
        const f32x4 one = {1.f, 1.f, 1.f, 1.f}, zero = {0.f, 0.f, 0.f, 0.f};
        const f32x4 r = bn_ld_channels<AL>(rstd + c + j), gm = gamma ? bn_ld_channels<AL>(gamma + c + j) : one;
        if constexpr (MASK == SSL4GIE_BN_MASK_X) {
            const f32x4 mu = bn_ld_channels<AL>(mean + c + j), be = beta ? bn_ld_channels<AL>(beta + c + j) : zero;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float mb;
                bn_affine(gm[i], be[i], mu[i], r[i], a[j + i], mb);
                t[j + i] = t[j + i] * a[j + i] + mb;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) a[j + i] = r[i] * gm[i];
        }
    }
    if constexpr (MASK != SSL4GIE_BN_MASK_NONE) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const bool keep = MASK == SSL4GIE_BN_MASK_BITS ? ((mk >> j) & 1u) != 0 : t[j] > 0.f;
            g[j] = keep ? g[j] : 0.f;
        }
    }
    if (dres) *(raw_t*)(dres + idx) = MASK == SSL4GIE_BN_MASK_NONE ? gv : pk<T>(g);
#pragma unroll
    for (int j = 0; j < V; ++j) g[j] *= a[j];
    *(raw_t*)(dx + idx) = pk<T>(g);
}
// with parameter gradients: lane mapping, rows in flight and partials of bn_bwd_reduce_kernel (partial[blk][0][c] =
// sum g, [1][c] = sum g xhat; x NULL: only sum g is wanted and [1] is zero), and dx = a g (+ dres) written in the
// same pass — bn_bwd_tail_kernel finishes dgamma / dbeta
template <typename T, int MASK>
__global__ __launch_bounds__(256) void bn_bwd_frozen_reduce_kernel(
    const T* __restrict__ dy, const void* __restrict__ mask, const T* __restrict__ x,
    const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ mean,
    const float* __restrict__ rstd, T* __restrict__ dx, T* __restrict__ dres, float* __restrict__ partial,
    long long rows, int C) {
    constexpr int V = V16<T>::N;
    typedef typename V16<T>::raw raw_t;
    __shared__ float red[3][2][64][V];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const BnLanes m = bn_lanes<V>(C, lane);
    float s[V], q[V];
#pragma unroll
    for (int j = 0; j < V; ++j) s[j] = q[j] = 0.f;
    if (m.c < C) {
        const bool hx = x != nullptr;
        float mu[V], rs[V], a[V];
        [[maybe_unused]] float mb[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            mu[j] = mean ? mean[m.c + j] : 0.f;
            rs[j] = rstd[m.c + j];
            float b;
            bn_affine(gamma ? gamma[m.c + j] : 1.f, beta ? beta[m.c + j] : 0.f, mu[j], rs[j], a[j], b);
            if constexpr (MASK == SSL4GIE_BN_MASK_X) mb[j] = b;
        }
        const T* y = (const T*)mask;
        [[maybe_unused]] const unsigned char* bits = (const unsigned char*)mask;
        // tv: the ReLU output (MASK_Y) or, in its first word, this vector's byte of the bit map (MASK_BITS)
        auto acc = [&](const raw_t& gv, const raw_t& tv, const raw_t& xv, size_t o) {
            float g[V], xx[V];
            un<T>(gv, g);
            un<T>(xv, xx);
            if constexpr (MASK == SSL4GIE_BN_MASK_X) {
#pragma unroll
                for (int j = 0; j < V; ++j) g[j] = xx[j] * a[j] + mb[j] > 0.f ? g[j] : 0.f;
            } else if constexpr (MASK == SSL4GIE_BN_MASK_BITS) {
                const unsigned mk = (unsigned)tv[0];
#pragma unroll
                for (int j = 0; j < V; ++j) g[j] = ((mk >> j) & 1u) ? g[j] : 0.f;
            } else if constexpr (MASK == SSL4GIE_BN_MASK_Y) {
                float yy[V];
                un<T>(tv, yy);
#pragma unroll
                for (int j = 0; j < V; ++j) g[j] = yy[j] > 0.f ? g[j] : 0.f;
            }
            if (dres) *(raw_t*)(dres + o) = MASK == SSL4GIE_BN_MASK_NONE ? gv : pk<T>(g);
            float d[V];
#pragma unroll
            for (int j = 0; j < V; ++j) {
                s[j] += g[j];
                if (hx) q[j] += g[j] * ((xx[j] - mu[j]) * rs[j]);
                d[j] = g[j] * a[j];
            }
            *(raw_t*)(dx + o) = pk<T>(d);
        };
        auto side = [&](const raw_t& gv, size_t o) -> raw_t {
            raw_t r = gv;
            if constexpr (MASK == SSL4GIE_BN_MASK_BITS && V == 8) { r = raw_t{}; r[0] = bits[o >> 3]; }
            if constexpr (MASK == SSL4GIE_BN_MASK_Y) r = *(const raw_t*)(y + o);
            return r;
        };
        const long long step = (long long)gridDim.y * 4 * m.rpw;
        long long r = ((long long)blockIdx.y * 4 + wave) * m.rpw + m.rsub;
        constexpr int NR = MASK == SSL4GIE_BN_MASK_Y ? 2 : 4;  // rows in flight per lane: up to ~8 16-B loads outstanding
        for (; r + (NR - 1) * step < rows; r += NR * step) {
            size_t o[NR];
            raw_t gv[NR], xv[NR], tv[NR];
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                o[i] = (size_t)(r + i * step) * C + m.c;
                gv[i] = *(const raw_t*)(dy + o[i]);
                xv[i] = hx ? *(const raw_t*)(x + o[i]) : gv[i];
                tv[i] = side(gv[i], o[i]);
            }
#pragma unroll
            for (int i = 0; i < NR; ++i) acc(gv[i], tv[i], xv[i], o[i]);
        }
        for (; r < rows; r += step) {
            const size_t o0 = (size_t)r * C + m.c;
            const raw_t g0 = *(const raw_t*)(dy + o0);
            acc(g0, side(g0, o0), hx ? *(const raw_t*)(x + o0) : g0, o0);
        }
    }
    bn_block_reduce<V>(s, q, red, m.lpr, lane, wave);
    if (wave == 0 && m.c < C && m.rsub == 0) {
        float* p = partial + (size_t)blockIdx.y * 2 * C;
#pragma unroll
        for (int j = 0; j < V; j += 4) {
            st4(p + m.c + j, f32x4{s[j], s[j + 1], s[j + 2], s[j + 3]});
            st4(p + C + m.c + j, f32x4{q[j], q[j + 1], q[j + 2], q[j + 3]});
        }
    }
}

// ------------------------------------------------------------------ MaxPool2d(3, 2, 1)
// arg = window position (dy*3+dx) of the first maximum in row-major scan order (ATen's choice); ATen's selection is
// `v > best || isnan(v)`: a NaN anywhere in the window becomes the output, the arg points at it and the backward
// routes the gradient to it
template <typename T>
__global__ void maxpool_fwd_kernel(const T* __restrict__ x, T* __restrict__ y,
                                   unsigned char* __restrict__ arg, int H, int W, int C, int Ho,
                                   int Wo, long long total) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    const long long p = idx / C;
    const int ox = (int)(p % Wo), oy = (int)((p / Wo) % Ho);
    const long long b = p / ((long long)Wo * Ho);
    float best = -INFINITY;
    int bi = 0;
    bool found = false;
    for (int dy = 0; dy < 3; ++dy) {
        const int iy = 2 * oy + dy - 1;
        if (iy < 0 || iy >= H) continue;
        for (int dx = 0; dx < 3; ++dx) {
            const int ix = 2 * ox + dx - 1;
            if (ix < 0 || ix >= W) continue;
            const float v = Elem<T>::ld(x + ((b * H + iy) * W + ix) * C + c);
            if (!found || v > best || v != v) {  // first maximum in scan order; a NaN wins from anywhere (ATen)
                best = v;
                bi = dy * 3 + dx;
                found = true;
            }
        }
    }
    Elem<T>::st(y + idx, best);
    arg[idx] = (unsigned char)bi;
}
template <typename T>
__global__ void maxpool_bwd_kernel(const T* __restrict__ dy, const unsigned char* __restrict__ arg,
                                   T* __restrict__ dx, int H, int W, int C, int Ho, int Wo,
                                   long long total) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    const long long p = idx / C;
    const int x = (int)(p % W), y = (int)((p / W) % H);
    const long long b = p / ((long long)W * H);
    float acc = 0.f;
    for (int dy_ = 0; dy_ < 3; ++dy_) {
        const int ny = y + 1 - dy_;
        if (ny < 0 || (ny & 1)) continue;
        const int oy = ny >> 1;
        if (oy >= Ho) continue;
        for (int dx_ = 0; dx_ < 3; ++dx_) {
            const int nx = x + 1 - dx_;
            if (nx < 0 || (nx & 1)) continue;
            const int ox = nx >> 1;
            if (ox >= Wo) continue;
            const size_t o = (((size_t)b * Ho + oy) * Wo + ox) * C + c;
            if (arg[o] == dy_ * 3 + dx_) acc += Elem<T>::ld(dy + o);
        }
    }
    Elem<T>::st(dx + idx, acc);
}

// the same with a thread owning V = 16 B / sizeof(T) channels of a pixel (C % V == 0): 16-byte
// loads / stores, V argmax bytes per store
// coef (optional, [2][C]): the window runs over act(x coef[0][c] + coef[1][c]) rounded to T — the training-mode
// BatchNorm (+ ReLU) between the stem convolution and the pool, applied on the way in: its output map is never
// written or re-read (values and argmax equal the two-kernel form bit for bit: same arithmetic, same rounding
// before the comparisons, so the many ties at 0 behind the ReLU resolve the same way)
template <typename T>
__global__ void maxpool_fwd_vec_kernel(const T* __restrict__ x, T* __restrict__ y,
                                       unsigned char* __restrict__ arg, int H, int W, int C, int Ho,
                                       int Wo, long long total, const float* __restrict__ coef, int relu) {
    constexpr int V = V16<T>::N;
    typedef typename V16<T>::raw raw_t;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const MapIdx mi = map_index(idx, total, C / V, Wo, Ho);
    const int c = mi.cv * V, ox = mi.x, oy = mi.y;
    const long long p = mi.p, b = mi.b;
    float best[V];
    unsigned char bi[V];
#pragma unroll
    for (int j = 0; j < V; ++j) { best[j] = -INFINITY; bi[j] = 0; }
    float ca[V], cb[V];
    if (coef) {
#pragma unroll
        for (int j = 0; j < V; j += 4) {
            *(f32x4*)(ca + j) = ld4(coef + c + j);
            *(f32x4*)(cb + j) = ld4(coef + C + c + j);
        }
    }
    bool found = false;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        const int iy = 2 * oy + dy - 1;
        if (iy < 0 || iy >= H) continue;
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int ix = 2 * ox + dx - 1;
            if (ix < 0 || ix >= W) continue;
            float v[V];
            un<T>(*(const raw_t*)(x + ((b * H + iy) * W + ix) * C + c), v);
            if (coef) {  // as bn_apply_kernel, then through T's rounding
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const float u = v[j] * ca[j] + cb[j];
                    v[j] = (relu && u < 0.f) ? 0.f : u;
                }
                un<T>(pk<T>(v), v);
            }
#pragma unroll
            for (int j = 0; j < V; ++j) {
                if (!found || v[j] > best[j] || v[j] != v[j]) {  // first maximum in scan order; a NaN wins (ATen)
                    best[j] = v[j];
                    bi[j] = (unsigned char)(dy * 3 + dx);
                }
            }
            found = true;
        }
    }
    *(raw_t*)(y + (size_t)p * C + c) = pk<T>(best);
#pragma unroll
    for (int j = 0; j < V; j += 4)
        *(unsigned*)(arg + (size_t)p * C + c + j) =
            bi[j] | (bi[j + 1] << 8) | (bi[j + 2] << 16) | ((unsigned)bi[j + 3] << 24);
}
template <typename T>
__global__ void maxpool_bwd_vec_kernel(const T* __restrict__ dy, const unsigned char* __restrict__ arg,
                                       T* __restrict__ dx, int H, int W, int C, int Ho, int Wo,
                                       long long total) {
    constexpr int V = V16<T>::N;
    typedef typename V16<T>::raw raw_t;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const MapIdx mi = map_index(idx, total, C / V, W, H);
    const int c = mi.cv * V, x = mi.x, y = mi.y;
    const long long p = mi.p, b = mi.b;
    float acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.f;
#pragma unroll
    for (int dy_ = 0; dy_ < 3; ++dy_) {
        const int ny = y + 1 - dy_;
        if (ny < 0 || (ny & 1)) continue;
        const int oy = ny >> 1;
        if (oy >= Ho) continue;
#pragma unroll
        for (int dx_ = 0; dx_ < 3; ++dx_) {
            const int nx = x + 1 - dx_;
            if (nx < 0 || (nx & 1)) continue;
            const int ox = nx >> 1;
            if (ox >= Wo) continue;
            const size_t o = (((size_t)b * Ho + oy) * Wo + ox) * C + c;
            float g[V];
            un<T>(*(const raw_t*)(dy + o), g);
#pragma unroll
            for (int j = 0; j < V; j += 4) {
                const unsigned a = *(const unsigned*)(arg + o + j);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (((a >> (8 * k)) & 0xff) == (unsigned)(dy_ * 3 + dx_)) acc[j + k] += g[j + k];
            }
        }
    }
    *(raw_t*)(dx + (size_t)p * C + c) = pk<T>(acc);
}

// ------------------------------------------------------------------ global average pool
// y[b, c] = mean over the HW rows of image b (fp32 out); one block per (image, 256-channel strip)
template <typename T>
__global__ void avgpool_fwd_kernel(const T* __restrict__ x, float* __restrict__ y, int HW, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (c >= C) return;
    float s = 0.f;
    for (int r = 0; r < HW; ++r) s += Elem<T>::ld(x + ((size_t)b * HW + r) * C + c);
    y[(size_t)b * C + c] = s / (float)HW;
}
template <typename T>
__global__ void avgpool_bwd_kernel(const float* __restrict__ dy, T* __restrict__ dx, int HW, int C,
                                   long long total) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    const long long b = idx / ((long long)HW * C);
    Elem<T>::st(dx + idx, dy[b * C + c] / (float)HW);
}

// =====================================================================================
// C ABI
// =====================================================================================
// grid of the two BatchNorm reductions: strips of 64 lanes x V channels over C (y: row partitions).
// ~64K elements per workgroup, at most 1024 partitions (the partials are parts x 2C floats)
static int bn_strips(int C, int dtype) {
    const int v = vecn(dtype);
    return (C / v + 63) / 64;
}
static int bn_parts(long long rows, int C) {
    long long p = ((rows * C) >> 16) / ((C + 511) / 512);
    return (int)(p < 1 ? 1 : (p > 1024 ? 1024 : p));
}

extern "C" int ssl4gie_stem_im2col7x7(const float* img, void* cols, int dtype, int B, int H, int W,
                                      long long ld, void* stream) {
    REQUIRE(img && cols && dt_ok(dtype) && B > 0 && H > 0 && W > 0 && ld >= 147 && ld % 8 == 0);
    hipStream_t st = (hipStream_t)stream;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const long long total = (long long)B * Ho * Wo * (ld / 8);
    MAP_LAUNCH(dtype, stem_im2col_kernel, blocks_of(total), 256, img, (T*)cols, B, H, W, Ho, Wo, ld, total);
    return 0;
}
extern "C" int ssl4gie_subsample2(const void* x, void* y, int dtype, int B, int H, int W, int C,
                                  int backward, void* stream) {
    REQUIRE(x && y && dt_ok(dtype) && B > 0 && H > 0 && W > 0 && C > 0 && C % vecn(dtype) == 0);
    hipStream_t st = (hipStream_t)stream;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    if (!backward) {
        const long long total = (long long)B * Ho * Wo * (C / vecn(dtype));
        MAP_LAUNCH(dtype, subsample2_kernel, blocks_of(total), 256, (const T*)x, (T*)y, H, W, C, Ho, Wo, total);
    } else {  // x = dy [B, Ho, Wo, C], y = dx [B, H, W, C]
        const long long total = (long long)B * H * W * (C / vecn(dtype));
        MAP_LAUNCH(dtype, subsample2_bwd_kernel, blocks_of(total), 256, (const T*)x, (T*)y, H, W, C, Ho, Wo, total);
    }
    return 0;
}
// ---- statistics that arrive as per-128-row partials from the producing GEMM's epilogue
// (ssl4gie_gemm_desc::colstats: [parts][2][C], sums about 0): many partials (12 544 for the stem
// map of a 512-image batch) are first folded to 64 by a wide grid, then finished by the tail kernel
#define BN_FOLD 64
__global__ __launch_bounds__(256) void bn_fold_partials_kernel(const float* __restrict__ pin, int parts,
                                                               float* __restrict__ pout, int C) {
    __shared__ float red[3][2][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane, k = blockIdx.y;
    float s = 0.f, q = 0.f;
    if (c < C) {
        int p = k + BN_FOLD * wave;  // eight rows' loads in flight, adds in row order (as bn_sum_partials)
        for (; p + 7 * BN_FOLD * 4 < parts; p += 8 * BN_FOLD * 4) {
            float a[8], b[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                a[u] = pin[(size_t)(p + u * BN_FOLD * 4) * 2 * C + c];
                b[u] = pin[(size_t)(p + u * BN_FOLD * 4) * 2 * C + C + c];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) { s += a[u]; q += b[u]; }
        }
        for (; p < parts; p += BN_FOLD * 4) {
            s += pin[(size_t)p * 2 * C + c];
            q += pin[(size_t)p * 2 * C + C + c];
        }
    }
    if (wave > 0) { red[wave - 1][0][lane] = s; red[wave - 1][1][lane] = q; }
    __syncthreads();
    if (wave == 0 && c < C) {
#pragma unroll
        for (int w = 0; w < 3; ++w) { s += red[w][0][lane]; q += red[w][1][lane]; }
        pout[(size_t)k * 2 * C + c] = s;
        pout[(size_t)k * 2 * C + C + c] = q;
    }
}
// -> (partials to hand to the tail kernels, their count); `scratch` holds BN_FOLD x 2C floats
#define BN_TAIL_WIDE 2048
// threads of the tail kernel for `np` partial rows (see bn_sum_partials)
static dim3 bn_tail_block(int np) { return dim3(np > 4 * BN_FOLD ? 1024 : 256); }
static int bn_fold(const float* partial, int parts, float* scratch, int C, hipStream_t st,
                   const float** out, int* nout) {
    if (parts <= BN_TAIL_WIDE) { *out = partial; *nout = parts; return 0; }
    hipLaunchKernelGGL(bn_fold_partials_kernel, dim3((C + 63) / 64, BN_FOLD), dim3(256), 0, st, partial,
                       parts, scratch, C);
    LAUNCH_CHECK();
    *out = scratch; *nout = BN_FOLD;
    return 0;
}
extern "C" int ssl4gie_maxpool3x3s2_fwd(const void* x, void* y, unsigned char* arg, int dtype, int B,
                                        int H, int W, int C, void* stream) {
    REQUIRE(x && y && arg && dt_ok(dtype) && B > 0 && H > 0 && W > 0 && C > 0);
    hipStream_t st = (hipStream_t)stream;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    if (C % vecn(dtype) == 0) {
        const long long total = (long long)B * Ho * Wo * (C / vecn(dtype));
        MAP_LAUNCH(dtype, maxpool_fwd_vec_kernel, blocks_of(total), 256, (const T*)x, (T*)y, arg, H, W, C, Ho, Wo,
                   total, (const float*)nullptr, 0);
        return 0;
    }
    const long long total = (long long)B * Ho * Wo * C;
    MAP_LAUNCH(dtype, maxpool_fwd_kernel, blocks_of(total), 256, (const T*)x, (T*)y, arg, H, W, C, Ho, Wo, total);
    return 0;
}
// MaxPool2d(3, 2, 1) over act(x coef[0][c] + coef[1][c]) (coef [2][C] from the coefficients-only ssl4gie_bn_fwd): BatchNorm
// + ReLU + pool of the ResNet stem in one pass over the convolution's output
extern "C" int ssl4gie_bn_maxpool3x3s2_fwd(const void* x, const float* coef, int relu, void* y,
                                           unsigned char* arg, int dtype, int B, int H, int W, int C,
                                           void* stream) {
    REQUIRE(x && coef && y && arg && dt_ok(dtype) && B > 0 && H > 0 && W > 0 && C > 0 && C % vecn(dtype) == 0);
    hipStream_t st = (hipStream_t)stream;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const long long total = (long long)B * Ho * Wo * (C / vecn(dtype));
    MAP_LAUNCH(dtype, maxpool_fwd_vec_kernel, blocks_of(total), 256, (const T*)x, (T*)y, arg, H, W, C, Ho, Wo, total,
               coef, relu);
    return 0;
}
extern "C" int ssl4gie_maxpool3x3s2_bwd(const void* dy, const unsigned char* arg, void* dx, int dtype,
                                        int B, int H, int W, int C, void* stream) {
    REQUIRE(dy && dx && arg && dt_ok(dtype) && B > 0 && H > 0 && W > 0 && C > 0);
    hipStream_t st = (hipStream_t)stream;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    if (C % vecn(dtype) == 0) {
        const long long total = (long long)B * H * W * (C / vecn(dtype));
        MAP_LAUNCH(dtype, maxpool_bwd_vec_kernel, blocks_of(total), 256, (const T*)dy, arg, (T*)dx, H, W, C, Ho, Wo,
                   total);
        return 0;
    }
    const long long total = (long long)B * H * W * C;
    MAP_LAUNCH(dtype, maxpool_bwd_kernel, blocks_of(total), 256, (const T*)dy, arg, (T*)dx, H, W, C, Ho, Wo, total);
    return 0;
}
extern "C" int ssl4gie_avgpool_fwd(const void* x, float* y, int dtype, int B, int HW, int C,
                                   void* stream) {
    REQUIRE(x && y && dt_ok(dtype) && B > 0 && HW > 0 && C > 0);
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((C + 255) / 256, B), block(256);
    MAP_LAUNCH(dtype, avgpool_fwd_kernel, grid, block, (const T*)x, y, HW, C);
    return 0;
}
extern "C" int ssl4gie_avgpool_bwd(const float* dy, void* dx, int dtype, int B, int HW, int C,
                                   void* stream) {
    REQUIRE(dy && dx && dt_ok(dtype) && B > 0 && HW > 0 && C > 0);
    hipStream_t st = (hipStream_t)stream;
    const long long total = (long long)B * HW * C;
    MAP_LAUNCH(dtype, avgpool_bwd_kernel, blocks_of(total), 256, dy, (T*)dx, HW, C, total);
    return 0;
}

// ------------------------------------------------------------------ pieces for SyncBatchNorm / MoCo
// dst = dst * m + src * (1 - m): MoCo._update_momentum_encoder (moco/builder.py:57-61) over a whole
// arena slice (base and momentum encoders are laid out identically)
__global__ void ema_update_kernel(float* __restrict__ dst, const float* __restrict__ src, float m,
                                  long long n) {
    const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i + 3 < n) {
        const f32x4 d = ld4(dst + i), v = ld4(src + i);
        st4(dst + i, d * m + v * (1.f - m));
    } else {
        for (long long j = i; j < n; ++j) dst[j] = dst[j] * m + src[j] * (1.f - m);
    }
}
extern "C" int ssl4gie_ema_update(float* dst, const float* src, float m, long long n, void* stream) {
    REQUIRE(dst && src && n >= 0);
    if (n == 0) return 0;
    hipLaunchKernelGGL(ema_update_kernel, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0,
                       (hipStream_t)stream, dst, src, m, n);
    LAUNCH_CHECK();
    return 0;
}
// sums [2][C] (about `pivot`, or about 0 without one) -> mean, biased var: the end of ssl4gie_bn_stats
__global__ void bn_local_stats_kernel(const float* __restrict__ sums, const float* __restrict__ pivot,
                                      float* __restrict__ mean, float* __restrict__ var, float count,
                                      int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float d = sums[c] / count;
    const float v = sums[C + c] / count - d * d;
    mean[c] = (pivot ? pivot[c] : 0.f) + d;
    var[c] = v > 0.f ? v : 0.f;
}
// ---- BatchNorm entry points (ABI 12; the product they span is described in include/ssl4gie_hip.h) -----------------
// The workspace, in floats: [coef 3C][partials parts x 2C][sums 2C][pivot C].  Caller-supplied partials are folded
// into the partials region (BN_FOLD x 2C), the backward keeps the forward's mask coefficients in `sums` and its
// aligned copy of mean in `pivot` (both free there), and the apply half, which has no partials, is the layout with
// parts = 0.
struct BnWs {
    float *coef, *partial, *sums, *pivot;
    BnWs(float* w, size_t parts, int C)
        : coef(w), partial(w + 3 * (size_t)C), sums(partial + parts * 2 * C), pivot(sums + 2 * (size_t)C) {}
    static size_t floats(size_t parts, int C) { return ((parts + 1) * 2 + 1 + 3 + 2 * BN_FOLD) * C; }
};
extern "C" size_t ssl4gie_bn_workspace_bytes(long long rows, int C) {
    size_t parts = (size_t)bn_parts(rows, C);
    if (parts < BN_FOLD) parts = BN_FOLD;  // the partials paths fold into BN_FOLD x 2C floats of this workspace
    return BnWs::floats(parts, C) * sizeof(float);
}

// ---- argument validation: a combination no kernel serves is SSL4GIE_EARG
static bool bn_map_ok(int dtype, long long rows, int C) { return dt_ok(dtype) && rows > 0 && C > 0 && C % 8 == 0; }
static bool bn_fwd_ok(int source, const void* x, const float* partial, int parts, const float* gamma,
                      const float* beta, const void* res, const void* y, const unsigned char* relu_bits,
                      const float* coef, const float* mean, const float* rstd, const float* running_mean,
                      const float* running_var, int relu, const float* workspace, int dtype, long long rows, int C) {
    if (source < SSL4GIE_BN_FROM_X || source > SSL4GIE_BN_FROM_COEF) return false;
    if ((source == SSL4GIE_BN_FROM_PARTIALS) != (partial != nullptr) || (partial && parts <= 0)) return false;
    if (source == SSL4GIE_BN_FROM_STATS && (running_mean || running_var)) return false;  // nothing to update
    if (source == SSL4GIE_BN_FROM_STATS && !y)  // coefficients of given statistics: no map, no workspace
        return mean && rstd && coef && C > 0 && !x && !res && !relu_bits && !workspace;
    if (rows <= 0 || C <= 0 || C % 8 != 0) return false;
    if (source == SSL4GIE_BN_FROM_COEF)  // given coefficients: the apply pass with the bit map (bf16)
        return x && coef && y && relu_bits && relu && dtype == SSL4GIE_BF16 && !gamma && !beta && !mean && !rstd &&
               !running_mean && !running_var && !workspace;
    if (!mean || !rstd || !workspace) return false;
    if (!y)  // coefficients only, into the caller's [2][C]: from partials (a statistics pass over x always writes y)
        return source == SSL4GIE_BN_FROM_PARTIALS && coef && !x && !res && !relu_bits;
    if (!x || coef || !dt_ok(dtype)) return false;
    return !relu_bits || (source == SSL4GIE_BN_FROM_PARTIALS && relu && dtype == SSL4GIE_BF16);
}
// what the three backward functions share; `dres` is NULL in the apply half
static bool bn_bwd_ok(const void* dy, int mask_kind, const void* mask, const void* x, const float* beta,
                      const float* mean, const float* rstd, const void* dres, const float* workspace, int dtype,
                      long long rows, int C) {
    if (!(dy && x && mean && rstd && workspace && bn_map_ok(dtype, rows, C))) return false;
    switch (mask_kind) {
    case SSL4GIE_BN_MASK_NONE: return !mask && !beta;
    case SSL4GIE_BN_MASK_Y: return mask && !beta;
    case SSL4GIE_BN_MASK_X: return !mask && !dres;  // BatchNorm + ReLU without a residual input
    case SSL4GIE_BN_MASK_BITS: return mask && !beta && dres && dtype == SSL4GIE_BF16;  // dres = the masked gradient
    }
    return false;
}

// ---- launches
static int bn_launch_stats(const void* x, const BnWs& ws, int parts, int dtype, long long rows, int C,
                           hipStream_t st) {
    dim3 grid(bn_strips(C, dtype), parts), block(256);
    MAP_LAUNCH(dtype, bn_stats_kernel, grid, block, (const T*)x, ws.partial, ws.pivot, rows, C);
    return 0;
}
static int bn_launch_apply(const void* x, const float* coef, const void* res, void* y, int relu,
                           unsigned char* relu_bits, int dtype, long long rows, int C, hipStream_t st) {
    const long long total = rows * C;
    MAP_LAUNCH(dtype, bn_apply_kernel, blocks_of(total / vecn(dtype)), 256, (const T*)x, coef, (const T*)res, (T*)y,
               relu, C, total, relu_bits);
    return 0;
}
template <typename T>
static int bn_launch_reduce_t(const void* dy, int mask_kind, const void* mask, const void* x, const float* gamma,
                              const float* beta, const float* mean, const float* rstd, void* dres, float* partial,
                              dim3 grid, long long rows, int C, hipStream_t st) {
    const int relu = mask_kind != SSL4GIE_BN_MASK_NONE;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, (const T*)dy, (const T*)mask, (const T*)x, mean, rstd,
                           (T*)dres, partial, relu, rows, C, gamma, beta);
    };
    if (mask_kind == SSL4GIE_BN_MASK_X) {
        launch(bn_bwd_reduce_kernel<T, 1>);
    } else if (mask_kind == SSL4GIE_BN_MASK_BITS) {
        if constexpr (sizeof(T) == 2) launch(bn_bwd_reduce_kernel<T, 2>);  // bf16 only (bn_bwd_ok)
    } else {
        launch(bn_bwd_reduce_kernel<T, 0>);
    }
    LAUNCH_CHECK();
    return 0;
}
// partial[parts][2][C] = this rank's sums of g and g xhat (and dres = g, if given)
static int bn_launch_reduce(const void* dy, int mask_kind, const void* mask, const void* x, const float* gamma,
                            const float* beta, const float* mean, const float* rstd, void* dres, float* partial,
                            int parts, int dtype, long long rows, int C, hipStream_t st) {
    dim3 grid(bn_strips(C, dtype), parts);
    return dtype == SSL4GIE_BF16
               ? bn_launch_reduce_t<bf16_t>(dy, mask_kind, mask, x, gamma, beta, mean, rstd, dres, partial, grid, rows, C, st)
               : bn_launch_reduce_t<float>(dy, mask_kind, mask, x, gamma, beta, mean, rstd, dres, partial, grid, rows, C, st);
}
static int bn_launch_bwd_apply(const void* g, const void* y, const void* x, const float* coef, void* dx, int relu,
                               const float* mcoef, const float* mu, int dtype, long long rows, int C,
                               hipStream_t st) {
    const long long total = rows * C;
    MAP_LAUNCH(dtype, bn_bwd_apply_kernel, blocks_of(total / vecn(dtype)), 256, (const T*)g, (const T*)y, (const T*)x,
               coef, (T*)dx, relu, C, total, mcoef, mu);
    return 0;
}

// ---- forward
// mean / rstd (+ running statistics) and the normalisation coefficients y = x coef[0][c] + coef[1][c] into `coef`
// (the workspace's region for the forms that write y, the caller's [2][C] for the coefficients-only ones).  The
// sums are finished by the tail kernel in its fixed wave order; FROM_STATS runs no reduction at all.
static int bn_fwd_coef(int source, const void* x, const float* partial, int parts, const float* gamma,
                       const float* beta, float* mean, float* rstd, float* running_mean, float* running_var,
                       float momentum, float eps, float* coef, float* workspace, int dtype, long long rows, int C,
                       hipStream_t st) {
    if (source == SSL4GIE_BN_FROM_STATS) {
        hipLaunchKernelGGL(bn_fwd_coef_kernel, dim3((C + 255) / 256), dim3(256), 0, st, mean, rstd, gamma, beta,
                           coef, C);
        LAUNCH_CHECK();
        return 0;
    }
    const float *pp, *pivot = nullptr;
    int np, rc;
    if (source == SSL4GIE_BN_FROM_X) {  // sums about the pivot x[0, c]
        np = bn_parts(rows, C);
        const BnWs ws(workspace, np, C);
        rc = bn_launch_stats(x, ws, np, dtype, rows, C, st);
        pp = ws.partial;
        pivot = ws.pivot;
    } else {  // the producing GEMM's partials (sums about 0): thousands of rows are folded to BN_FOLD first
        rc = bn_fold(partial, parts, BnWs(workspace, BN_FOLD, C).partial, C, st, &pp, &np);
    }
    if (rc) return rc;
    hipLaunchKernelGGL(bn_fwd_tail_kernel, dim3((C + 63) / 64), bn_tail_block(np), 0, st, pp, np, pivot, gamma, beta,
                       mean, rstd, running_mean, running_var, coef, (float)rows, eps, momentum, C);
    LAUNCH_CHECK();
    return 0;
}
extern "C" int ssl4gie_bn_fwd(int source, const void* x, const float* partial, int parts, const float* gamma,
                              const float* beta, const void* res, void* y, unsigned char* relu_bits, float* coef,
                              float* mean, float* rstd, float* running_mean, float* running_var, float momentum,
                              float eps, int relu, float* workspace, int dtype, long long rows, int C,
                              void* stream) {
    REQUIRE(bn_fwd_ok(source, x, partial, parts, gamma, beta, res, y, relu_bits, coef, mean, rstd, running_mean,
                      running_var, relu, workspace, dtype, rows, C));
    hipStream_t st = (hipStream_t)stream;
    if (!y)  // coefficients only
        return bn_fwd_coef(source, x, partial, parts, gamma, beta, mean, rstd, running_mean, running_var, momentum,
                           eps, coef, workspace, dtype, rows, C, st);
    // algorithmic bytes: (statistics pass: x) + apply: x (+ res) -> y
    ProfScope prof(PROF_BN, (double)(rows * C) * (dtype == SSL4GIE_BF16 ? 2 : 4) *
                                ((source == SSL4GIE_BN_FROM_X ? 1 : 0) + 2 + (res ? 1 : 0)), st);
    if (source != SSL4GIE_BN_FROM_COEF) {
        coef = workspace;  // BnWs::coef
        int rc = bn_fwd_coef(source, x, partial, parts, gamma, beta, mean, rstd, running_mean, running_var,
                             momentum, eps, coef, workspace, dtype, rows, C, st);
        if (rc) return rc;
    }
    return bn_launch_apply(x, coef, res, y, relu, relu_bits, dtype, rows, C, st);
}
// the LOCAL (mean, biased var) of SyncBatchNorm's forward.  The sums are finished by
// ssl4gie_internal_reduce_partials, not by the tail kernel: the summation order differs.
extern "C" int ssl4gie_bn_stats(const void* x, const float* partial, int parts, float* mean, float* var,
                                float* workspace, int dtype, long long rows, int C, void* stream) {
    REQUIRE(mean && var && workspace && rows > 0 && C > 0 && C % 8 == 0);
    REQUIRE(partial ? (parts > 0 && !x) : (x && dt_ok(dtype)));
    hipStream_t st = (hipStream_t)stream;
    const int parts_x = partial ? BN_FOLD : bn_parts(rows, C);
    const BnWs ws(workspace, parts_x, C);
    const float *pp = ws.partial, *pivot = partial ? nullptr : ws.pivot;
    int np = parts_x;
    int rc = partial ? bn_fold(partial, parts, ws.partial, C, st, &pp, &np)
                     : bn_launch_stats(x, ws, np, dtype, rows, C, st);
    if (rc) return rc;
    rc = ssl4gie_internal_reduce_partials(pp, ws.sums, np, 2 * C, (size_t)2 * C, 0, st);
    if (rc) return rc;
    hipLaunchKernelGGL(bn_local_stats_kernel, dim3((C + 255) / 256), dim3(256), 0, st, ws.sums, pivot, mean, var,
                       (float)rows, C);
    LAUNCH_CHECK();
    return 0;
}

// ---- backward
// fused: dgamma / dbeta (overwritten or accumulated), dx and (optional) the residual gradient dres
extern "C" int ssl4gie_bn_bwd(const void* dy, int mask_kind, const void* mask, const void* x, const float* gamma,
                              const float* beta, const float* mean, const float* rstd, void* dx, void* dres,
                              float* dgamma, float* dbeta, int accumulate, float* workspace, int dtype,
                              long long rows, int C, void* stream) {
    REQUIRE(dx && bn_bwd_ok(dy, mask_kind, mask, x, beta, mean, rstd, dres, workspace, dtype, rows, C));
    hipStream_t st = (hipStream_t)stream;
    const int parts = bn_parts(rows, C), relu = mask_kind != SSL4GIE_BN_MASK_NONE;
    const bool from_y = mask_kind == SSL4GIE_BN_MASK_Y;
    // with a residual branch the reduction pass writes dres = the MASKED gradient (dy or 0, no rounding): the apply
    // pass reads that one tensor instead of dy and the ReLU output (6 -> 4 B/element read on the widest BatchNorm
    // of a bottleneck)
    const bool masked = relu && dres;
    // algorithmic bytes: reduce reads dy, x (+ the ReLU output when the mask comes from it; the bit map is 1/16 of
    // a tensor) and writes dres; apply reads the gradient, x (+ the ReLU output) and writes dx
    ProfScope prof(PROF_BN, (double)rows * C * (dtype == SSL4GIE_BF16 ? 2 : 4) *
                                ((2 + (from_y ? 1 : 0) + (mask_kind == SSL4GIE_BN_MASK_BITS ? 0.0625 : 0) + (dres ? 1 : 0)) +
                                 (2 + ((from_y && !masked) ? 1 : 0) + 1)), st);
    const BnWs ws(workspace, parts, C);
    float* mcoef = mask_kind == SSL4GIE_BN_MASK_X ? ws.sums : nullptr;  // the forward's y = x a + b, for the apply pass
    int rc = bn_launch_reduce(dy, mask_kind, mask, x, gamma, beta, mean, rstd, dres, ws.partial, parts, dtype, rows,
                              C, st);
    if (rc) return rc;
    // dbeta = sum g, dgamma = sum g xhat, and the dx coefficients, in one launch.  No fold in front: bn_parts caps
    // the partitions at 1024 <= BN_TAIL_WIDE, so the tail always sums the reduction's partials itself
    hipLaunchKernelGGL(bn_bwd_tail_kernel, dim3((C + 63) / 64), bn_tail_block(parts), 0, st, ws.partial, parts, mean,
                       rstd, gamma, 1.0f / (float)rows, ws.coef, dgamma, dbeta, accumulate, C, beta, mcoef, ws.pivot);
    LAUNCH_CHECK();
    return bn_launch_bwd_apply(masked ? dres : dy, masked ? nullptr : mask, x, ws.coef, dx, masked ? 0 : relu, mcoef,
                               ws.pivot, dtype, rows, C, st);
}
// SyncBatchNorm's halves: sums[0][c] = sum g, sums[1][c] = sum g xhat over the LOCAL rows (the caller all-reduces
// them), then dx with the GLOBAL sums and 1 / (global row count)
extern "C" int ssl4gie_bn_bwd_reduce(const void* dy, int mask_kind, const void* mask, const void* x,
                                     const float* gamma, const float* beta, const float* mean, const float* rstd,
                                     void* dres, float* sums, float* workspace, int dtype, long long rows, int C,
                                     void* stream) {
    REQUIRE(sums && bn_bwd_ok(dy, mask_kind, mask, x, beta, mean, rstd, dres, workspace, dtype, rows, C));
    REQUIRE(mask_kind == SSL4GIE_BN_MASK_X || !gamma);  // gamma / beta only rebuild the mask here
    hipStream_t st = (hipStream_t)stream;
    const int parts = bn_parts(rows, C);
    const BnWs ws(workspace, parts, C);
    int rc = bn_launch_reduce(dy, mask_kind, mask, x, gamma, beta, mean, rstd, dres, ws.partial, parts, dtype, rows,
                              C, st);
    if (rc) return rc;
    return ssl4gie_internal_reduce_partials(ws.partial, sums, parts, 2 * C, (size_t)2 * C, 0, st);
}
extern "C" int ssl4gie_bn_bwd_apply(const void* dy, int mask_kind, const void* mask, const void* x,
                                    const float* gamma, const float* beta, const float* mean, const float* rstd,
                                    const float* sums, float inv_count, void* dx, float* workspace, int dtype,
                                    long long rows, int C, void* stream) {
    REQUIRE(sums && dx && mask_kind != SSL4GIE_BN_MASK_BITS &&  // the caller applies on the reduce half's dres, no mask
            bn_bwd_ok(dy, mask_kind, mask, x, beta, mean, rstd, nullptr, workspace, dtype, rows, C));
    hipStream_t st = (hipStream_t)stream;
    const BnWs ws(workspace, 0, C);  // no partials: [dx coefficients 3C][mask coefficients 2C][copy of mean C]
    float* mcoef = mask_kind == SSL4GIE_BN_MASK_X ? ws.sums : nullptr;
    hipLaunchKernelGGL(bn_bwd_coef_kernel, dim3((C + 255) / 256), dim3(256), 0, st, mean, rstd, gamma, sums,
                       inv_count, ws.coef, C, ws.pivot);
    LAUNCH_CHECK();
    if (mcoef) {
        hipLaunchKernelGGL(bn_fwd_coef_kernel, dim3((C + 255) / 256), dim3(256), 0, st, mean, rstd, gamma, beta, mcoef,
                           C);
        LAUNCH_CHECK();
    }
    return bn_launch_bwd_apply(dy, mask, x, ws.coef, dx, mask_kind != SSL4GIE_BN_MASK_NONE, mcoef, ws.pivot, dtype,
                               rows, C, st);
}
// backward through FIXED statistics (evaluation mode, FrozenBatchNorm2d): dx = rstd gamma g, dres = g; with dgamma /
// dbeta one reduction pass that writes dx and dres as well, without them one flat pass that reads x only for MASK_X
template <typename T, int MASK>
static void bn_launch_frozen_t(const void* dy, const void* mask, const void* x, const float* gamma, const float* beta,
                               const float* mean, const float* rstd, void* dx, void* dres, float* partial, int parts,
                               int dtype, long long rows, int C, hipStream_t st) {
    if (partial) {
        hipLaunchKernelGGL((bn_bwd_frozen_reduce_kernel<T, MASK>), dim3(bn_strips(C, dtype), parts), dim3(256), 0, st,
                           (const T*)dy, mask, (const T*)x, gamma, beta, mean, rstd, (T*)dx, (T*)dres, partial, rows,
                           C);
        return;
    }
    const long long total = rows * C;
    const dim3 grid(blocks_of(total / vecn(dtype)));
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, (const T*)dy, mask, (const T*)x, gamma, beta, mean, rstd,
                           (T*)dx, (T*)dres, C, total);
    };
    if (is16(gamma) && is16(beta) && is16(mean) && is16(rstd)) launch(bn_bwd_frozen_kernel<T, MASK, true>);
    else launch(bn_bwd_frozen_kernel<T, MASK, false>);
}
template <typename T>
static void bn_launch_frozen(int mask_kind, const void* dy, const void* mask, const void* x, const float* gamma,
                             const float* beta, const float* mean, const float* rstd, void* dx, void* dres,
                             float* partial, int parts, int dtype, long long rows, int C, hipStream_t st) {
#define FROZEN(MASK) \
    bn_launch_frozen_t<T, MASK>(dy, mask, x, gamma, beta, mean, rstd, dx, dres, partial, parts, dtype, rows, C, st)
    switch (mask_kind) {
    case SSL4GIE_BN_MASK_NONE: FROZEN(SSL4GIE_BN_MASK_NONE); break;
    case SSL4GIE_BN_MASK_Y: FROZEN(SSL4GIE_BN_MASK_Y); break;
    case SSL4GIE_BN_MASK_X: FROZEN(SSL4GIE_BN_MASK_X); break;
    case SSL4GIE_BN_MASK_BITS:
        if constexpr (sizeof(T) == 2) FROZEN(SSL4GIE_BN_MASK_BITS);  // bf16 only (checked by the caller)
        break;
    }
#undef FROZEN
}
extern "C" int ssl4gie_bn_bwd_frozen(const void* dy, int mask_kind, const void* mask, const void* x,
                                     const float* gamma, const float* beta, const float* mean, const float* rstd,
                                     void* dx, void* dres, float* dgamma, float* dbeta, int accumulate,
                                     float* workspace, int dtype, long long rows, int C, void* stream) {
    REQUIRE(dy && rstd && dx && dt_ok(dtype) && rows > 0 && C > 0 && C % vecn(dtype) == 0);
    const bool params = dgamma || dbeta, need_x = mask_kind == SSL4GIE_BN_MASK_X || dgamma;
    // a pointer the form does not use is NULL: x and mean without MASK_X and dgamma, the workspace without a reduction
    REQUIRE(!x == !need_x && !mean == !need_x && !workspace == !params);
    switch (mask_kind) {
    case SSL4GIE_BN_MASK_NONE: REQUIRE(!mask && !beta); break;
    case SSL4GIE_BN_MASK_Y: REQUIRE(mask && !beta); break;
    case SSL4GIE_BN_MASK_X: REQUIRE(!mask && !dres); break;
    case SSL4GIE_BN_MASK_BITS: REQUIRE(mask && !beta && dres && dtype == SSL4GIE_BF16); break;
    default: return ARG_ERR;
    }
    hipStream_t st = (hipStream_t)stream;
    // algorithmic bytes: dy (+ the ReLU output | 1/16 of a map of bits) (+ x) -> dx (+ dres)
    ProfScope prof(PROF_BN, (double)rows * C * (dtype == SSL4GIE_BF16 ? 2 : 4) *
                                (2 + (mask_kind == SSL4GIE_BN_MASK_Y ? 1 : 0) +
                                 (mask_kind == SSL4GIE_BN_MASK_BITS ? 0.0625 : 0) + (x ? 1 : 0) + (dres ? 1 : 0)), st);
    const int parts = bn_parts(rows, C);
    float* partial = params ? BnWs(workspace, parts, C).partial : nullptr;
    if (dtype == SSL4GIE_BF16)
        bn_launch_frozen<bf16_t>(mask_kind, dy, mask, x, gamma, beta, mean, rstd, dx, dres, partial, parts, dtype, rows,
                                 C, st);
    else
        bn_launch_frozen<float>(mask_kind, dy, mask, x, gamma, beta, mean, rstd, dx, dres, partial, parts, dtype, rows,
                                C, st);
    LAUNCH_CHECK();
    if (!params) return 0;
    // dbeta = sum g, dgamma = sum g xhat by the training-mode tail (bn_parts <= 1024 <= BN_TAIL_WIDE: no fold).  Its dx
    // coefficients and copy of mean land in the workspace unread; without x there is no mean to copy and rstd stands in
    const BnWs ws(workspace, parts, C);
    hipLaunchKernelGGL(bn_bwd_tail_kernel, dim3((C + 63) / 64), bn_tail_block(parts), 0, st, ws.partial, parts,
                       mean ? mean : rstd, rstd, gamma, 0.f, ws.coef, dgamma, dbeta, accumulate, C,
                       (const float*)nullptr, (float*)nullptr, ws.pivot);
    LAUNCH_CHECK();
    return 0;
}

// ---- SyncBatchNorm: pooled statistics out of the gathered per-rank records ----------------------------
// gathered [W][2C + 1] = (mean_w[C], biased var_w[C], rows_w) of every rank (ranks may hold different
// row counts): total = sum rows_w, mean = sum rows_w/total mean_w, var = sum rows_w/total (var_w +
// (mean_w - mean)^2); rstd = rsqrt(var + eps); running statistics with the unbiased factor total/(total-1).
// One launch instead of ~10 torch kernels on [W, 2C+1] floats per layer; everything stays on the device.
__global__ void bn_combine_stats_kernel(const float* __restrict__ g, int W, int C, float eps, float momentum,
                                        float* __restrict__ running_mean, float* __restrict__ running_var,
                                        float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                        float* __restrict__ total_out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    const int rec = 2 * C + 1;
    float total = 0.f;
    for (int w = 0; w < W; ++w) total += g[(size_t)w * rec + 2 * C];
    if (c == 0) *total_out = total;
    if (c >= C) return;
    const float inv = 1.f / total;
    float mean = 0.f;
    for (int w = 0; w < W; ++w) mean += g[(size_t)w * rec + c] * (g[(size_t)w * rec + 2 * C] * inv);
    float var = 0.f;
    for (int w = 0; w < W; ++w) {
        const float d = g[(size_t)w * rec + c] - mean;
        var += (g[(size_t)w * rec + C + c] + d * d) * (g[(size_t)w * rec + 2 * C] * inv);
    }
    mean_out[c] = mean;
    rstd_out[c] = rsqrtf(var + eps);
    if (running_mean) {
        const float unb = total / fmaxf(total - 1.f, 1.f);
        running_mean[c] = running_mean[c] * (1.f - momentum) + mean * momentum;
        running_var[c] = running_var[c] * (1.f - momentum) + var * unb * momentum;
    }
}

extern "C" int ssl4gie_bn_combine_stats(const float* gathered, int world, int C, float eps, float momentum,
                                        float* running_mean, float* running_var, float* mean, float* rstd,
                                        float* total, void* stream) {
    REQUIRE(gathered && mean && rstd && total && world >= 1 && C >= 1 && (!running_mean == !running_var));
    hipLaunchKernelGGL(bn_combine_stats_kernel, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, gathered,
                       world, C, eps, momentum, running_mean, running_var, mean, rstd, total);
    LAUNCH_CHECK();
    return 0;
}
