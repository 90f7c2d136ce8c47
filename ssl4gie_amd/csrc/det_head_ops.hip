// The Faster R-CNN heads' box operations on the device: Object_detection/train_detection.py:244-250 wraps the backbone
// in torchvision.models.detection.faster_rcnn.FasterRCNN, whose proposal and detection stages run torchvision's C++ /
// CUDA ops (nms, batched_nms, roi_align) and chains of small box ops around them.  ssl4gie_amd/Models/detection.py
// states the rules (torchvision 0.10's published source); this file has the kernels.
//
//  * nms       segmented greedy NMS without a host round trip.  `pairs`: one wave per 64 x 64 tile of a segment's upper
//              triangle writes a 64-bit suppression word per row (row i, word w: bit b set when box 64 w + b > i has
//              IoU > thr with box i).  `sweep`: one wave per segment; lane l holds the `removed` word l (64 lanes x 64
//              bits = the 4096-box cap), rows are fetched eight at a time ahead of the eight dependent keep decisions.
//              torchvision's CUDA nms copies the mask to the host for this sweep.
//  * decode    BoxCoder.decode_single + clip_boxes_to_image + remove_small_boxes + the score test in one launch, in the
//              RPN form (anchor from (level, flat index), deltas and logit gathered by the top-k index, sigmoid) and
//              the RoI form (explicit proposals, per-class deltas, row softmax, background column dropped).
//  * roi_align MultiScaleRoIAlign(["0".."3"], 7, 2): level per RoI on the device, lanes along channels of the
//              channels-last maps (every tap is one contiguous row of C floats), the [C][49] tile of a RoI staged in
//              LDS so that fc6's (c, ph, pw) row leaves / arrives as one contiguous run.  The backward adds into zeroed
//              fp32 maps with float atomics, one add per (RoI, touched pixel) — the taps of a RoI that share a pixel are
//              merged first — and one wave instruction = 64 consecutive channels = 256 contiguous bytes; the sums depend
//              on arrival order: not bitwise reproducible.
//
// The decisions (IoU against the threshold, sizes against min_size, the level) are fp32 operations rounded one by one,
// as torch rounds them: the Makefile builds this object with -ffp-contract=off (see det_map_ops.hip on why the pragma
// alone does not do it).
#include "common.h"
#include "ssl4gie_hip.h"

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

constexpr int NMS_MAX = SSL4GIE_NMS_MAX_PER_SEGMENT;  // 4096 = 64 lanes x 64 bits
constexpr int RA_P = 7, RA_BINS = RA_P * RA_P, RA_S = 2;  // pooled size, bins, samples per bin side
constexpr int RA_MAXT = 256;                             // channels per workgroup

// ------------------------------------------------------------------ nms
struct NmsSeg { int s0, ns; };
// the segment as the kernels read it: nothing is read through offsets that do not describe it
DEVI NmsSeg nms_seg(const int* __restrict__ seg_off, int seg, long long n, int max_seg) {
    NmsSeg r;
    const int a = seg_off[seg], b = seg_off[seg + 1];
    r.s0 = a;
    r.ns = 0;
    if (a < 0 || b < a || (long long)b > n) return r;
    r.ns = b - a < max_seg ? b - a : max_seg;
    return r;
}

__global__ __launch_bounds__(64) void nms_pairs_kernel(const float* __restrict__ boxes,
                                                       const int* __restrict__ seg_off, long long n, int max_seg,
                                                       int words, float thr, u64* __restrict__ mask) {
    __shared__ float cb[64][4];
    const int colb = blockIdx.x, rowb = blockIdx.y, seg = blockIdx.z, t = threadIdx.x;
    if (colb < rowb) return;
    const NmsSeg s = nms_seg(seg_off, seg, n, max_seg);
    if (rowb * 64 >= s.ns || colb * 64 >= s.ns) return;
    const int cj = colb * 64 + t;
    if (cj < s.ns) {
        const f32x4 b = *(const f32x4*)(boxes + (size_t)(s.s0 + cj) * 4);
        cb[t][0] = b[0]; cb[t][1] = b[1]; cb[t][2] = b[2]; cb[t][3] = b[3];
    }
    __syncthreads();
    const int i = rowb * 64 + t;
    if (i >= s.ns) return;
    const f32x4 a = *(const f32x4*)(boxes + (size_t)(s.s0 + i) * 4);
    const float area_a = (a[2] - a[0]) * (a[3] - a[1]);
    const int ncol = s.ns - colb * 64 < 64 ? s.ns - colb * 64 : 64;
    u64 bits = 0;
    for (int j = 0; j < ncol; ++j) {
        if (colb * 64 + j <= i) continue;
        const float bx1 = cb[j][0], by1 = cb[j][1], bx2 = cb[j][2], by2 = cb[j][3];
        const float area_b = (bx2 - bx1) * (by2 - by1);
        const float w = fmaxf(0.f, fminf(a[2], bx2) - fmaxf(a[0], bx1));
        const float h = fmaxf(0.f, fminf(a[3], by2) - fmaxf(a[1], by1));
        const float inter = w * h;
        const float iou = inter / (area_a + area_b - inter);
        if (iou > thr) bits |= 1ull << j;
    }
    mask[(size_t)(s.s0 + i) * words + colb] = bits;
}

DEVI u64 shfl64(u64 v, int src) {
    const unsigned lo = __shfl((unsigned)v, src, 64), hi = __shfl((unsigned)(v >> 32), src, 64);
    return ((u64)hi << 32) | lo;
}

__global__ __launch_bounds__(64) void nms_sweep_kernel(const u64* __restrict__ mask,
                                                       const unsigned char* __restrict__ valid,
                                                       const int* __restrict__ seg_off, long long n, int max_seg,
                                                       int words, int* __restrict__ keep_rank,
                                                       int* __restrict__ count) {
    const int seg = blockIdx.x, lane = threadIdx.x;
    const NmsSeg s = nms_seg(seg_off, seg, n, max_seg);
    const int nblk = (s.ns + 63) >> 6;
    // a box that is not there, or not valid, is never kept and suppresses nothing: it starts out removed
    u64 removed = ~0ull;
    if (lane < nblk) {
        u64 ok = 0;
        const int left = s.ns - lane * 64, m = left < 64 ? left : 64;
        for (int b = 0; b < m; ++b)
            if (!valid || valid[(size_t)s.s0 + lane * 64 + b]) ok |= 1ull << b;
        removed = ~ok;
    }
    const bool mine = lane < nblk;
    for (int blk = 0; blk < nblk; ++blk) {
        u64 cur = shfl64(removed, blk);  // wave-uniform: the state of this block's 64 boxes
        for (int c = 0; c < 64; c += 8) {
            if (blk * 64 + c >= s.ns) break;
            u64 row[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {  // independent loads, ahead of the decisions that use them
                const int i = blk * 64 + c + k;
                row[k] = (i < s.ns && mine && lane >= blk) ? mask[(size_t)(s.s0 + i) * words + lane] : 0ull;
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (!((cur >> (c + k)) & 1ull)) {  // kept (uniform branch)
                    removed |= row[k];
                    cur |= shfl64(row[k], blk);
                }
            }
        }
    }
    // kept rank = position among the kept boxes of the segment, -1 for a dropped one
    const u64 kept = ~removed;
    const int mycount = __popcll(kept);
    int incl = mycount;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(incl, o, 64);
        if (lane >= o) incl += u;
    }
    int r = incl - mycount;
    if (mine) {
        const int left = s.ns - lane * 64, m = left < 64 ? left : 64;
        for (int b = 0; b < m; ++b) {
            const bool k = (kept >> b) & 1ull;
            keep_rank[(size_t)s.s0 + lane * 64 + b] = k ? r : -1;
            r += k;
        }
    }
    if (lane == 63) count[seg] = incl;
}

// ------------------------------------------------------------------ decode
struct BoxOut { float x1, y1, x2, y2; };
// BoxCoder.decode_single on one box + clip_boxes_to_image, in torchvision's order of operations
DEVI BoxOut decode_clip(float ax1, float ay1, float ax2, float ay2, float dx, float dy, float dw, float dh, float wx,
                        float wy, float ww, float wh, float clip, float W, float H) {
    const float widths = ax2 - ax1, heights = ay2 - ay1;
    const float ctr_x = ax1 + 0.5f * widths, ctr_y = ay1 + 0.5f * heights;
    dx = dx / wx; dy = dy / wy; dw = dw / ww; dh = dh / wh;
    dw = fminf(dw, clip);
    dh = fminf(dh, clip);
    const float pcx = dx * widths + ctr_x, pcy = dy * heights + ctr_y;
    const float pw = expf(dw) * widths, ph = expf(dh) * heights;
    BoxOut o;
    o.x1 = fminf(fmaxf(pcx - 0.5f * pw, 0.f), W);
    o.y1 = fminf(fmaxf(pcy - 0.5f * ph, 0.f), H);
    o.x2 = fminf(fmaxf(pcx + 0.5f * pw, 0.f), W);
    o.y2 = fminf(fmaxf(pcy + 0.5f * ph, 0.f), H);
    return o;
}

struct RpnLevels {
    const float* head[SSL4GIE_RPN_MAX_LEVELS];
    int grid[SSL4GIE_RPN_MAX_LEVELS];
    int koff[SSL4GIE_RPN_MAX_LEVELS + 1];
    float base[SSL4GIE_RPN_MAX_LEVELS * SSL4GIE_RPN_MAX_ANCHORS * 4];
};

__global__ __launch_bounds__(256) void rpn_decode_kernel(const RpnLevels lv, int L, int A, int ld,
                                                         const long long* __restrict__ topk_idx, int B, int F,
                                                         float clip, float min_size, float score_thresh,
                                                         float* __restrict__ boxes, float* __restrict__ scores,
                                                         unsigned char* __restrict__ valid) {
    const int ktot = lv.koff[L];
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)B * ktot) return;
    const int b = (int)(t / ktot), j = (int)(t - (long long)b * ktot);
    int l = 0;
    while (l + 1 < L && j >= lv.koff[l + 1]) ++l;
    const int g = lv.grid[l];
    const long long idx = topk_idx[t];
    BoxOut o = {0.f, 0.f, 0.f, 0.f};
    float sc = 0.f;
    bool ok = false;
    if (idx >= 0 && idx < (long long)A * g * g) {  // never an address otherwise
        const int loc = (int)(idx / A), a = (int)(idx - (long long)loc * A);
        const int y = loc / g, x = loc - y * g;
        const float stride = (float)(F / g);
        const float sx = (float)x * stride, sy = (float)y * stride;
        const float* ba = lv.base + (l * A + a) * 4;
        const float* row = lv.head[l] + ((size_t)b * g * g + loc) * ld;
        const float* d = row + A + a * 4;
        o = decode_clip(sx + ba[0], sy + ba[1], sx + ba[2], sy + ba[3], d[0], d[1], d[2], d[3], 1.f, 1.f, 1.f, 1.f,
                        clip, (float)F, (float)F);
        sc = 1.f / (1.f + expf(-row[a]));
        ok = (o.x2 - o.x1 >= min_size) && (o.y2 - o.y1 >= min_size) && (sc >= score_thresh);
    }
    *(f32x4*)(boxes + (size_t)t * 4) = f32x4{o.x1, o.y1, o.x2, o.y2};
    scores[t] = sc;
    valid[t] = ok ? 1 : 0;
}

__global__ __launch_bounds__(256) void roi_decode_kernel(const float* __restrict__ proposals,
                                                         const float* __restrict__ logits, int ld_logits,
                                                         const float* __restrict__ deltas, int ld_deltas, int K, int C,
                                                         float wx, float wy, float ww, float wh, float clip, float W,
                                                         float H, float min_size, float score_thresh,
                                                         float* __restrict__ boxes, float* __restrict__ scores,
                                                         unsigned char* __restrict__ valid) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)K * (C - 1)) return;
    const int k = (int)(t / (C - 1)), c = 1 + (int)(t - (long long)k * (C - 1));
    const float* lg = logits + (size_t)k * ld_logits;
    float m = lg[0];
    for (int q = 1; q < C; ++q) m = fmaxf(m, lg[q]);
    float sum = 0.f;
    for (int q = 0; q < C; ++q) sum += expf(lg[q] - m);
    const float sc = expf(lg[c] - m) / sum;
    const f32x4 p = *(const f32x4*)(proposals + (size_t)k * 4);
    const float* d = deltas + (size_t)k * ld_deltas + c * 4;
    const BoxOut o = decode_clip(p[0], p[1], p[2], p[3], d[0], d[1], d[2], d[3], wx, wy, ww, wh, clip, W, H);
    *(f32x4*)(boxes + (size_t)t * 4) = f32x4{o.x1, o.y1, o.x2, o.y2};
    scores[t] = sc;
    valid[t] = ((o.x2 - o.x1 >= min_size) && (o.y2 - o.y1 >= min_size) && (sc >= score_thresh)) ? 1 : 0;
}

// ------------------------------------------------------------------ roi_align
struct RaMaps {
    float* map[4];
    int H[4], W[4];
    float scale[4];
};

// LevelMapper(k_min 2, k_max 5, canonical scale 224, canonical level 4, eps 1e-6) -> 0 .. 3
DEVI int roi_level(float x1, float y1, float x2, float y2) {
    const float s = sqrtf((x2 - x1) * (y2 - y1));
    float k = floorf(4.f + log2f(s / 224.f) + 1e-6f);
    k = fminf(fmaxf(k, 2.f), 5.f);  // -inf (zero area) and NaN end on a level too
    return (k >= 2.f && k <= 5.f) ? (int)k - 2 : 0;
}

struct RaTap { int off[4]; float w[4]; };  // offsets in pixels (y * W + x); all weights 0 for a sample outside
DEVI RaTap ra_tap(float y, float x, int H, int W) {
    RaTap t;
    if (y < -1.f || y > (float)H || x < -1.f || x > (float)W) {
        t.off[0] = t.off[1] = t.off[2] = t.off[3] = 0;
        t.w[0] = t.w[1] = t.w[2] = t.w[3] = 0.f;
        return t;
    }
    if (y <= 0.f) y = 0.f;
    if (x <= 0.f) x = 0.f;
    int yl = (int)y, xl = (int)x, yh, xh;
    if (yl >= H - 1) { yh = yl = H - 1; y = (float)yl; } else yh = yl + 1;
    if (xl >= W - 1) { xh = xl = W - 1; x = (float)xl; } else xh = xl + 1;
    const float ly = y - (float)yl, lx = x - (float)xl, hy = 1.f - ly, hx = 1.f - lx;
    t.off[0] = yl * W + xl; t.off[1] = yl * W + xh; t.off[2] = yh * W + xl; t.off[3] = yh * W + xh;
    t.w[0] = hy * hx; t.w[1] = hy * lx; t.w[2] = ly * hx; t.w[3] = ly * lx;
    return t;
}

struct RaGeom { float sh, sw, bh, bw; int lvl, H, W; float* base; bool ok; };
DEVI RaGeom ra_geom(const RaMaps& mp, const float* __restrict__ rois, const int* __restrict__ roi_batch, int k, int B,
                    int C) {
    RaGeom g;
    const f32x4 r = *(const f32x4*)(rois + (size_t)k * 4);
    const int b = roi_batch[k];
    g.lvl = roi_level(r[0], r[1], r[2], r[3]);
    g.ok = b >= 0 && b < B;
    g.H = mp.H[g.lvl]; g.W = mp.W[g.lvl];
    const float sc = mp.scale[g.lvl];
    g.sw = r[0] * sc; g.sh = r[1] * sc;
    const float ew = r[2] * sc, eh = r[3] * sc;
    g.bw = fmaxf(ew - g.sw, 1.f) / (float)RA_P;
    g.bh = fmaxf(eh - g.sh, 1.f) / (float)RA_P;
    g.base = mp.map[g.lvl] + (size_t)(g.ok ? b : 0) * g.H * g.W * C;
    return g;
}

template <typename T>
__global__ __launch_bounds__(RA_MAXT) void roi_align_fwd_kernel(const RaMaps mp, const float* __restrict__ rois,
                                                                const int* __restrict__ roi_batch, int B, int C,
                                                                T* __restrict__ out, int* __restrict__ levels) {
    __shared__ float tile[RA_MAXT * RA_BINS];
    const int k = blockIdx.x, c0 = blockIdx.y * blockDim.x, t = threadIdx.x, c = c0 + t;
    const RaGeom g = ra_geom(mp, rois, roi_batch, k, B, C);
    if (levels && blockIdx.y == 0 && t == 0) levels[k] = g.lvl;
    for (int ph = 0; ph < RA_P; ++ph)
        for (int pw = 0; pw < RA_P; ++pw) {
            float acc = 0.f;
            if (g.ok) {
#pragma unroll
                for (int iy = 0; iy < RA_S; ++iy) {
                    const float y = g.sh + (float)ph * g.bh + ((float)iy + 0.5f) * g.bh / (float)RA_S;
#pragma unroll
                    for (int ix = 0; ix < RA_S; ++ix) {
                        const float x = g.sw + (float)pw * g.bw + ((float)ix + 0.5f) * g.bw / (float)RA_S;
                        const RaTap tp = ra_tap(y, x, g.H, g.W);
                        const float* p = g.base + c;
                        acc += tp.w[0] * p[(size_t)tp.off[0] * C] + tp.w[1] * p[(size_t)tp.off[1] * C] +
                               tp.w[2] * p[(size_t)tp.off[2] * C] + tp.w[3] * p[(size_t)tp.off[3] * C];
                    }
                }
            }
            tile[t * RA_BINS + ph * RA_P + pw] = acc / (float)(RA_S * RA_S);
        }
    __syncthreads();
    // the block's (c, ph, pw) run of the RoI's row is contiguous: out[k][c0 * 49 ...]
    T* o = out + (size_t)k * C * RA_BINS + (size_t)c0 * RA_BINS;
    const int nrun = blockDim.x * RA_BINS;
    for (int i = t; i < nrun; i += blockDim.x) Elem<T>::st(o + i, tile[i]);
}

// The backward of one RoI is separable: the gradient of pixel (r, c) is sum_ph sum_pw Wy[r][ph] Wx[c][pw] dy[ph][pw] / 4,
// Wy[r][ph] = the bilinear weights that the (at most two) valid samples of bin row ph give to map row r.  An axis has at
// most 7 bins x 2 samples x 2 taps = 28 distinct rows; taps that share a row are merged here, so a pixel receives ONE add
// per RoI instead of one per tap (fewer atomics, and less rounding where many RoIs meet on the same rows).
struct RaAxis {
    int n;
    int idx[RA_P * RA_S * 2], lo[RA_P * RA_S * 2], hi[RA_P * RA_S * 2];  // map row, first / last bin that touches it
    float w[RA_P * RA_S * 2][RA_P];
};
DEVI void ra_axis_build(RaAxis& ax, float start, float bin, int N) {
    int n = 0;
    for (int p = 0; p < RA_P; ++p)
        for (int i = 0; i < RA_S; ++i) {
            float v = start + (float)p * bin + ((float)i + 0.5f) * bin / (float)RA_S;  // the forward's expression
            if (v < -1.f || v > (float)N) continue;
            if (v <= 0.f) v = 0.f;
            int l = (int)v, h;
            if (l >= N - 1) { h = l = N - 1; v = (float)l; } else h = l + 1;
            const float fl = v - (float)l, fh = 1.f - fl;
            for (int q = 0; q < 2; ++q) {
                const int r = q ? h : l;
                const float wt = q ? fl : fh;
                int j = 0;
                while (j < n && ax.idx[j] != r) ++j;
                if (j == n) {
                    ax.idx[j] = r;
                    ax.lo[j] = p;
                    for (int z = 0; z < RA_P; ++z) ax.w[j][z] = 0.f;
                    ++n;
                }
                ax.w[j][p] += wt;
                ax.hi[j] = p;
            }
        }
    ax.n = n;
}

template <typename T>
__global__ __launch_bounds__(RA_MAXT) void roi_align_bwd_kernel(const RaMaps mp, const float* __restrict__ rois,
                                                                const int* __restrict__ roi_batch, int B, int C,
                                                                const T* __restrict__ dy) {
    __shared__ float tile[RA_MAXT * RA_BINS];
    __shared__ RaAxis ay, ax;
    const int k = blockIdx.x, c0 = blockIdx.y * blockDim.x, t = threadIdx.x, c = c0 + t;
    const RaGeom g = ra_geom(mp, rois, roi_batch, k, B, C);
    if (!g.ok) return;  // uniform
    if (t == 0) ra_axis_build(ay, g.sh, g.bh, g.H);
    if (t == 1) ra_axis_build(ax, g.sw, g.bw, g.W);
    const T* src = dy + (size_t)k * C * RA_BINS + (size_t)c0 * RA_BINS;
    const int nrun = blockDim.x * RA_BINS;
    for (int i = t; i < nrun; i += blockDim.x) tile[i] = Elem<T>::ld(src + i);
    __syncthreads();
    const float* mine = tile + t * RA_BINS;
    float* p = g.base + c;
    const int ny = ay.n, nx = ax.n;
    for (int j = 0; j < ny; ++j) {
        const int r = ay.idx[j], plo = ay.lo[j], phi = ay.hi[j];
        for (int i = 0; i < nx; ++i) {
            const int qlo = ax.lo[i], qhi = ax.hi[i];
            float acc = 0.f;
            for (int ph = plo; ph <= phi; ++ph) {
                float rowacc = 0.f;
                for (int pw = qlo; pw <= qhi; ++pw) rowacc += ax.w[i][pw] * mine[ph * RA_P + pw];
                acc += ay.w[j][ph] * rowacc;
            }
            // one wave instruction = 64 consecutive channels of one pixel = 256 contiguous bytes
            unsafeAtomicAdd(p + (size_t)(r * g.W + ax.idx[i]) * C, acc / (float)(RA_S * RA_S));
        }
    }
}

inline bool ra_fill(RaMaps& mp, void* const* maps, const int* hw, const float* scales) {
    for (int l = 0; l < 4; ++l) {
        if (!maps[l] || hw[2 * l] <= 0 || hw[2 * l + 1] <= 0 || !(scales[l] > 0.f)) return false;
        if ((long long)hw[2 * l] * hw[2 * l + 1] > (1 << 26)) return false;
        mp.map[l] = (float*)maps[l];
        mp.H[l] = hw[2 * l];
        mp.W[l] = hw[2 * l + 1];
        mp.scale[l] = scales[l];
    }
    return true;
}
inline int ra_threads(int C) { return C < RA_MAXT ? C : RA_MAXT; }

}  // namespace

// a row of the suppression mask has one word per 64 boxes of the longest segment
extern "C" size_t ssl4gie_nms_workspace_bytes(long long n, int max_seg) {
    if (n <= 0 || n > SSL4GIE_NMS_MAX_TOTAL || max_seg <= 0 || max_seg > NMS_MAX) return 0;
    return (size_t)n * ((max_seg + 63) / 64) * sizeof(u64);
}

extern "C" int ssl4gie_nms_segments(const float* boxes, const unsigned char* valid, const int* seg_off, int n_seg,
                                    long long n, int max_seg, float thr, int* keep_rank, int* count, void* workspace,
                                    void* stream) {
    REQUIRE(boxes && seg_off && keep_rank && count && workspace);
    REQUIRE(n_seg > 0 && n_seg <= 65535 && n > 0 && n <= SSL4GIE_NMS_MAX_TOTAL);
    REQUIRE(max_seg > 0 && max_seg <= NMS_MAX);
    REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)boxes & 15) == 0);
    hipStream_t st = (hipStream_t)stream;
    HIP_RET(hipMemsetAsync(keep_rank, 0xff, sizeof(int) * (size_t)n, st));  // -1: a box outside every segment is dropped
    const int nb = (max_seg + 63) / 64;
    hipLaunchKernelGGL(nms_pairs_kernel, dim3(nb, nb, n_seg), dim3(64), 0, st, boxes, seg_off, n, max_seg, nb, thr,
                       (u64*)workspace);
    hipLaunchKernelGGL(nms_sweep_kernel, dim3(n_seg), dim3(64), 0, st, (const u64*)workspace, valid, seg_off, n,
                       max_seg, nb, keep_rank, count);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int ssl4gie_rpn_decode(const float* const* head, const int* grids, const int* k_off, const float* base_anchors,
                                  int L, int A, int ld, const long long* topk_idx, int B, int F, float min_size,
                                  float score_thresh, float* boxes, float* scores, unsigned char* valid, void* stream) {
    REQUIRE(head && grids && k_off && base_anchors && topk_idx && boxes && scores && valid);
    REQUIRE(L > 0 && L <= SSL4GIE_RPN_MAX_LEVELS && A > 0 && A <= SSL4GIE_RPN_MAX_ANCHORS && ld >= 5 * A);
    REQUIRE(B > 0 && F > 0 && k_off[0] == 0 && ((uintptr_t)boxes & 15) == 0);
    RpnLevels lv;
    for (int l = 0; l < L; ++l) {
        REQUIRE(head[l] && grids[l] > 0 && grids[l] <= F && k_off[l + 1] >= k_off[l]);
        REQUIRE((long long)grids[l] * grids[l] * A <= 0x7fffffffLL);
        lv.head[l] = head[l];
        lv.grid[l] = grids[l];
        lv.koff[l] = k_off[l];
        for (int q = 0; q < A * 4; ++q) lv.base[l * A * 4 + q] = base_anchors[l * A * 4 + q];
    }
    lv.koff[L] = k_off[L];
    const long long total = (long long)B * k_off[L];
    REQUIRE(total > 0 && total <= SSL4GIE_NMS_MAX_TOTAL);
    hipLaunchKernelGGL(rpn_decode_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, lv, L,
                       A, ld, topk_idx, B, F, logf(1000.f / 16.f), min_size, score_thresh, boxes, scores, valid);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int ssl4gie_roi_decode(const float* proposals, const float* logits, int ld_logits, const float* deltas,
                                  int ld_deltas, int K, int C, float wx, float wy, float ww, float wh, float W, float H,
                                  float min_size, float score_thresh, float* boxes, float* scores, unsigned char* valid,
                                  void* stream) {
    REQUIRE(proposals && logits && deltas && boxes && scores && valid);
    REQUIRE(K > 0 && C >= 2 && C <= 4096 && ld_logits >= C && ld_deltas >= 4 * C);
    REQUIRE(wx > 0.f && wy > 0.f && ww > 0.f && wh > 0.f && W > 0.f && H > 0.f);
    REQUIRE(((uintptr_t)boxes & 15) == 0 && ((uintptr_t)proposals & 15) == 0);
    const long long total = (long long)K * (C - 1);
    REQUIRE(total <= SSL4GIE_NMS_MAX_TOTAL);
    hipLaunchKernelGGL(roi_decode_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       proposals, logits, ld_logits, deltas, ld_deltas, K, C, wx, wy, ww, wh, logf(1000.f / 16.f), W, H,
                       min_size, score_thresh, boxes, scores, valid);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int ssl4gie_roi_align_fwd(const float* const* maps, const int* map_hw, const float* scales, int B, int C,
                                     const float* rois, const int* roi_batch, int K, void* out, int out_dtype,
                                     int* levels, void* stream) {
    REQUIRE(maps && map_hw && scales && rois && roi_batch && out);
    REQUIRE(B > 0 && K > 0 && K <= SSL4GIE_NMS_MAX_TOTAL && C >= 64 && C % 64 == 0 && (C <= RA_MAXT || C % RA_MAXT == 0));
    REQUIRE(out_dtype == SSL4GIE_F32 || out_dtype == SSL4GIE_BF16);
    REQUIRE(((uintptr_t)rois & 15) == 0);
    RaMaps mp;
    REQUIRE(ra_fill(mp, (void* const*)maps, map_hw, scales));
    const int T = ra_threads(C);
    const dim3 grid((unsigned)K, (unsigned)(C / T));
    if (out_dtype == SSL4GIE_F32)
        hipLaunchKernelGGL(roi_align_fwd_kernel<float>, grid, dim3(T), 0, (hipStream_t)stream, mp, rois, roi_batch, B, C,
                           (float*)out, levels);
    else
        hipLaunchKernelGGL(roi_align_fwd_kernel<bf16_t>, grid, dim3(T), 0, (hipStream_t)stream, mp, rois, roi_batch, B, C,
                           (bf16_t*)out, levels);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int ssl4gie_roi_align_bwd(float* const* dmaps, const int* map_hw, const float* scales, int B, int C,
                                     const float* rois, const int* roi_batch, int K, const void* dy, int dy_dtype,
                                     void* stream) {
    REQUIRE(dmaps && map_hw && scales && rois && roi_batch && dy);
    REQUIRE(B > 0 && K > 0 && K <= SSL4GIE_NMS_MAX_TOTAL && C >= 64 && C % 64 == 0 && (C <= RA_MAXT || C % RA_MAXT == 0));
    REQUIRE(dy_dtype == SSL4GIE_F32 || dy_dtype == SSL4GIE_BF16);
    REQUIRE(((uintptr_t)rois & 15) == 0);
    RaMaps mp;
    REQUIRE(ra_fill(mp, (void* const*)dmaps, map_hw, scales));
    const int T = ra_threads(C);
    const dim3 grid((unsigned)K, (unsigned)(C / T));
    if (dy_dtype == SSL4GIE_F32)
        hipLaunchKernelGGL(roi_align_bwd_kernel<float>, grid, dim3(T), 0, (hipStream_t)stream, mp, rois, roi_batch, B, C,
                           (const float*)dy);
    else
        hipLaunchKernelGGL(roi_align_bwd_kernel<bf16_t>, grid, dim3(T), 0, (hipStream_t)stream, mp, rois, roi_batch, B, C,
                           (const bf16_t*)dy);
    LAUNCH_CHECK();
    return 0;
}
