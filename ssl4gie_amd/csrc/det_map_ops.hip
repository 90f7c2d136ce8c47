// COCO mean average precision of the detection drivers on the device: Object_detection/train_detection.py:113-151 and
// Object_detection/eval_detection.py:21-44 score the model with torchmetrics' MeanAveragePrecision() (pycocotools'
// COCOeval behind it), which moves everything to the host and loops in Python on every compute().  Three stages:
//
//  * match       one workgroup per image: the image's detections and ground truths are staged in LDS, every detection
//                gets its stable rank among the same-label detections of its image (by counting: at most 1024), and the
//                40 greedy passes of COCOeval.evaluateImg (4 area ranges x 10 IoU thresholds) run as 40 lanes of one
//                wave, each sequential over the first 100 ranked detections of a class.  Per detection: rank, a 40-bit
//                matched mask and a 40-bit ignored mask (bit = area * 10 + threshold).  Per class and area: the number
//                of non-ignored ground truths, by integer atomics.
//  * order       a stable least-significant-digit radix sort (five 8-bit passes over the 40-bit key label : inverted
//                score) of the kept detections; the first pass drops the detections of rank >= 100, the digit totals of
//                the last one are the class segments.  Insertion order breaks ties, as pycocotools' mergesort over the
//                per-image concatenation does.
//  * accumulate  one workgroup per (present class, (area, maxDet) pair, threshold): a chunked prefix scan of tp / fp
//                over the class segment, the suffix maximum of the precision, the 101-point sum and the final recall
//                (COCOeval.accumulate); a last launch of one workgroup forms the twelve summaries, the class list and
//                the label-range flag.
//
// Every decision (IoU, areas, comparisons, recall and precision quotients) is fp64 and rounded operation by operation:
// no contraction.  The library's -ffp-contract=fast disregards the pragma below (only fast-honor-pragmas obeys it, and
// HIP's __dmul_rn / __dsub_rn are plain operators that get fused all the same), so the Makefile builds this object with
// -ffp-contract=off: without it the union of box_iou becomes fma(-w, h, area + area'), the unrounded intersection.
// Counts use integer atomics, floating sums run in a fixed order: bit-identical from run to run.
#include "common.h"
#include "ssl4gie_hip.h"

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

constexpr int DM_MAX = SSL4GIE_DET_MAP_MAX_PER_IMAGE;  // detections / ground truths of one image
constexpr int DM_KEEP = 100;                           // COCOeval's largest maxDet
constexpr int DM_CLASSES = SSL4GIE_DET_MAP_CLASSES;
constexpr int DM_T = 10, DM_A = 4, DM_LANES = DM_T * DM_A, DM_R = 101, DM_COMBOS = 6;
constexpr int DM_BITW = DM_MAX / 32 + 1;               // words of a lane's matched-ground-truth set (+ 1: LDS banks)
constexpr int SORT_TILE = 256, SORT_CHUNK = 4096;      // elements per step / per workgroup of the radix passes
constexpr int SORT_PASSES = 5;
constexpr int ACC_CHUNK = SSL4GIE_DET_MAP_CHUNK;

struct DmIouThr { double t[DM_T]; };
struct DmRecThr { double r[DM_R]; };

DEVI double area_lo(int a) { return a == 2 ? 1024.0 : (a == 3 ? 9216.0 : 0.0); }
DEVI double area_hi(int a) { return a == 1 ? 1024.0 : (a == 2 ? 9216.0 : 1e10); }

// pycocotools' bbIou on (x, y, w, h) boxes without crowd
DEVI double box_iou(double dx, double dy, double dw, double dh, double gx, double gy, double gw, double gh) {
    const double w = fmin(dx + dw, gx + gw) - fmax(dx, gx);
    if (w <= 0.0) return 0.0;
    const double h = fmin(dy + dh, gy + gh) - fmax(dy, gy);
    if (h <= 0.0) return 0.0;
    const double i = w * h;
    const double u = dw * dh + gw * gh - i;  // the ROUNDED intersection: this object is built with -ffp-contract=off
    return i / u;
}

// ------------------------------------------------------------------ match
__global__ __launch_bounds__(256) void dm_match_kernel(const float* __restrict__ det_boxes,
                                                       const float* __restrict__ det_scores,
                                                       const long long* __restrict__ det_labels,
                                                       const int* __restrict__ det_off,
                                                       const float* __restrict__ gt_boxes,
                                                       const long long* __restrict__ gt_labels,
                                                       const int* __restrict__ gt_off, int n_det, int n_gt,
                                                       int* __restrict__ rank_out, u64* __restrict__ matched_out,
                                                       u64* __restrict__ ignored_out, int* __restrict__ npig,
                                                       int* __restrict__ present, int* __restrict__ flag,
                                                       const DmIouThr thr) {
    __shared__ float dX[DM_MAX], dY[DM_MAX], dW[DM_MAX], dH[DM_MAX], dS[DM_MAX];
    __shared__ float gX[DM_MAX], gY[DM_MAX], gW[DM_MAX], gH[DM_MAX];
    __shared__ short dL[DM_MAX], gL[DM_MAX];
    __shared__ unsigned short dOrd[DM_MAX], gOrd[DM_MAX];
    __shared__ unsigned gSet[DM_LANES][DM_BITW];

    const int img = blockIdx.x, tid = threadIdx.x;
    const int d0 = det_off[img], d1 = det_off[img + 1], g0 = gt_off[img], g1 = gt_off[img + 1];
    if (d0 < 0 || d1 < d0 || d1 > n_det || d1 - d0 > DM_MAX || g0 < 0 || g1 < g0 || g1 > n_gt || g1 - g0 > DM_MAX) {
        if (tid == 0) atomicOr(flag, 2);  // offsets that do not describe this image: nothing is read through them
        return;
    }
    const int nd = d1 - d0, ng = g1 - g0;
    bool bad = false;
    for (int i = tid; i < nd; i += 256) {
        const float* b = det_boxes + (size_t)(d0 + i) * 4;
        const float x1 = b[0], y1 = b[1], x2 = b[2], y2 = b[3];
        dX[i] = x1; dY[i] = y1; dW[i] = x2 - x1; dH[i] = y2 - y1;  // box_convert xyxy -> xywh on fp32 tensors
        dS[i] = det_scores[d0 + i];
        const long long l = det_labels[d0 + i];
        const bool ok = l >= 0 && l < DM_CLASSES;
        bad |= !ok;
        dL[i] = ok ? (short)l : (short)DM_CLASSES;
        dOrd[i] = 0xFFFFu;
    }
    for (int i = tid; i < ng; i += 256) {
        const float* b = gt_boxes + (size_t)(g0 + i) * 4;
        const float x1 = b[0], y1 = b[1], x2 = b[2], y2 = b[3];
        gX[i] = x1; gY[i] = y1; gW[i] = x2 - x1; gH[i] = y2 - y1;
        const long long l = gt_labels[g0 + i];
        const bool ok = l >= 0 && l < DM_CLASSES;
        bad |= !ok;
        gL[i] = ok ? (short)l : (short)DM_CLASSES;
        gOrd[i] = 0xFFFFu;
    }
    if (bad) atomicOr(flag, 1);  // a label outside [0, 255]: never an index; the caller raises
    __syncthreads();

    // stable rank among the same-label detections (descending score, insertion order on ties) and the position in the
    // (label, rank) order; a detection of rank >= DM_KEEP or with a refused label is dropped
    for (int i = tid; i < nd; i += 256) {
        const int l = dL[i];
        const float s = dS[i];
        int r = 0, lt = 0;
        for (int j = 0; j < nd; ++j) {
            const int lj = dL[j];
            const float sj = dS[j];
            lt += lj < l;
            r += lj == l && (sj > s || (sj == s && j < i));
        }
        rank_out[d0 + i] = l < DM_CLASSES ? r : DM_MAX;
        if (lt + r < nd) dOrd[lt + r] = (unsigned short)i;  // always, unless a NaN score breaks the order
        if (r >= DM_KEEP || l >= DM_CLASSES) {
            matched_out[d0 + i] = 0;
            ignored_out[d0 + i] = 0;
        }
    }
    for (int i = tid; i < ng; i += 256) {
        const int l = gL[i];
        int p = 0;
        for (int j = 0; j < ng; ++j) {
            const int lj = gL[j];
            p += lj < l || (lj == l && j < i);
        }
        gOrd[p] = (unsigned short)i;
    }
    __syncthreads();
    if (tid >= 64) return;

    // wave 0: lane = area * 10 + threshold walks the classes of the image in label order, all lanes together
    const int lane = tid;
    const bool active = lane < DM_LANES;
    const int a = active ? lane / DM_T : 0, t = active ? lane % DM_T : 0;
    const double lo = area_lo(a), hi = area_hi(a);
    const double thr0 = fmin(thr.t[t], 1.0 - 1e-10);
    unsigned* mine = gSet[active ? lane : 0];
    int di = 0, gi = 0;
    while (true) {
        const int od = di < nd ? dOrd[di] : 0xFFFF, og = gi < ng ? gOrd[gi] : 0xFFFF;
        const int cd = od < nd ? dL[od] : DM_CLASSES, cg = og < ng ? gL[og] : DM_CLASSES;
        const int c = cd < cg ? cd : cg;
        if (c >= DM_CLASSES) break;
        int de = di, ge = gi;
        while (de < nd && dOrd[de] < nd && dL[dOrd[de]] == c) ++de;
        while (ge < ng && gL[gOrd[ge]] == c) ++ge;
        const int ngc = ge - gi;
        if (active) {
            for (int w = 0; w < (ngc + 31) / 32; ++w) mine[w] = 0u;
            if (t == 0) {
                int cnt = 0;
                for (int q = gi; q < ge; ++q) {
                    const int g = gOrd[q];
                    const double ar = (double)gW[g] * (double)gH[g];
                    cnt += !(ar < lo || ar > hi);
                }
                if (cnt) atomicAdd(npig + c * DM_A + a, cnt);
            }
        }
        if (lane == 0) atomicOr(present + c, 1);
        const int kd = de - di < DM_KEEP ? de - di : DM_KEEP;
        for (int k = 0; k < kd; ++k) {
            const int d = dOrd[di + k];
            const double x = (double)dX[d], y = (double)dY[d], w = (double)dW[d], h = (double)dH[d];
            int m = -1;
            bool mig = false;
            if (active) {
                double best = thr0;
                // the ground truths are sorted non-ignored first: one sweep over those, and, only if it took none,
                // one over the ignored ones (the walk stops where they begin once a regular match is held)
                for (int sweep = 0; sweep < 2; ++sweep) {
                    for (int q = gi; q < ge; ++q) {
                        const int g = gOrd[q];
                        const double gw = (double)gW[g], gh = (double)gH[g];
                        const double ar = gw * gh;
                        const bool ig = ar < lo || ar > hi;
                        if (ig != (sweep == 1)) continue;
                        if ((mine[(q - gi) >> 5] >> ((q - gi) & 31)) & 1u) continue;
                        const double iou = box_iou(x, y, w, h, (double)gX[g], (double)gY[g], gw, gh);
                        if (iou < best) continue;
                        best = iou;
                        m = q;
                        mig = ig;
                    }
                    if (m >= 0) break;
                }
                if (m >= 0) mine[(m - gi) >> 5] |= 1u << ((m - gi) & 31);
            }
            const double dar = w * h;
            const bool ign = m >= 0 ? mig : (dar < lo || dar > hi);
            const u64 mm = __ballot(active && m >= 0), im = __ballot(active && ign);
            if (lane == 0) {
                matched_out[d0 + d] = mm;
                ignored_out[d0 + d] = im;
            }
        }
        di = de;
        gi = ge;
    }
}

// ------------------------------------------------------------------ order
// label in bits [39:32]; below it the score's bit pattern mapped so that a larger score gives a smaller key
DEVI u64 dm_key(float score, int label) {
    uint32_t b = __float_as_uint(score);
    if (score == 0.f) b = 0u;  // -0 and +0 tie
    const uint32_t asc = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((u64)(unsigned)label << 32) | (u64)(~asc);
}
struct SortIn {
    const float* scores;       // pass 0: the raw detections
    const long long* labels;
    const int* rank;
    const u64* keys;           // later passes
    const unsigned* idx;
    const int* n_dev;          // later passes: the kept count on the device
    int n;                     // pass 0: all detections
};
DEVI bool sort_load(const SortIn& in, int pass, int i, int n, u64& key, unsigned& idx) {
    if (i >= n) return false;
    if (pass == 0) {
        const long long l = in.labels[i];
        if (in.rank[i] >= DM_KEEP || l < 0 || l >= DM_CLASSES) return false;
        key = dm_key(in.scores[i], (int)l);
        idx = (unsigned)i;
        return true;
    }
    key = in.keys[i];
    idx = in.idx[i];
    return true;
}
DEVI int sort_n(const SortIn& in, int pass) {
    if (pass == 0) return in.n;
    const int n = *in.n_dev;
    return n < 0 ? 0 : (n > in.n ? in.n : n);
}

// table[digit][block] = number of this block's elements with that digit
__global__ __launch_bounds__(SORT_TILE) void dm_sort_hist_kernel(const SortIn in, int pass, int* __restrict__ table,
                                                                 int nb) {
    __shared__ int h[256];
    const int tid = threadIdx.x, n = sort_n(in, pass);
    h[tid] = 0;
    __syncthreads();
    const int base = blockIdx.x * SORT_CHUNK;
    for (int k = 0; k < SORT_CHUNK; k += SORT_TILE) {
        u64 key;
        unsigned idx;
        if (sort_load(in, pass, base + k + tid, n, key, idx)) atomicAdd(&h[(int)((key >> (8 * pass)) & 255u)], 1);
    }
    __syncthreads();
    table[tid * nb + blockIdx.x] = h[tid];
}

// one workgroup: the table becomes exclusive offsets in (digit, block) order; pass 0 leaves the kept count, the last
// pass (the label digit) the class segments
__global__ __launch_bounds__(256) void dm_sort_scan_kernel(int* __restrict__ table, int nb, int pass,
                                                           int* __restrict__ n_kept, int* __restrict__ seg_off) {
    __shared__ int tot[256];
    const int d = threadIdx.x;
    int s = 0;
    for (int b = 0; b < nb; ++b) s += table[d * nb + b];
    tot[d] = s;
    __syncthreads();
    int before = 0;
    for (int j = 0; j < d; ++j) before += tot[j];
    if (pass == SORT_PASSES - 1) {
        seg_off[d] = before;
        if (d == 255) seg_off[256] = before + s;
    }
    if (pass == 0 && d == 255) *n_kept = before + s;
    for (int b = 0; b < nb; ++b) {
        const int c = table[d * nb + b];
        table[d * nb + b] = before;
        before += c;
    }
}

// stable scatter: a tile of 256 elements at a time; an element's place is its digit's running offset + the elements
// of the same digit in earlier waves of the tile + those in lower lanes of its own wave
__global__ __launch_bounds__(SORT_TILE) void dm_sort_scatter_kernel(const SortIn in, int pass,
                                                                    const int* __restrict__ table, int nb,
                                                                    u64* __restrict__ keys_out,
                                                                    unsigned* __restrict__ idx_out) {
    __shared__ int off[256];
    __shared__ int wcnt[4][256];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n = sort_n(in, pass);
    off[tid] = table[tid * nb + blockIdx.x];
    const int base = blockIdx.x * SORT_CHUNK;
    for (int k = 0; k < SORT_CHUNK; k += SORT_TILE) {
        if (base + k >= n) break;  // uniform
#pragma unroll
        for (int w = 0; w < 4; ++w) wcnt[w][tid] = 0;
        __syncthreads();
        u64 key = 0;
        unsigned idx = 0;
        const bool valid = sort_load(in, pass, base + k + tid, n, key, idx);
        const int digit = (int)((key >> (8 * pass)) & 255u);
        u64 peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const u64 bal = __ballot((digit >> b) & 1);
            peers &= ((digit >> b) & 1) ? bal : ~bal;
        }
        const int below = __popcll(peers & ((1ull << lane) - 1ull));
        if (valid && below == 0) wcnt[wave][digit] = __popcll(peers);
        __syncthreads();
        if (valid) {
            int pos = off[digit] + below;
            for (int w = 0; w < wave; ++w) pos += wcnt[w][digit];
            if (pos >= 0 && pos < in.n) {
                keys_out[pos] = key;
                idx_out[pos] = idx;
            }
        }
        __syncthreads();
        off[tid] += wcnt[0][tid] + wcnt[1][tid] + wcnt[2][tid] + wcnt[3][tid];
    }
}

inline int sort_blocks(long long n) { return (int)((n + SORT_CHUNK - 1) / SORT_CHUNK); }
// workspace: keys A | keys B | idx A | idx B | table int [256][blocks] | kept count
struct SortWs { u64 *ka, *kb; unsigned *ia, *ib; int *table, *n_kept; };
inline SortWs sort_ws(void* ws, long long n) {
    SortWs w;
    char* p = (char*)ws;
    w.ka = (u64*)p; p += align256((size_t)n * 8);
    w.kb = (u64*)p; p += align256((size_t)n * 8);
    w.ia = (unsigned*)p; p += align256((size_t)n * 4);
    w.ib = (unsigned*)p; p += align256((size_t)n * 4);
    w.table = (int*)p; p += align256((size_t)256 * sort_blocks(n) * 4);
    w.n_kept = (int*)p;
    return w;
}
inline size_t sort_ws_bytes(long long n) {
    return 2 * align256((size_t)n * 8) + 2 * align256((size_t)n * 4) + align256((size_t)256 * sort_blocks(n) * 4) + 256;
}

// ------------------------------------------------------------------ accumulate
DEVI int combo_area(int combo) { return combo < DM_A ? combo : 0; }
DEVI int combo_maxdet(int combo) { return combo == 4 ? 1 : (combo == 5 ? 10 : DM_KEEP); }

// stats[((c * 6 + combo) * 10 + t) * 2] = sum over the 101 recall thresholds of the interpolated precision, [+ 1] =
// the final recall; both -1 for a class without a non-ignored ground truth in the area
__global__ __launch_bounds__(ACC_CHUNK) void dm_accumulate_kernel(const unsigned* __restrict__ sorted_idx,
                                                                  const int* __restrict__ seg_off,
                                                                  const int* __restrict__ rank,
                                                                  const u64* __restrict__ matched,
                                                                  const u64* __restrict__ ignored,
                                                                  const int* __restrict__ npig,
                                                                  const int* __restrict__ present, int n_det,
                                                                  double* __restrict__ stats, const DmRecThr rec) {
    __shared__ double sm[2][ACC_CHUNK];
    __shared__ int ck[ACC_CHUNK];
    __shared__ int wtot[ACC_CHUNK / 64];
    const int c = blockIdx.x, combo = blockIdx.y, t = blockIdx.z, tid = threadIdx.x;
    if (!present[c]) return;
    const int a = combo_area(combo), maxdet = combo_maxdet(combo), bit = a * DM_T + t;
    double* out = stats + ((size_t)(c * DM_COMBOS + combo) * DM_T + t) * 2;
    const int np = npig[c * DM_A + a];
    if (np <= 0) {
        if (tid == 0) { out[0] = -1.0; out[1] = -1.0; }
        return;
    }
    int s = seg_off[c], e = seg_off[c + 1];
    s = s < 0 ? 0 : (s > n_det ? n_det : s);
    e = e < s ? s : (e > n_det ? n_det : e);
    // thread r: the number of true positives at which the recall first reaches rec.r[r] (at least one: the precision
    // in front of the first true positive is 0, below every later value)
    int kr = 0x7fffffff;
    double best = 0.0;
    if (tid < DM_R) {
        const double th = rec.r[tid], dn = (double)np;
        long long k = (long long)ceil(th * dn);
        k = k < 0 ? 0 : (k > np ? np : k);
        while (k > 0 && (double)(k - 1) / dn >= th) --k;
        while (k < np && (double)k / dn < th) ++k;
        kr = k < 1 ? 1 : (int)k;
    }
    int K0 = 0, F0 = 0;
    for (int base = s; base < e; base += ACC_CHUNK) {
        const int i = base + tid;
        int tp = 0, fp = 0;
        if (i < e) {
            const unsigned j = sorted_idx[i];
            if (j < (unsigned)n_det && rank[j] < maxdet && !((ignored[j] >> bit) & 1ull)) {
                tp = (int)((matched[j] >> bit) & 1ull);
                fp = 1 - tp;
            }
        }
        // inclusive scan of (tp, fp) packed as tp | fp << 16 (at most 256 each)
        int v = tp | (fp << 16);
        const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(v, o, 64);
            if (lane >= o) v += u;
        }
        if (lane == 63) wtot[wave] = v;
        __syncthreads();
        for (int w = 0; w < wave; ++w) v += wtot[w];
        const int ctp = K0 + (v & 0xffff), cfp = F0 + (v >> 16);
        // pr = tp / (fp + tp + np.spacing(1)) at a true positive; anywhere else it is no larger than at the one before
        sm[0][tid] = tp ? (double)ctp / ((double)(cfp + ctp) + 2.220446049250313e-16) : 0.0;
        ck[tid] = ctp;
        __syncthreads();
        int cur = 0;
        for (int o = 1; o < ACC_CHUNK; o <<= 1) {  // suffix maximum
            double x = sm[cur][tid];
            if (tid + o < ACC_CHUNK) x = fmax(x, sm[cur][tid + o]);
            sm[cur ^ 1][tid] = x;
            cur ^= 1;
            __syncthreads();
        }
        if (tid < DM_R) {
            int lo = 0, hi = ACC_CHUNK;  // first entry of the chunk with ck >= kr
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (ck[mid] >= kr) hi = mid; else lo = mid + 1;
            }
            if (lo < ACC_CHUNK) best = fmax(best, sm[cur][lo]);
        }
        const int last = ck[ACC_CHUNK - 1];
        int fsum = wtot[0] >> 16;
        for (int w = 1; w < ACC_CHUNK / 64; ++w) fsum += wtot[w] >> 16;
        K0 = last;
        F0 += fsum;
        __syncthreads();
    }
    sm[0][tid] = tid < DM_R ? best : 0.0;
    __syncthreads();
    if (tid == 0) {
        double sum = 0.0;
        for (int r = 0; r < DM_R; ++r) sum += sm[0][r];
        out[0] = sum;
        out[1] = (double)K0 / (double)np;
    }
}

// the twelve summaries (COCOeval.summarize as torchmetrics 1.1.2 reads it): the mean over the entries > -1, -1 without
// any.  out64 / out32 [12]: map, map_50, map_75, map_small, map_medium, map_large, mar_1, mar_10, mar_100, mar_small,
// mar_medium, mar_large.  outi: [0] number of classes, [1] flag word, [2 ...] the classes seen, ascending.
__global__ __launch_bounds__(256) void dm_summarize_kernel(const double* __restrict__ stats,
                                                           const int* __restrict__ npig,
                                                           const int* __restrict__ present,
                                                           const int* __restrict__ flag, double* __restrict__ out64,
                                                           float* __restrict__ out32, int* __restrict__ outi) {
    __shared__ double val[12][DM_CLASSES];
    __shared__ int cnt[12][DM_CLASSES];
    const int c = threadIdx.x;
    // summary k: combo, which statistic (0 precision sum, 1 recall), first threshold, number of thresholds
    const int combo_of[12] = {0, 0, 0, 1, 2, 3, 4, 5, 0, 1, 2, 3};
    const int t0_of[12] = {0, 0, 5, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int nt_of[12] = {DM_T, 1, 1, DM_T, DM_T, DM_T, DM_T, DM_T, DM_T, DM_T, DM_T, DM_T};
    const bool here = present[c] != 0;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        const int combo = combo_of[k], which = k >= 6;
        double v = 0.0;
        int n = 0;
        if (here && npig[c * DM_A + combo_area(combo)] > 0) {
            const double* st = stats + (size_t)(c * DM_COMBOS + combo) * DM_T * 2;
            for (int t = t0_of[k]; t < t0_of[k] + nt_of[k]; ++t) v += st[t * 2 + which];
            n = 1;
        }
        val[k][c] = v;
        cnt[k][c] = n;
    }
    __syncthreads();
    if (c < 12) {
        double sum = 0.0;
        int n = 0;
        for (int j = 0; j < DM_CLASSES; ++j) { sum += val[c][j]; n += cnt[c][j]; }
        const double per = (double)nt_of[c] * (c < 6 ? (double)DM_R : 1.0);
        const double r = n ? sum / ((double)n * per) : -1.0;
        out64[c] = r;
        out32[c] = (float)r;
    }
    if (c == 0) {
        int n = 0;
        for (int j = 0; j < DM_CLASSES; ++j)
            if (present[j]) outi[2 + n++] = j;
        for (int j = n; j < DM_CLASSES; ++j) outi[2 + j] = -1;
        outi[0] = n;
        outi[1] = *flag;
    }
}

}  // namespace

// the workspace is the sort's: its size depends on n_det alone; n_img and n_gt are only checked (0 for a size <= 0)
extern "C" size_t ssl4gie_det_map_workspace_bytes(int n_img, long long n_det, long long n_gt) {
    if (n_img <= 0 || n_det <= 0 || n_gt <= 0 || n_det > SSL4GIE_DET_MAP_MAX_TOTAL || n_gt > SSL4GIE_DET_MAP_MAX_TOTAL)
        return 0;
    return sort_ws_bytes(n_det);
}

extern "C" int ssl4gie_det_map_match(const float* det_boxes, const float* det_scores, const long long* det_labels,
                                     const int* det_off, const float* gt_boxes, const long long* gt_labels,
                                     const int* gt_off, int n_img, long long n_det, long long n_gt,
                                     const double* iou_thresholds, int* rank, unsigned long long* matched,
                                     unsigned long long* ignored, int* npig, int* present, int* flag, void* stream) {
    REQUIRE(det_off && gt_off && iou_thresholds && npig && present && flag && n_img > 0);
    REQUIRE(n_det >= 0 && n_gt >= 0 && n_det <= SSL4GIE_DET_MAP_MAX_TOTAL && n_gt <= SSL4GIE_DET_MAP_MAX_TOTAL);
    REQUIRE(n_det == 0 || (det_boxes && det_scores && det_labels && rank && matched && ignored));
    REQUIRE(n_gt == 0 || (gt_boxes && gt_labels));
    hipStream_t st = (hipStream_t)stream;
    DmIouThr thr;
    for (int t = 0; t < DM_T; ++t) thr.t[t] = iou_thresholds[t];
    HIP_RET(hipMemsetAsync(npig, 0, sizeof(int) * DM_CLASSES * DM_A, st));
    HIP_RET(hipMemsetAsync(present, 0, sizeof(int) * DM_CLASSES, st));
    HIP_RET(hipMemsetAsync(flag, 0, sizeof(int), st));
    hipLaunchKernelGGL(dm_match_kernel, dim3((unsigned)n_img), dim3(256), 0, st, det_boxes, det_scores, det_labels,
                       det_off, gt_boxes, gt_labels, gt_off, (int)n_det, (int)n_gt, rank, (u64*)matched, (u64*)ignored,
                       npig, present, flag, thr);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int ssl4gie_det_map_order(const float* det_scores, const long long* det_labels, const int* rank,
                                     long long n_det, unsigned* sorted_idx, int* seg_off, void* workspace,
                                     void* stream) {
    REQUIRE(det_scores && det_labels && rank && sorted_idx && seg_off && workspace);
    REQUIRE(n_det > 0 && n_det <= SSL4GIE_DET_MAP_MAX_TOTAL && ((uintptr_t)workspace & 15) == 0);
    hipStream_t st = (hipStream_t)stream;
    const SortWs w = sort_ws(workspace, n_det);
    const int nb = sort_blocks(n_det);
    for (int pass = 0; pass < SORT_PASSES; ++pass) {
        SortIn in;
        in.scores = det_scores; in.labels = det_labels; in.rank = rank;
        in.keys = (pass & 1) ? w.ka : w.kb;   // pass 0 writes A, pass 1 reads A and writes B, ...
        in.idx = (pass & 1) ? w.ia : w.ib;
        in.n_dev = w.n_kept;
        in.n = (int)n_det;
        u64* ko = (pass & 1) ? w.kb : w.ka;
        unsigned* io = pass == SORT_PASSES - 1 ? sorted_idx : ((pass & 1) ? w.ib : w.ia);
        hipLaunchKernelGGL(dm_sort_hist_kernel, dim3(nb), dim3(SORT_TILE), 0, st, in, pass, w.table, nb);
        hipLaunchKernelGGL(dm_sort_scan_kernel, dim3(1), dim3(256), 0, st, w.table, nb, pass, w.n_kept, seg_off);
        hipLaunchKernelGGL(dm_sort_scatter_kernel, dim3(nb), dim3(SORT_TILE), 0, st, in, pass, (const int*)w.table, nb,
                           ko, io);
    }
    LAUNCH_CHECK();
    return 0;
}

extern "C" int ssl4gie_det_map_accumulate(const unsigned* sorted_idx, const int* seg_off, const int* rank,
                                          const unsigned long long* matched, const unsigned long long* ignored,
                                          const int* npig, const int* present, const int* flag, long long n_det,
                                          const double* rec_thresholds, double* stats, double* out64, float* out32,
                                          int* outi, void* stream) {
    REQUIRE(seg_off && npig && present && flag && rec_thresholds && stats && out64 && out32 && outi);
    REQUIRE(n_det >= 0 && n_det <= SSL4GIE_DET_MAP_MAX_TOTAL);
    REQUIRE(n_det == 0 || (sorted_idx && rank && matched && ignored));
    hipStream_t st = (hipStream_t)stream;
    DmRecThr rec;
    for (int r = 0; r < DM_R; ++r) rec.r[r] = rec_thresholds[r];
    hipLaunchKernelGGL(dm_accumulate_kernel, dim3(DM_CLASSES, DM_COMBOS, DM_T), dim3(ACC_CHUNK), 0, st, sorted_idx,
                       seg_off, rank, (const u64*)matched, (const u64*)ignored, npig, present, (int)n_det, stats, rec);
    hipLaunchKernelGGL(dm_summarize_kernel, dim3(1), dim3(256), 0, st, (const double*)stats, npig, present, flag,
                       out64, out32, outi);
    LAUNCH_CHECK();
    return 0;
}
