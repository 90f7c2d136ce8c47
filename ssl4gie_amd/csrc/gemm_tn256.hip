// 256x256x64 ping-pong bf16 TN GEMM for gfx950:  C[M,N] = alpha * At[K,M]^T Bt[K,N]  (fp32 out).
//
// The weight-gradient product dW[out,in] = dY[T,out]^T X[T,in]: the contraction runs over tokens
// (K = T = 12 800 / 50 432 in the MAE step) while M, N are the small layer widths, so the work is
// split along K across workgroups (fp32 slabs + deterministic slab reduction, no atomics).
//
// The four-phase schedule gemm_nt256.hip had until round 4 (4 phases per K-tile of 16 MFMAs, two staggered wave
// rows, LDS-DMA half-tile stream 7 ahead behind a counted vmcnt; hazard bookkeeping in that file's header).  The
// two-phase form that made the NT K-loop 8 % faster was measured here too and is 4-5 % SLOWER (dec.dWfc1 104 ->
// 116 us, profiles/r04t_tn_two_phase.log): a phase would issue 32 transposed reads against the 4-bit lgkmcnt.  What
// differs is the operand image: both operands are k-major in memory, so a half-tile is 64 k-rows x
// 256 B (128 m- or n-values), staged by 4-row LDS-DMA pieces, and MFMA fragments are gathered
// with ds_read_b64_tr_b16 (hardware transpose, two reads per fragment).  Image: 16-B chunk c of
// k-row r at position c ^ tn_swz(r) (same swizzle as the 128x128 TN kernel, conflict-free for the
// transposed reads; tools/lds_bank_sim.py).  P0 issues 8 + 16 transposed reads; lgkmcnt is a
// 4-bit counter, so the early retire of the B_h0 reads is s_waitcnt lgkmcnt(15) (oldest 9 done).
//
// Replaces the autograd weight-gradient GEMMs of nn.Linear in timm Block / MAE decoder (SURVEY
// §2.2 "bwd adds dW = X^T dY"; reference modules Models/mae/models_mae.py:39-41,47,53-55,59).
#include "gemm256.h"
#include "prof.h"

#include <type_traits>

DEVI int q_swz(int k) { return ((k & 3) | ((k >> 1) & 4)) << 1; }

// MFMA operand (16 x-values x 32 k) out of a k-major half-tile image: lane l gets, for
// x = x0 + (l & 15), the 8 k-values krow0 .. krow0+7 (krow0 = 32 ks + 8 (l >> 4))
DEVI bf16x8 q_frag(const char* img, int krow0, int x0, int lane) {
    const int q = (lane & 15) >> 2, p = lane & 3;
    const int c = (x0 >> 3) + (p >> 1);
    const int r0 = krow0 + q, r1 = krow0 + 4 + q;
    const int o0 = r0 * 256 + ((c ^ q_swz(r0)) << 4) + ((p & 1) << 3);
    const int o1 = r1 * 256 + ((c ^ q_swz(r1)) << 4) + ((p & 1) << 3);
    typedef __attribute__((address_space(3))) s16x4* lp_t;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp_t)(img + o0));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp_t)(img + o1));
    typedef __attribute__((ext_vector_type(8))) short s16x8;
    const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, v);
}

// grid.x = ntiles * splits; split s of tile t covers K-tiles [nkt*s/splits, nkt*(s+1)/splits).
// COLSUM: the workgroups of the first tile column (n0 == 0) also produce colsum[m] = sum_k At[k][m]
// (the bias gradient): wave (wr, wc) multiplies its wc-th A fragment of each quadrant against a
// ones fragment — 2 extra MFMAs in P0 and in P2 — and writes 2 x 16 sums.
// CONV: 0 = Bt is a matrix; 1 = Bt is the implicit 3x3 patch matrix of the map at `Bt` (k-row =
// output pixel, column = (tap, channel); ssl4gie_conv3x3_geom); 2 = with ReLU on the B fragments.
// PARTIAL: the launch has tiles that M x N does not fill (see `mmask` below); a separate instantiation, so that
// the full-tile kernels keep their register allocation.
template <bool COLSUM, int CONV, bool PARTIAL = false>
__global__ __launch_bounds__(512, 2) void gemm_bf16_tn256_kernel(
    const bf16_t* __restrict__ At, long long ldat, const bf16_t* __restrict__ Bt, long long ldbt,
    float* __restrict__ C, long long ldc, float* __restrict__ slabs, int M, int N, int K,
    int tiles_n, int ntiles, int splits, float alpha, int accumulate, float* __restrict__ colsum,
    float* __restrict__ colsum_part, ConvK cg, TnExtras ex) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int all_tiles = ntiles + ex.total_tiles;
    const int split = bid / all_tiles;
    int tile = bid % all_tiles;
    if (tile >= ntiles) {  // grouped launch: this workgroup belongs to a later product (uniform)
        const int rel = tile - ntiles;
#pragma unroll
        for (int i = 0; i < TN_GROUP_MAX - 1; ++i) {
            if (i < ex.n && rel >= ex.p[i].tile0 && rel < ex.p[i].tile0 + ex.p[i].ntiles) {
                tile = rel - ex.p[i].tile0;
                At = (const bf16_t*)ex.p[i].At; ldat = ex.p[i].ldat;
                Bt = (const bf16_t*)ex.p[i].Bt; ldbt = ex.p[i].ldbt;
                C = ex.p[i].C; ldc = ex.p[i].ldc; slabs = ex.p[i].slabs;
                M = ex.p[i].M; N = ex.p[i].N; tiles_n = ex.p[i].tiles_n;
                colsum = ex.p[i].colsum; colsum_part = ex.p[i].colsum_part;
                alpha = ex.p[i].alpha; accumulate = ex.p[i].accumulate;
            }
        }
    }
    // Consecutive tiles of one K-split sit on one XCD (xcd_remap) and share operand slabs through its
    // L2: a run of r x c tiles reads r + c slabs, so the run should be as square as possible — the
    // SHORTER tile dimension is the inner one (a 3 x 12 product walked row by row makes a 27-tile XCD
    // chunk read 3 + 12 slabs and its 9-tile neighbour 1 + 9; column by column they read 3 + 9 and 3 + 3:
    // 18 slab reads instead of 25 against a minimum of 15).
    const int tiles_m = (M + P_BM - 1) / P_BM;
    const bool m_inner = tiles_m < tiles_n;
    const int m0 = (m_inner ? tile % tiles_m : tile / tiles_n) * P_BM;
    const int n0 = (m_inner ? tile / tiles_m : tile % tiles_n) * P_BN;
    const int nkt = K / P_BK;
    const int kt0 = (int)((long long)nkt * split / splits);
    const int kt1 = (int)((long long)nkt * (split + 1) / splits);
    const int total_kt = kt1 - kt0;

    // ---- LDS-DMA stream: this lane's source element offsets (without the k-row term of the
    // K-tile, which advances the wave-uniform base): piece i covers k-rows 4 (2 wave + i) .. +3
    unsigned v0_0, v0_1, v1_0, v1_1, v2_0, v2_1, v3_0, v3_1;
    // CONV: v0_* / v2_* hold the lane's tap as ((dy*W + dx)*C + ci)*2 | dy << 2 | dx (the byte
    // offset is a multiple of 16); the pixel of k-row piece i of the cursor's K-tile is kept as
    // o_i (byte offset of its tap (0,0)) and yx_i (y0 << 16 | x0 & 0xffff)
    const int c_H = cg.H, c_W = cg.W, c_C = cg.C, c_Wo = cg.Wo, c_HoWo = cg.HoWo, c_s = cg.stride;
    const unsigned c_mgw = cg.mg_wo, c_shw = cg.sh_wo, c_mgh = cg.mg_hw, c_shh = cg.sh_hw;
    const char* c_zero = (const char*)cg.zero;
    int o_0 = 0, o_1 = 0;
    unsigned yx_0 = 0, yx_1 = 0;
    {
        const int mch = (M >> 3) - 1, nch = (N >> 3) - 1;  // last valid 16-B chunk of a row
        auto offs = [&](int i, int h, bool is_a) -> unsigned {
            const int kr = (wave * 2 + i) * 4 + (lane >> 4);  // k-row inside the K-tile
            const int c = (lane & 15) ^ q_swz(kr);            // logical chunk kept at position l&15
            if (is_a) {
                int ch = ((m0 + (c >> 3) * 128 + h * 64) >> 3) + (c & 7);
                ch = ch < mch ? ch : mch;
                return (unsigned)(((long long)kr * ldat + ch * 8) * 2);
            }
            int ch = ((n0 + (c >> 2) * 64 + h * 32) >> 3) + (c & 3);
            ch = ch < nch ? ch : nch;
            if constexpr (CONV != 0) {
                const int n = ch * 8, tap = n / c_C, ci = n - tap * c_C;
                const int dy = tap / 3, dx = tap - dy * 3;
                return (unsigned)((((dy * c_W + dx) * c_C + ci) * 2) | (dy << 2) | dx);
            }
            return (unsigned)(((long long)kr * ldbt + ch * 8) * 2);
        };
        v0_0 = offs(0, 0, false); v0_1 = offs(1, 0, false);  // B_h0
        v1_0 = offs(0, 0, true);  v1_1 = offs(1, 0, true);   // A_h0
        v2_0 = offs(0, 1, false); v2_1 = offs(1, 1, false);  // B_h1
        v3_0 = offs(0, 1, true);  v3_1 = offs(1, 1, true);   // A_h1
    }
    const unsigned lds0 = __builtin_amdgcn_readfirstlane(p_lds_addr(smem) + wave * 2048);
    int s_kt = 0;  // stream cursor (K-tile relative to kt0)
    auto issue = [&](auto Jc) {
        constexpr int J = decltype(Jc)::value;
        if (s_kt < total_kt) {
            const unsigned dst = lds0 + (s_kt & 1) * P_BUF + J * P_HALF;
            const size_t krow = (size_t)(kt0 + s_kt) * P_BK;
            const bf16_t* base = (J & 1) ? At + krow * ldat : Bt + krow * ldbt;
            const unsigned va = J == 0 ? v0_0 : J == 1 ? v1_0 : J == 2 ? v2_0 : v3_0;
            const unsigned vb = J == 0 ? v0_1 : J == 1 ? v1_1 : J == 2 ? v2_1 : v3_1;
            if constexpr (CONV != 0 && !(J & 1)) {
                if (J == 0) {  // decompose the two k-rows (output pixels) of this K-tile once
                    auto pix = [&](int i, int& o, unsigned& yx) {
                        const unsigned m = (unsigned)krow + (wave * 2 + i) * 4 + (lane >> 4);
                        const unsigned b = p_fastdiv(m, c_mgh, c_shh);
                        const unsigned r = m - b * (unsigned)c_HoWo;
                        const unsigned oy = p_fastdiv(r, c_mgw, c_shw);
                        const unsigned ox = r - oy * (unsigned)c_Wo;
                        const int y0 = (int)oy * c_s - 1, x0 = (int)ox * c_s - 1;
                        o = ((((int)b * c_H + y0) * c_W + x0) * c_C) * 2;
                        yx = ((unsigned)y0 << 16) | ((unsigned)x0 & 0xffffu);
                    };
                    pix(0, o_0, yx_0);
                    pix(1, o_1, yx_1);
                }
                auto src = [&](unsigned tapv, int o, unsigned yx) -> const char* {
                    const int y = ((int)yx >> 16) + (int)((tapv >> 2) & 3);
                    const int x = (int)(short)(yx & 0xffffu) + (int)(tapv & 3);
                    const bool ok = (unsigned)y < (unsigned)c_H && (unsigned)x < (unsigned)c_W;
                    return ok ? (const char*)Bt + (long long)(o + (int)(tapv & ~15u)) : c_zero;
                };
                p_glds2v(src(va, o_0, yx_0), src(vb, o_1, yx_1), dst, dst + 1024);
            } else {
                p_glds2(base, va, vb, dst, dst + 1024);
            }
        }
        if (J == 3) ++s_kt;
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    using I3 = std::integral_constant<int, 3>;

    const int kl = 8 * (lane >> 4);
    // Unused: what is left of the retired fragment-read ablation.  The optimiser deletes it, but without it the
    // compiler orders the prologue of six instantiations differently (same registers, four of them 4 bytes longer),
    // and the shipped kernels stay as they were measured (profiles/gemm256_dispatch_codegen.md).
    [[maybe_unused]] bf16x8 unused_z;
#pragma unroll
    for (int j = 0; j < 8; ++j) unused_z[j] = (__bf16)(0.001f * (float)(lane + j));
    auto ldA = [&](int buf, int h, int mi, int ks) -> bf16x8 {
        return q_frag(smem + buf * P_BUF + (h ? 3 : 1) * P_HALF, ks * 32 + kl, wr * 64 + mi * 16, lane);
    };
    auto ldB = [&](int buf, int h, int ni, int ks) -> bf16x8 {
        return q_frag(smem + buf * P_BUF + (h ? 2 : 0) * P_HALF, ks * 32 + kl, wc * 32 + ni * 16, lane);
    };

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0, 0, 0, 0};
    bf16x8 a[4][2], b0[2][2], b1[2][2];
    f32x4 accb[2] = {f32x4{0, 0, 0, 0}, f32x4{0, 0, 0, 0}};
    const bool do_cs = COLSUM && (n0 == 0) && colsum != nullptr;
    bf16x8 ones;
#pragma unroll
    for (int j = 0; j < 8; ++j) ones[j] = (__bf16)1.0f;

    // Partial tiles (the 1x1-convolution weight gradients of ResNet's first stages: dW [64, 256], [128, 512] ...
    // over hundreds of thousands of pixels — one or two tiles, HBM-streaming): 16-row / 16-column fragment blocks
    // that lie wholly outside M x N are skipped (wave-uniform masks), so a 64-row product costs a quarter of the
    // tile's MFMAs instead of all of them and stays HBM-bound.  Full tiles take the unconditional sequence.
    [[maybe_unused]] unsigned mmask = 0xffu, nmask = 0xfu;
    if constexpr (PARTIAL) {
        mmask = nmask = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) mmask |= (m0 + wr * 128 + (i >> 2) * 64 + (i & 3) * 16 < M ? 1u : 0u) << i;
#pragma unroll
        for (int i = 0; i < 4; ++i) nmask |= (n0 + wc * 64 + (i >> 1) * 32 + (i & 1) * 16 < N ? 1u : 0u) << i;
        mmask = __builtin_amdgcn_readfirstlane(mmask);
        nmask = __builtin_amdgcn_readfirstlane(nmask);
    }
    auto mma = [&](auto QMc, auto QNc, bf16x8 (&bb)[2][2]) {
        constexpr int QM = decltype(QMc)::value, QN = decltype(QNc)::value;
        __builtin_amdgcn_s_setprio(1);
        if constexpr (CONV == 2 && QM == 0) {  // P0 has just loaded b0, P1 b1
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) bb[ni][ks] = p_relu8(bb[ni][ks]);
        }
        if constexpr (COLSUM && QM == QN) {  // P0 and P2: the phases that have just loaded `a`
            if (do_cs) {
                auto cs = [&](bf16x8 (&af)[2]) {
                    accb[QM] = P_MFMA(ones, af[0], accb[QM]);
                    accb[QM] = P_MFMA(ones, af[1], accb[QM]);
                };
                if (wc == 0) cs(a[0]);
                else if (wc == 1) cs(a[1]);
                else if (wc == 2) cs(a[2]);
                else cs(a[3]);
            }
        }
        if constexpr (!PARTIAL) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni)
                        acc[QM * 4 + mi][QN * 2 + ni] =
                            P_MFMA(bb[ni][ks], a[mi][ks], acc[QM * 4 + mi][QN * 2 + ni]);
        } else {
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) {
                if (!((mmask >> (QM * 4 + mi)) & 1u)) continue;
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) {
                    if (!((nmask >> (QN * 2 + ni)) & 1u)) continue;
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks)
                        acc[QM * 4 + mi][QN * 2 + ni] =
                            P_MFMA(bb[ni][ks], a[mi][ks], acc[QM * 4 + mi][QN * 2 + ni]);
                }
            }
        }
        __builtin_amdgcn_s_setprio(0);
    };

    if (total_kt > 0) {
        issue(I0{}); issue(I1{}); issue(I2{}); issue(I3{});
        issue(I0{}); issue(I1{}); issue(I2{});
        if (total_kt >= 2) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (wr == 1) __builtin_amdgcn_s_barrier();

        for (int T = 0; T < total_kt; ++T) {
            const int cb = T & 1;
            // ---------------- P0
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) b0[ni][ks] = ldB(cb, 0, ni, ks);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) a[mi][ks] = ldA(cb, 0, mi, ks);
            __builtin_amdgcn_sched_barrier(0);
            issue(I3{});
            asm volatile("s_waitcnt lgkmcnt(15)" ::: "memory");  // the 8 B_h0 reads are retired
            __builtin_amdgcn_s_barrier();
            mma(I0{}, I0{}, b0);
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            // ---------------- P1
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) b1[ni][ks] = ldB(cb, 1, ni, ks);
            __builtin_amdgcn_sched_barrier(0);
            issue(I0{});
            __builtin_amdgcn_s_barrier();
            mma(I0{}, I1{}, b1);
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            // ---------------- P2
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) a[mi][ks] = ldA(cb, 1, mi, ks);
            __builtin_amdgcn_sched_barrier(0);
            issue(I1{});
            __builtin_amdgcn_s_barrier();
            mma(I1{}, I1{}, b1);
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            // ---------------- P3
            issue(I2{});
            if (T + 2 < total_kt) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            mma(I1{}, I0{}, b0);
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
        }
        if (wr == 0) __builtin_amdgcn_s_barrier();
    }

    // ---- column sums: D[n][m] is the same for every n, so lanes 0..15 hold m = l, register 0
    if constexpr (COLSUM) {
        if (do_cs && lane < 16) {
#pragma unroll
            for (int qm = 0; qm < 2; ++qm) {
                const int m = m0 + wr * 128 + qm * 64 + wc * 16 + lane;
                if (m < M) {
                    if (splits == 1) colsum[m] = accumulate ? colsum[m] + accb[qm][0] : accb[qm][0];
                    else colsum_part[(size_t)split * M + m] = accb[qm][0];
                }
            }
        }
    }
    // ---- epilogue: slab (splits > 1) or C
    const f32x4 zero4 = {0, 0, 0, 0};
    char* stg = smem + 2 * P_BUF + wave * P_STG_WAVE;
    float* out = (splits == 1) ? C : slabs + (size_t)split * M * N;
    const long long ldo = (splits == 1) ? ldc : N;
    const float al = (splits == 1) ? alpha : 1.f;
    const bool accu = (splits == 1) && accumulate;
    if (m0 + P_BM <= M && n0 + P_BN <= N)
        p_store_f32<true, false>(acc, stg, al, zero4, nullptr, 0, accu, out, ldo, m0 + wr * 128,
                                 n0 + wc * 64, M, N, lane);
    else
        p_store_f32<false, false>(acc, stg, al, zero4, nullptr, 0, accu, out, ldo, m0 + wr * 128,
                                  n0 + wc * 64, M, N, lane);
}

// =====================================================================================
// Round 5: the K-SPLIT form of the same product (plain operands, full or clamped tiles).
//
// What the ablations of the kernel above showed (profiles/r05a; the ablation switches are retired, profiles/HISTORY.md): its K-loop is
// not bound by the transposed reads (reads + skeleton alone: 0.2 us per K-tile) but by two things that add up —
// the four-phase skeleton around the MFMAs (1.67 us per K-tile with MFMAs only: 8 intervals of 16 MFMAs + ~110
// cycles of barrier / wait overhead each, where the NT kernel's two-phase form has 4 of 32) and the LDS-DMA stream
// (1.6 us per K-tile with the DMA only), whose requests were 128-byte (A) and 64-byte (B) pieces of a row: a
// half-tile was "half of the tile's COLUMNS over all 64 k-rows", the NT kernel's split, which suits operands that
// are contiguous along k.  These operands are contiguous along m / n, so here a stage is "32 K-ROWS of all 256
// columns": a row is one contiguous 512-byte run, a DMA piece two whole rows.
//
//  * stage = 32 k-rows of A (16 KiB) + 32 k-rows of B (16 KiB); ring of 4 stages (A stages at 0 .. 64 KiB, B stages
//    at 64 .. 128 KiB, so that every fragment address is a loop-invariant VGPR + a 16-bit immediate);
//  * ONE uniform phase per stage: {LOAD: 24 ds_read_b64_tr_b16 (8 A + 4 B fragments: the k extent of a stage IS the
//    32 of one MFMA) + the DMA of stage s + 3 (two A pieces, two B pieces per wave) + the counted wait for stage
//    s + 1 + lgkmcnt(0); s_barrier; MMA: 32 MFMAs; s_barrier} — the two wave rows one barrier apart as before;
//    48 fragment registers instead of 64, reads balanced 24 / 24 instead of 24 / 8 / 16 / 0;
//  * hazards (interval I_n between barriers n - 1 and n; wr = 0 runs LOAD(s) in I_2s and MMA(s) in I_2s+1, wr = 1
//    one interval later):
//      WAR  LOAD(s) issues stage s + 3 = s - 1 (mod 4) over what LOAD(s - 1) read; every LOAD ends with
//           lgkmcnt(0) before its barrier, so either group's reads of LOAD(s - 1) are complete at least one
//           barrier before either group's LOAD(s);
//      RAW  each wave waits at the end of LOAD(s) until all but its 8 youngest pieces (stages s + 2, s + 3) have
//           landed, i.e. its pieces of stage s + 1; wr = 0 reads stage s + 1 in I_2s+2, after the barrier that
//           ends wr = 1's LOAD(s) in I_2s+1.
// Image of a stage half: k-row r at r * 512 B, 32-byte unit u (16 m- or n-values) at position u ^ k_swz(r): the 32
// lanes of a ds_read_b64_tr_b16 group read 8 rows x 32 B and k_swz takes 8 distinct values on them (conflict-free).
// Same accumulator layout, same per-accumulator summation order (k ascending) as the kernel above: results are
// bit-identical.  Every product with plain operands and full (or clamped) tiles runs here; the kernel above keeps the
// patch-matrix operands (CONV) and the lone partial-tile products (PARTIAL).
DEVI int k_swz(int k) { return (k & 3) | ((k >> 1) & 4); }

template <bool COLSUM>
__global__ __launch_bounds__(512, 2) void gemm_bf16_tn256k_kernel(
    const bf16_t* __restrict__ At, long long ldat, const bf16_t* __restrict__ Bt, long long ldbt,
    float* __restrict__ C, long long ldc, float* __restrict__ slabs, int M, int N, int K,
    int tiles_n, int ntiles, int splits, float alpha, int accumulate, float* __restrict__ colsum,
    float* __restrict__ colsum_part, TnExtras ex) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int all_tiles = ntiles + ex.total_tiles;
    const int split = bid / all_tiles;
    int tile = bid % all_tiles;
    if (tile >= ntiles) {  // grouped launch: this workgroup belongs to a later product (uniform)
        const int rel = tile - ntiles;
#pragma unroll
        for (int i = 0; i < TN_GROUP_MAX - 1; ++i) {
            if (i < ex.n && rel >= ex.p[i].tile0 && rel < ex.p[i].tile0 + ex.p[i].ntiles) {
                tile = rel - ex.p[i].tile0;
                At = (const bf16_t*)ex.p[i].At; ldat = ex.p[i].ldat;
                Bt = (const bf16_t*)ex.p[i].Bt; ldbt = ex.p[i].ldbt;
                C = ex.p[i].C; ldc = ex.p[i].ldc; slabs = ex.p[i].slabs;
                M = ex.p[i].M; N = ex.p[i].N; tiles_n = ex.p[i].tiles_n;
                colsum = ex.p[i].colsum; colsum_part = ex.p[i].colsum_part;
                alpha = ex.p[i].alpha; accumulate = ex.p[i].accumulate;
            }
        }
    }
    const int tiles_m = (M + P_BM - 1) / P_BM;
    const bool m_inner = tiles_m < tiles_n;  // (tile walk: see the kernel above)
    const int m0 = (m_inner ? tile % tiles_m : tile / tiles_n) * P_BM;
    const int n0 = (m_inner ? tile / tiles_m : tile % tiles_n) * P_BN;
    const int nkt = K / P_BK;
    const int kt0 = (int)((long long)nkt * split / splits);
    const int kt1 = (int)((long long)nkt * (split + 1) / splits);
    const int total_kt = kt1 - kt0;
    const int nph = 2 * total_kt;  // 32-row stages

    // ---- LDS-DMA stream.  Piece j (0, 1) of this wave in a stage half: LDS rows 4 wave + 2 j + (lane >> 5), 16-byte
    // slot lane & 31 of the row; the slot holds the logical chunk whose swizzled position it is.
    unsigned va0, va1, vb0, vb1;
    {
        auto offs = [&](int j, bool is_a) -> unsigned {
            const int kr = wave * 4 + j * 2 + (lane >> 5);
            const int slot = lane & 31;
            int ch = (((slot >> 1) ^ k_swz(kr)) << 1) + (slot & 1) + ((is_a ? m0 : n0) >> 3);
            const int last = ((is_a ? M : N) >> 3) - 1;  // last valid 16-byte chunk of a row
            ch = ch < last ? ch : last;
            return (unsigned)(((long long)kr * (is_a ? ldat : ldbt) + ch * 8) * 2);
        };
        va0 = offs(0, true); va1 = offs(1, true);
        vb0 = offs(0, false); vb1 = offs(1, false);
    }
    const unsigned lds0 = __builtin_amdgcn_readfirstlane(p_lds_addr(smem) + wave * 2048);
    // ring slots: A stages 0-3 at 0 .. 64 KiB, B stages 0-3 at 64 .. 128 KiB
    auto a_slot = [](int t) -> unsigned { return (unsigned)t * 16384u; };
    auto b_slot = [](int t) -> unsigned { return 65536u + (unsigned)t * 16384u; };
    const char* baseA = (const char*)(At + (size_t)kt0 * P_BK * ldat);
    const char* baseB = (const char*)(Bt + (size_t)kt0 * P_BK * ldbt);
    const long long stepA = 64LL * ldat, stepB = 64LL * ldbt;  // 32 rows, in bytes
    int s_ph = 0;  // stream cursor (stage index)
    auto issue = [&](auto STc) {
        constexpr int ST = decltype(STc)::value;  // ring slot of the stage being issued
        if (s_ph < nph) {
            const unsigned da = lds0 + a_slot(ST), db = lds0 + b_slot(ST);
            p_glds2(baseA, va0, va1, da, da + 1024);
            p_glds2(baseB, vb0, vb1, db, db + 1024);
            baseA += stepA;
            baseB += stepB;
        }
        ++s_ph;
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    using I3 = std::integral_constant<int, 3>;

    // ---- fragment addresses: lane (g = l >> 4, q = (l & 15) >> 2, p = l & 3) reads row 8 g + q (+ 4 for the second
    // read) of the stage, 8 bytes at p * 8 of the swizzled 32-byte unit
    const int fg = lane >> 4, fq = (lane & 15) >> 2, fp = lane & 3;
    const int frow = (8 * fg + fq) * 512 + fp * 8, fsw = k_swz(8 * fg + fq);
    unsigned aoff[8], boff[4];
#pragma unroll
    for (int mi = 0; mi < 8; ++mi) aoff[mi] = (unsigned)(frow + (((wr * 8 + mi) ^ fsw) << 5));
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) boff[ni] = (unsigned)(65536 + frow + (((wc * 4 + ni) ^ fsw) << 5));
    auto frag = [&](unsigned off, int imm) -> bf16x8 {
        typedef __attribute__((address_space(3))) s16x4* lp_t;
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp_t)(smem + off + imm));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp_t)(smem + off + imm + 2048));
        typedef __attribute__((ext_vector_type(8))) short s16x8;
        const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        return __builtin_bit_cast(bf16x8, v);
    };

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0, 0, 0, 0};
    bf16x8 a[8], b[4];
    f32x4 accb[2] = {f32x4{0, 0, 0, 0}, f32x4{0, 0, 0, 0}};
    const bool do_cs = COLSUM && (n0 == 0) && colsum != nullptr;
    bf16x8 ones;
#pragma unroll
    for (int j = 0; j < 8; ++j) ones[j] = (__bf16)1.0f;

    // one phase on ring slot ST (the stage it issues, s + 3, lives in slot (ST + 3) & 3)
    auto phase = [&](auto STc, int s) {
        constexpr int ST = decltype(STc)::value;
        // ---------------- LOAD
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) b[ni] = frag(boff[ni], ST * 16384);
#pragma unroll
        for (int mi = 0; mi < 8; ++mi) a[mi] = frag(aoff[mi], ST * 16384);
        __builtin_amdgcn_sched_barrier(0);
        issue(std::integral_constant<int, (ST + 3) % 4>{});
        // stage s + 1 must have landed: all but this wave's pieces of the stages after it may stay in flight
        if (s + 3 < nph) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else if (s + 2 < nph) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        // ---------------- MMA
        __builtin_amdgcn_s_setprio(1);
        if constexpr (COLSUM) {
            if (do_cs) {
                auto cs = [&](const bf16x8& lo, const bf16x8& hi) {
                    accb[0] = P_MFMA(ones, lo, accb[0]);
                    accb[1] = P_MFMA(ones, hi, accb[1]);
                };
                if (wc == 0) cs(a[0], a[4]);
                else if (wc == 1) cs(a[1], a[5]);
                else if (wc == 2) cs(a[2], a[6]);
                else cs(a[3], a[7]);
            }
        }
#pragma unroll
        for (int mi = 0; mi < 8; ++mi)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = P_MFMA(b[ni], a[mi], acc[mi][ni]);
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
    };

    if (total_kt > 0) {
        issue(I0{}); issue(I1{}); issue(I2{});
        // stage 0 landed: the later ones (nph is even: >= 2) may stay in flight
        if (nph >= 3) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");  // nph == 2: stage 1 may
        __builtin_amdgcn_s_barrier();
        if (wr == 1) __builtin_amdgcn_s_barrier();
        int s = 0;
        for (; s + 3 < nph; s += 4) {
            phase(I0{}, s);
            phase(I1{}, s + 1);
            phase(I2{}, s + 2);
            phase(I3{}, s + 3);
        }
        if (s < nph) {  // an odd number of K-tiles: two more stages, slots 0 and 1
            phase(I0{}, s);
            phase(I1{}, s + 1);
        }
        if (wr == 0) __builtin_amdgcn_s_barrier();
    }

    if constexpr (COLSUM) {  // D[n][m] is the same for every n: lanes 0..15 hold m = l, register 0
        if (do_cs && lane < 16) {
#pragma unroll
            for (int qm = 0; qm < 2; ++qm) {
                const int m = m0 + wr * 128 + qm * 64 + wc * 16 + lane;
                if (m < M) {
                    if (splits == 1) colsum[m] = accumulate ? colsum[m] + accb[qm][0] : accb[qm][0];
                    else colsum_part[(size_t)split * M + m] = accb[qm][0];
                }
            }
        }
    }
    const f32x4 zero4 = {0, 0, 0, 0};
    char* stg = smem + 2 * P_BUF + wave * P_STG_WAVE;
    float* out = (splits == 1) ? C : slabs + (size_t)split * M * N;
    const long long ldo = (splits == 1) ? ldc : N;
    const float al = (splits == 1) ? alpha : 1.f;
    const bool accu = (splits == 1) && accumulate;
    if (m0 + P_BM <= M && n0 + P_BN <= N)
        p_store_f32<true, false>(acc, stg, al, zero4, nullptr, 0, accu, out, ldo, m0 + wr * 128,
                                 n0 + wc * 64, M, N, lane);
    else
        p_store_f32<false, false>(acc, stg, al, zero4, nullptr, 0, accu, out, ldo, m0 + wr * 128,
                                  n0 + wc * 64, M, N, lane);
}

// =====================================================================================
// host side
// =====================================================================================
// share of the CUs (percent) a lone product and a paired launch aim to fill
constexpr int TN_FILL_LONE = 75, TN_FILL_PAIR = 75;

bool ssl4gie_internal_tn256_ok(const ssl4gie_gemm_desc* d) {
    if (d->K % P_BK != 0 || d->K < P_BK) return false;
    if (d->conv)
        return ssl4gie_internal_conv_geom_ok(d->conv) && d->conv->C % 8 == 0 &&
               d->N == 9 * d->conv->C && (long long)d->K == conv_rows(d->conv) &&
               (long long)d->K * d->sAk * 2 < (1LL << 32);
    if ((long long)d->K * d->sAk * 2 >= (1LL << 32) || (long long)d->K * d->sBk * 2 >= (1LL << 32))
        return false;  // 32-bit per-lane byte offsets are relative to a per-K-tile base: generous
    // (round 5, measured and not changed: the narrow long-contraction products of ResNet50's layer1 — dW [256, 64],
    // [64, 256], [64, 64], [128, 256] over 802 816 pixels — and the MLP heads' short ones stay on the 128-tile
    // kernel: 98 / 98 / 70 / 121 us there (5.2 TB/s) against 158 / 120 / 108 / 140 us on the partial-tile path
    // here, tools/tn_small_bench.py, profiles/r05_tn_small_routing.log; the "206 us" those launches showed in the
    // round-4 MoCo profile was concurrency with the data-gradient chain, not the kernel)
    return d->K >= 16 * P_BK && (long long)d->M * d->N >= 128 * 128 * 4;
}

// Split-K count of one launch of n products with the same K.  The lone product, the pair and the group share the
// arithmetic; they differ in the share of the CUs they aim to fill, the cap and the group's whole-K rule.
int ssl4gie_internal_tn256_splits(const ssl4gie_gemm_desc* descs, int n, TnSplitPolicy policy) {
    int tiles = 0;
    for (int i = 0; i < n; ++i)
        tiles += ((descs[i].M + P_BM - 1) / P_BM) * ((descs[i].N + P_BN - 1) / P_BN);
    const int nkt = descs[0].K / P_BK;
    const int cus = ssl4gie_internal_compute_cus();
    int fill = 100, cap = 64;
    if (policy == TN_SPLIT_LONE) {
        // These launches run beside the data-gradient chain on a weight-gradient stream, like the pairs (whose fill is
        // 75 % too): MoCo-R50 step 55.5 / 55.7 -> 54.9 / 55.0 ms against 100 % in a same-box A/B
        // (profiles/r04cy_tn_fill1.log), depth and MAE unchanged
        fill = TN_FILL_LONE;
        cap = 256;  // (a single-tile product over a long contraction: one split per CU)
    } else if (policy == TN_SPLIT_PAIR) {
        // on the weight-gradient side stream fewer, longer workgroups mean less slab traffic (measured:
        // profiles/r01w_ab_grid_sizing.log)
        fill = TN_FILL_PAIR;
    } else if (tiles * 10 >= cus * 7) {
        return 1;  // group: >= 70 % of the CUs busy with whole-K tiles: no slabs at all
    }
    int s = (cus * fill / 100 + tiles / 2) / tiles;  // one workgroup per CU
    if (s > nkt / 8) s = nkt / 8;                    // at least 8 K-tiles per split
    if (s < 1) s = 1;
    if (s > cap) s = cap;
    return s;
}

int ssl4gie_internal_tn256_launch(const ssl4gie_gemm_desc* descs, int n, int splits, float* const* slabs_v,
                                  float* const* cs_v, hipStream_t st) {
    if (n < 1 || n > TN_GROUP_MAX) return ARG_ERR;
    const ssl4gie_gemm_desc* d = &descs[0];
    float* slabs = slabs_v[0];
    float* colsum_part = cs_v[0];
    const int tm = (d->M + P_BM - 1) / P_BM, tn = (d->N + P_BN - 1) / P_BN;
    TnExtras sec{};
    bool any_colsum = d->colsum_a != nullptr;
    for (int i = 1; i < n; ++i) {
        const ssl4gie_gemm_desc* d2 = &descs[i];
        if (d2->K != d->K || d2->conv) return ARG_ERR;
        const int tm2 = (d2->M + P_BM - 1) / P_BM, tn2 = (d2->N + P_BN - 1) / P_BN;
        TnSecond& q = sec.p[i - 1];
        q.At = d2->A; q.ldat = d2->sAk; q.Bt = d2->B; q.ldbt = d2->sBk;
        q.C = (float*)d2->C; q.ldc = d2->ldc; q.slabs = slabs_v[i];
        q.M = d2->M; q.N = d2->N; q.tiles_n = tn2; q.ntiles = tm2 * tn2;
        q.colsum = d2->colsum_a; q.colsum_part = cs_v[i];
        q.alpha = d2->alpha; q.accumulate = d2->accumulate; q.tile0 = sec.total_tiles;
        sec.total_tiles += q.ntiles;
        any_colsum = any_colsum || d2->colsum_a != nullptr;
    }
    sec.n = n - 1;
    dim3 grid((tm * tn + sec.total_tiles) * splits);
    ConvK ck{};
    if (d->conv) {
        const int rc = ssl4gie_internal_conv_k(d->conv, &ck);
        if (rc) return rc;
    }
    const int cv = d->conv ? (d->conv->relu ? 2 : 1) : 0;
    // a lone plain product whose tiles M x N does not fill (ResNet's narrow 1x1 weight gradients)
    const bool partial = n == 1 && cv == 0 && (d->M % P_BM != 0 || d->N % P_BN != 0);
    // the arguments both kernels share; `tail`: (ck, sec) for the column-split kernel, (sec) for the k-split one
    auto run = [&](auto k, const auto&... tail) {
        return p_launch<decltype(k)::fn>(grid, st, (const bf16_t*)d->A, d->sAk, (const bf16_t*)d->B, d->sBk,
                                         (float*)d->C, d->ldc, slabs, d->M, d->N, d->K, tn, tm * tn, splits,
                                         d->alpha, d->accumulate, d->colsum_a, colsum_part, tail...);
    };
    // plain operands, no skipped fragment blocks: the k-split kernel
    if (cv == 0 && !partial)
        return any_colsum ? run(P_KERNEL<gemm_bf16_tn256k_kernel<true>>{}, sec)
                          : run(P_KERNEL<gemm_bf16_tn256k_kernel<false>>{}, sec);
    // the column-split kernel, (COLSUM, CONV, PARTIAL): the partial tiles of plain operands, or a patch matrix
    auto column_split = [&](auto cs) {
        constexpr bool CS = decltype(cs)::value;
        if (partial) return run(P_KERNEL<gemm_bf16_tn256_kernel<CS, 0, true>>{}, ck, sec);
        if (cv == 1) return run(P_KERNEL<gemm_bf16_tn256_kernel<CS, 1, false>>{}, ck, sec);
        return run(P_KERNEL<gemm_bf16_tn256_kernel<CS, 2, false>>{}, ck, sec);
    };
    return any_colsum ? column_split(std::true_type{}) : column_split(std::false_type{});
}
