/* libssl4gie_hip.so — C ABI of the MI355X (gfx950) compute path for the SSL4GIE hot path.
 *
 * The reference (ESandML/SSL4GIE) is pure Python/PyTorch and has no native boundary of its own:
 * its hot path is the ATen ops reached from timm `Block`/`PatchEmbed` (un-vendored) and
 * `Models/mae/models_mae.py`, `Models/models.py`.  Every entry point below names the reference
 * call site(s) whose arithmetic it replaces.  Conventions:
 *   - plain C types only; device pointers + explicit sizes/strides + a HIP stream (`void*`);
 *   - no per-call allocation, nothing freed, no host synchronisation; workspaces are
 *     caller-allocated and sized by the matching `*_workspace_bytes()` query.  Three objects are
 *     created once per device on first use and live as long as the library: the 256-byte zero page
 *     of the implicit convolution, the weight-gradient side stream + its events
 *     (ssl4gie_set_wgrad_stream), and — opt-in — the launch profiler (ssl4gie_prof_*); the direct
 *     all-reduce owns one IPC exchange region per handle (ssl4gie_allreduce_direct_init / _destroy);
 *   - returns 0 on success, SSL4GIE_EARG (1000) for an invalid argument, otherwise a hipError_t;
 *   - callable from any host thread; the only mutable process-wide settings are the execution
 *     options ssl4gie_set_wgrad_stream / ssl4gie_set_compute_cus and the profiler;
 *   - ssl4gie_abi_version() = 13 (revision 13 LOST ssl4gie_adamw_arena_lp, ssl4gie_adamw_arena_range and ssl4gie_adamw_arena_range_ctl and CHANGED the
 *     signature of ssl4gie_adamw_arena, which now is the one AdamW step: a range of the arena, the optional bf16 copy, and the step count either from the
 *     host (ctl == NULL) or from a device counter behind the control block (ctl != NULL) — the same two kernels and launches as before; ssl4gie_sgd_arena
 *     is unchanged (its source moved from probe_ops.hip to optim_ops.hip); 12: ssl4gie_view_sample_u8, after it ssl4gie_color_augment{_workspace_bytes,}, and after those ssl4gie_color_augment_ft / ssl4gie_paired_warp, joined revision 12
 *     without a new number: added symbols, nothing existing changed, so a caller built against the earlier 12 runs unchanged; the evaluation
 *     metrics ssl4gie_seg_{counts,scores} / ssl4gie_confusion_{update,scores} / ssl4gie_lower_median_{workspace_bytes,f32} / ssl4gie_depth_eval{_workspace_bytes,}
 *     joined it the same way, and so did the detection input entry points ssl4gie_det_color{_workspace_bytes,} / ssl4gie_det_geometry / ssl4gie_det_boxes and the
 *     detection metric ssl4gie_det_map_{workspace_bytes,match,order,accumulate}, and the Faster R-CNN head entry points ssl4gie_nms_{workspace_bytes,segments} /
 *     ssl4gie_rpn_decode / ssl4gie_roi_decode / ssl4gie_roi_align_{fwd,bwd}, and the fine-tuning recipe's ssl4gie_block_{dp_workspace_bytes,fwd_dp,bwd_dp} /
 *     ssl4gie_drop_path_{add,scale_cast} / ssl4gie_mixup{,_target} / ssl4gie_soft_cross_entropy{_workspace_bytes,}, and its loader's ssl4gie_quantize_u8 / ssl4gie_randaug_layer{_workspace_bytes,} /
 *     ssl4gie_normalize_erase_u8, and the linear probe's ssl4gie_topk_{workspace_bytes,update} / ssl4gie_sgd_arena; revision 12 later LOST ssl4gie_conv3x3_direct_{fwd,wgrad}_affine,
 *     ssl4gie_block_wgrad_descs, ssl4gie_wgrad_group and the SSL4GIE_BWD_DEFER_WGRAD flag of ssl4gie_block_bwd with the two opt-in paths of the Python
 *     package that were their only callers (measured null or slower, profiles/HISTORY.md appendix 4) — the number is kept because the suite asserts 12
 *     in nine places; a caller of those four entry points fails at symbol resolution instead; 11: before the sixteen BatchNorm entry points that had grown one per fusion (ssl4gie_bn_fwd / _fwd_partials / _fwd_partials_bits /
 *     _coef_partials / _coef_stats / _apply_bits, _stats / _stats_partials, _bwd / _bwd_xmask / _bwd_bits, _bwd_reduce / _reduce_xmask / _reduce_bits,
 *     _bwd_apply / _apply_xmask) were REPLACED by five with a source and a mask kind — the same launches, new signatures; 10: before the diagnostics entry point that read the 256x256 NT kernel's in-kernel
 *     time stamps was REMOVED with the debug build of the library — the one removal in this history; 9: before ssl4gie_infonce_{workspace_bytes,loss} / ssl4gie_cross_entropy{_workspace_bytes,} /
 *     ssl4gie_bt_loss{_workspace_bytes,,_grad} existed — additions only; 8: before ssl4gie_grad_norm_{workspace_bytes,arena} / ssl4gie_grad_scale_arena /
 *     ssl4gie_adamw_arena_range_ctl existed — additions only; 7: before ssl4gie_stem3x3_{tiles,fwd,wgrad_workspace_bytes,wgrad} existed — additions only; 6: before ssl4gie_bn_coef_stats / ssl4gie_bn_apply_bits / ssl4gie_bn_bwd_reduce_bits existed — additions only; 5: before SSL4GIE_PROF_KINDS grew from 5 to 7 — the profiler's arrays; 1: before ssl4gie_gemm_desc gained `colsum_a` / `conv`; 2: before
 *     ssl4gie_block_bwd's `accumulate` became a flag word and the grouped / deferred weight-gradient
 *     entry points existed; 3: before the direct transport's error word / time-out / all-gather,
 *     ssl4gie_bn_combine_stats and that time-stamp reader existed — additions only; 4: before
 *     ssl4gie_gemm_desc gained `scale` / `relu` (appended; SSL4GIE_EPI_AFFINE_AUX_RELU and the
 *     statistics-only product with C == NULL) and ssl4gie_bn_bwd_xmask / ssl4gie_bn_coef_partials / ssl4gie_bn_maxpool3x3s2_fwd /
 *     ssl4gie_conv3x3_direct_{fwd,wgrad}_affine / ssl4gie_bn_fwd_partials_bits / ssl4gie_bn_bwd_bits /
 *     ssl4gie_bn_bwd_{reduce,apply}_xmask / ssl4gie_conv3x3_weight_pack_batch existed);
 *   - "lp" tensors are the MFMA operand type: SSL4GIE_BF16 for the production path,
 *     SSL4GIE_F32 for the exact-fp32 parity path (f32 MFMA, bit-level fp32 FMA chains).
 */
#ifndef SSL4GIE_HIP_H
#define SSL4GIE_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SSL4GIE_F32 0
#define SSL4GIE_BF16 1
#define SSL4GIE_EARG 1000
#define SSL4GIE_EPEER 1001 /* direct all-reduce: a peer did not arrive in time (sticky, see _error) */

int ssl4gie_abi_version(void);

/* ---------------------------------------------------------------- LayerNorm (eps=1e-6)
 * replaces nn.LayerNorm at models_mae.py:227 / models.py:384,498 inside timm Block
 * (norm1/norm2) and the final `norm` (models_mae.py:168).  x fp32 [rows, cols]; y in
 * y_dtype; mean/rstd fp32 [rows] saved for backward (may be NULL). */
int ssl4gie_layernorm_fwd(const float* x, const float* gamma, const float* beta, void* y,
                          int y_dtype, float* mean, float* rstd, int rows, int cols, float eps,
                          void* stream);
size_t ssl4gie_layernorm_bwd_workspace_bytes(int rows, int cols);
/* dx = (dres ? dres : 0) + LN'(dy); dx_lp (optional) is the same value in lp_dtype (feeds the
 * next backward GEMM); dgamma/dbeta overwritten or accumulated. */
int ssl4gie_layernorm_bwd(const void* dy, int dy_dtype, const float* x, const float* gamma,
                          const float* mean, const float* rstd, const float* dres, float* dx,
                          void* dx_lp, int lp_dtype, float* dgamma, float* dbeta, int accumulate,
                          float* workspace, int rows, int cols, void* stream);

/* column sums of x[rows, cols] (row stride ld) -> out[cols]: bias gradients of nn.Linear */
size_t ssl4gie_colsum_workspace_bytes(int rows, int cols);
int ssl4gie_colsum(const void* x, int dtype, float* out, int accumulate, float* workspace,
                   int rows, int cols, long long ld, void* stream);

/* ---------------------------------------------------------------- GEMM with fused epilogues
 * replaces nn.Linear fwd/bwd (timm Attention.qkv/proj, Mlp.fc1/fc2; decoder_embed/decoder_pred
 * models_mae.py:47,59), the patch-embed conv lowered to a GEMM (models_mae.py:33), and the
 * batched QK^T / PV products of the fp32 parity attention.
 *   C[b](m,n) = epilogue( alpha * sum_k A[b](m,k) * B[b](k,n) )
 * A(m,k) at A + b1*sAb1 + b2*sAb2 + m*sAm + k*sAk (element strides), likewise B(k,n);
 * C row-major with row stride ldc.  Fast MFMA-bf16 paths: "NT" (sAk==1 && sBk==1, K%64==0)
 * and "TN" (sAm==1 && sBn==1, split-K through the workspace); anything else takes the generic
 * f32-MFMA kernel. */
enum {
    SSL4GIE_EPI_NONE = 0,          /* C = alpha*acc                       */
    SSL4GIE_EPI_BIAS = 1,          /* C = acc + bias[n]                   */
    SSL4GIE_EPI_BIAS_GELU = 2,     /* C = u = acc + bias[n]; out2 = gelu(u) (exact erf) */
    SSL4GIE_EPI_BIAS_RESIDUAL = 3, /* C = acc + bias[n] + residual[m,n] (fp32 residual) */
    SSL4GIE_EPI_DGELU = 4,         /* C = acc * gelu'(aux[m,n])           */
    /* the pair the block executor uses: the forward stores gelu'(u) instead of u, so that the
     * backward epilogue is one multiply (no transcendental work on the data-gradient GEMM) */
    SSL4GIE_EPI_BIAS_GELU_GRAD = 5, /* u = acc + bias[n]; C = gelu'(u); out2 = gelu(u) */
    SSL4GIE_EPI_MUL_AUX = 6,        /* C = acc * aux[m,n]                  */
    SSL4GIE_EPI_RELU_MASK_AUX = 7,  /* C = aux[m,n] > 0 ? acc : 0: gradient through the ReLU in front of a
                                       convolution (aux = the convolution's input); implicit-conv NT
                                       products with bf16 output only */
    SSL4GIE_EPI_ADD_AUX = 8,        /* C = acc + aux[m,n]: a second gradient contribution of the same
                                       tensor (residual branch) joined in the data-gradient GEMM;
                                       256x256 NT kernel, bf16 output only */
    SSL4GIE_EPI_AFFINE_AUX_RELU = 9 /* C = act(acc * scale[n] + bias[n] (+ aux[m,n])), act = ReLU if `relu`:
                                       the training-mode BatchNorm after a 1x1 convolution (scale = rstd gamma,
                                       bias = beta - mean scale, from a statistics-only first product: colstats
                                       with C == NULL), the bottleneck's residual add and ReLU, applied to the
                                       fp32 accumulators — the raw convolution output is never written or re-read
                                       (torchvision Bottleneck conv3 / bn3 / downsample under torch.no_grad();
                                       256x256 NT kernel, bf16 output only; aux may be NULL) */
};
/* Implicit patch-matrix operand of a 3x3 / pad-1 convolution over a channels-last bf16 map
 * x [B, H, W, C] (ssl4gie_gemm_desc::conv).  The patch matrix
 *     P[(b, oy, ox), (dy*3 + dx)*C + c] = act(x[b, oy*s + dy - 1, ox*s + dx - 1, c])   (0 outside)
 * of ssl4gie_im2col3x3 is never materialised: the 256x256 kernels gather its K-tiles straight
 * from the map with per-lane LDS-DMA addresses (out-of-image taps read a zero page), act = ReLU
 * applied to the MFMA fragments when `relu`.  Replaces the cuDNN implicit-GEMM convolutions
 * behind nn.Conv2d(k=3, p=1) in Models/DPT_decoder.py:212-233,397-447,469-478 and torchvision
 * Bottleneck.conv2.
 *   NT (forward / stride-1 data gradient):  A := P, d->A = x, M = B*Ho*Wo, K = 9*C, C % 64 == 0;
 *       sAm / sAk are ignored.
 *   TN (weight gradient dW = dY^T P):       B := P, d->B = x, K = B*Ho*Wo (% 64 == 0), N = 9*C,
 *       C % 8 == 0; sBk / sBn are ignored.
 * Limits: bf16 operands, stride in {1, 2}, map smaller than 2 GiB, Wo >= 2.  A descriptor that
 * carries `conv` and does not meet them is rejected with SSL4GIE_EARG (no fallback inside). */
typedef struct ssl4gie_conv3x3_geom {
    int B, H, W, C;
    int stride;
    int relu;
} ssl4gie_conv3x3_geom;

typedef struct ssl4gie_gemm_desc {
    int M, N, K;
    int batch1, batch2; /* >=1 */
    const void* A;
    long long sAm, sAk, sAb1, sAb2;
    const void* B;
    long long sBk, sBn, sBb1, sBb2;
    void* C;
    long long ldc, sCb1, sCb2;
    int dtype_ab; /* SSL4GIE_F32 | SSL4GIE_BF16 */
    int dtype_c;  /* type of C, out2 and aux */
    float alpha;
    int epilogue;
    const float* bias;     /* [N] */
    const float* residual; /* fp32 [M, N], row stride ldr */
    long long ldr;
    const void* aux; /* [M, N] row stride ldc, dtype_c */
    void* out2;      /* [M, N] row stride ldc, dtype_c */
    int accumulate;  /* C += (EPI_NONE only) */
    /* optional [M] fp32: colsum_a[m] (+)= sum_k A(m,k) with the same `accumulate` flag (alpha not
     * applied).  The bias gradient of nn.Linear riding on its weight-gradient product
     * dW = dY^T X (A = dY^T): fused into the 256x256 TN kernel (one extra MFMA against a ones
     * fragment per A fragment), a separate column-sum pass on the other paths.  Needs sAm == 1. */
    float* colsum_a;
    /* optional: the K-major operand (A of an NT product, B of a TN product) is the implicit 3x3
     * patch matrix of this map instead of a matrix in memory (see ssl4gie_conv3x3_geom) */
    const ssl4gie_conv3x3_geom* conv;
    /* optional fp32 [ceil(M / 128)][2][N]: per 128-row block, the column sums ([0]) and sums of
     * squares ([1]) of the STORED outputs — the batch statistics of the BatchNorm that follows a
     * convolution, produced by the GEMM's epilogue (see ssl4gie_bn_fwd, FROM_PARTIALS).  NT products with
     * bf16 C, EPI_NONE, no accumulate, N % 8 == 0 only; anything else is SSL4GIE_EARG.  With C == NULL the
     * product only produces these statistics (of the values it WOULD store, bf16-rounded): nothing is written
     * to C — the first half of the BatchNorm-fused 1x1 convolution (SSL4GIE_EPI_AFFINE_AUX_RELU). */
    float* colstats;
    const float* scale; /* [N], SSL4GIE_EPI_AFFINE_AUX_RELU only */
    int relu;           /* SSL4GIE_EPI_AFFINE_AUX_RELU only */
} ssl4gie_gemm_desc;
size_t ssl4gie_gemm_workspace_bytes(const ssl4gie_gemm_desc* d);
int ssl4gie_gemm(const ssl4gie_gemm_desc* d, void* workspace, size_t workspace_bytes,
                 void* stream);
/* Two weight-gradient (TN) products with the same contraction length K in one launch: they share
 * the one-workgroup-per-CU grid, so each needs half the split-K slabs (and half the reduction
 * traffic) it would need alone.  Descriptors as for ssl4gie_gemm; pairs that do not qualify run as
 * two ssl4gie_gemm calls.  Used for (dW_fc2, dW_fc1) and (dW_proj, dW_qkv) of a transformer block. */
size_t ssl4gie_gemm_tn_pair_workspace_bytes(const ssl4gie_gemm_desc* a, const ssl4gie_gemm_desc* b);
int ssl4gie_gemm_tn_pair(const ssl4gie_gemm_desc* a, const ssl4gie_gemm_desc* b, void* workspace,
                         size_t workspace_bytes, void* stream);
/* n (1..16) weight-gradient (TN) products with the same contraction length K in ONE launch.  With
 * enough output tiles in the group (>= 70 % of the CUs) every workgroup runs a whole-K tile and
 * writes C directly: no split-K slabs, no slab reduction — the 8 + 8 products of two encoder blocks
 * (216 tiles) or four decoder blocks (192 tiles) of the MAE step.  Smaller groups split K like the
 * pair.  `descs` is an array of n descriptors (alpha / accumulate / colsum_a per product); products
 * that do not qualify run as n ssl4gie_gemm calls.  Replaces the per-layer autograd weight-gradient
 * GEMMs of nn.Linear (Models/mae/models_mae.py:39-41,53-55 via timm Block). */
size_t ssl4gie_gemm_tn_group_workspace_bytes(const ssl4gie_gemm_desc* descs, int n);
int ssl4gie_gemm_tn_group(const ssl4gie_gemm_desc* descs, int n, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- attention
 * replaces timm Attention.forward == Models/models.py:195-209 minus windowing:
 * softmax(q k^T * hd^-1/2) v on the packed qkv activation [B, N, 3, H, hd] (row = token).
 * out [B, N, H*hd]; lse fp32 [B, H, N] (saved for backward).  bf16 path is one fused kernel
 * (whole K/V of a head staged in LDS, softmax in registers, no N x N materialisation); the
 * f32 parity path materialises scores in the caller-provided workspace. */
size_t ssl4gie_attn_workspace_bytes(int dtype, int B, int N, int H, int hd);
int ssl4gie_attn_fwd(const void* qkv, void* out, float* lse, int dtype, int B, int N, int H,
                     int hd, void* workspace, void* stream);
int ssl4gie_attn_bwd(const void* qkv, const void* out, const void* dout, const float* lse,
                     void* dqkv, int dtype, int B, int N, int H, int hd, void* workspace,
                     void* stream);

/* ---------------------------------------------------------------- casts
 * fp32 master weights -> MFMA operand copies (bf16), plain and transposed ([R,C] -> [C,R]). */
int ssl4gie_cast(const float* src, void* dst, int dst_dtype, long long n, void* stream);
int ssl4gie_cast_transpose(const float* src, void* dst, int dst_dtype, int rows, int cols,
                           void* stream);
/* bf16 transposed copies of S matrices of one fp32 arena in ONE launch (the per-step refresh of the
 * pre-transposed weight operands).  Device tables: mat_off [S] int64 element offsets (the same in src
 * and dst), mat_rows / mat_cols [S], tile_start [S+1] = running count of 64 x 64 tiles per matrix
 * (ceil(rows/64) * ceil(cols/64)), total_tiles = tile_start[S] (passed by value: no device read).
 * dst[off + c * rows + r] = bf16(src[off + r * cols + c]). */
int ssl4gie_cast_transpose_batch(const float* src, void* dst, const long long* mat_off,
                                 const int* mat_rows, const int* mat_cols, const int* tile_start,
                                 int S, int total_tiles, void* stream);
/* out = a + b (b may be NULL), optionally also written as an operand-type copy out_lp:
 * plumbing of the fp32 residual-gradient stream (tap gradients, models.py:450-454). n % 4 == 0 */
int ssl4gie_add_cast(const float* a, const float* b, float* out, void* out_lp, int lp_dtype,
                     long long n, void* stream);

/* ---------------------------------------------------------------- MAE glue
 * random_masking (models_mae.py:123-148): stable argsort of fp32 noise [B, L] ->
 * ids_shuffle / ids_restore (int64, bit-exact) and mask (fp32; 1 = removed). */
int ssl4gie_mask_argsort(const float* noise, long long* ids_shuffle, long long* ids_restore,
                         float* mask, int B, int L, int len_keep, void* stream);
/* im2col of non-overlapping p x p patches (PatchEmbed conv k=s=p as a GEMM, models_mae.py:152):
 * out[b*nsel + j, c*p*p + py*p + px] = img[b, c, gy*p+py, gx*p+px], patch = ids ? ids[b, j] : j.
 * order==1 emits the 'nhwpqc' layout of patchify (models_mae.py:95-107) instead. */
int ssl4gie_patch_gather(const float* img, const long long* ids, void* out, int out_dtype,
                         int B, int C, int H, int W, int p, int nsel, long long ids_stride,
                         int order, void* stream);
/* encoder input assembly (models_mae.py:155-163 / models.py:445-448):
 * x[b,0,:] = cls + pos[0]; x[b,1+j,:] = y[b*nsel+j,:] + pos[1 + (ids ? ids[b,j] : j)] */
int ssl4gie_tokens_assemble(const void* y, int y_dtype, const float* cls, const float* pos,
                            const long long* ids, long long ids_stride, float* x, int B,
                            int nsel, int D, void* stream);
/* backward of the above: dy[b*nsel+j] = dx[b,1+j]; dcls = sum_b dx[b,0] */
int ssl4gie_tokens_assemble_bwd(const float* dx, void* dy, int dy_dtype, float* dcls,
                                int accumulate, int B, int nsel, int D, void* stream);
/* decoder input assembly (models_mae.py:177-183): xd[b,0] = y[b,0] + dpos[0];
 * xd[b,1+i] = (r = ids_restore[b,i]) < nkeep ? y[b,1+r] : mask_token, + dpos[1+i] */
int ssl4gie_decoder_assemble(const void* y, int y_dtype, const float* mask_token,
                             const float* dpos, const long long* ids_restore, float* xd, int B,
                             int L, int nkeep, int D, void* stream);
size_t ssl4gie_decoder_assemble_bwd_workspace_bytes(int B, int L, int D);
/* dy[b,0] = dxd[b,0]; dy[b,1+j] = dxd[b, 1+ids_shuffle[b,j]] (j<nkeep);
 * dmask_token = sum over removed positions of dxd */
int ssl4gie_decoder_assemble_bwd(const float* dxd, const long long* ids_shuffle, void* dy,
                                 int dy_dtype, float* dmask_token, int accumulate,
                                 float* workspace, int B, int L, int nkeep, int D, void* stream);
/* forward_loss (models_mae.py:198-214) and its gradient.  pred fp32 [B, has_cls+L, P] (with
 * has_cls=1 row 0 of each sample is the cls prediction and is ignored: decoder_pred runs on all
 * 1+L tokens, models_mae.py:191-194), img fp32 NCHW, mask [B, L] (1 = removed).
 *   per_patch (optional) [B, L] = mask * mean_k (pred - target)^2   (host sums / mask.sum())
 *   dpred (optional, same shape as pred) = gscale_host * gpp[b,l] * mask * 2 (pred-target) / P, cls rows
 *   zeroed; gpp [B, L] is the upstream gradient of per_patch (NULL = 1). */
int ssl4gie_mae_loss(const float* pred, const float* img, const float* mask, float* per_patch,
                     float* dpred, const float* gpp, float gscale_host, int norm_pix,
                     int has_cls, int B, int C, int H, int W, int p, void* stream);

/* ---------------------------------------------------------------- transformer-block executor
 * One timm Block: x += proj(attn(norm1(x))); x += fc2(gelu(fc1(norm2(x)))).
 * Residual stream fp32; MFMA operands in `dtype`.  `w*` are operand-type copies of the weights
 * ([out,in] row-major) and `w*_t` their transposes ([in,out]) used by the data-gradient GEMMs.
 * Saved activations live in caller-owned buffers (`ssl4gie_block_act`). */
typedef struct ssl4gie_block_weights {
    const float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
    const float *bqkv, *bproj, *bfc1, *bfc2;
    const void *wqkv, *wproj, *wfc1, *wfc2;         /* [3D,D] [D,D] [F,D] [D,F] */
    const void *wqkv_t, *wproj_t, *wfc1_t, *wfc2_t; /* transposes (backward only) */
} ssl4gie_block_weights;
typedef struct ssl4gie_block_grads { /* fp32, same shapes as the fp32 master parameters */
    float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
    float *bqkv, *bproj, *bfc1, *bfc2;
    float *wqkv, *wproj, *wfc1, *wfc2;
} ssl4gie_block_grads;
typedef struct ssl4gie_block_act { /* per-block saved activations; T = tokens = B*N */
    float *mean1, *rstd1, *mean2, *rstd2; /* [T] */
    void* h1;                             /* [T, D]  norm1 out     */
    void* qkv;                            /* [T, 3D]               */
    void* attn;                           /* [T, D]  attention out */
    float* lse;                           /* [B, H, N]             */
    float* xmid;                          /* [T, D]  fp32          */
    void* h2;                             /* [T, D]  norm2 out     */
    void* u;                              /* [T, F]  gelu'(fc1 pre-activation) */
    void* g;                              /* [T, F]  gelu(u)       */
} ssl4gie_block_act;
typedef struct ssl4gie_block_dims {
    int B, N, D, H, F; /* F = mlp hidden */
    int dtype;
    float eps;
} ssl4gie_block_dims;
size_t ssl4gie_block_workspace_bytes(const ssl4gie_block_dims* d);
/* x_in fp32 [T, D] -> x_out fp32 [T, D] (may alias nothing) */
int ssl4gie_block_fwd(const ssl4gie_block_dims* d, const ssl4gie_block_weights* w,
                      const ssl4gie_block_act* a, const float* x_in, float* x_out,
                      void* workspace, void* stream);
/* dx_out fp32 (+ dx_out_lp, its operand-type copy; may be NULL in f32 mode) -> dx_in fp32 and
 * dx_in_lp; parameter grads overwritten or accumulated.  `accumulate` is a flag word:
 * SSL4GIE_BWD_ACCUMULATE (1), SSL4GIE_BWD_NO_JOIN (4) and SSL4GIE_BWD_SLOT(s); bit 1 is unused. */
#define SSL4GIE_BWD_ACCUMULATE 1
/* SSL4GIE_BWD_NO_JOIN | SSL4GIE_BWD_SLOT(s), s in 0..3: `stream` does NOT wait for the block's weight-gradient
 * products at the end of the call (the default join makes the next block's first data-gradient GEMM wait for
 * this block's last weight gradient: 20 stalls per MAE step).  Instead their completion is recorded under slot s
 * on the side stream: `workspace`, dx_out_lp and the gradient targets must stay untouched until
 * ssl4gie_wgrad_wait(s, stream) has been called — the caller alternates two workspaces and slots. */
#define SSL4GIE_BWD_NO_JOIN 4
#define SSL4GIE_BWD_SLOT(s) (((s) & 3) << 4)
int ssl4gie_block_bwd(const ssl4gie_block_dims* d, const ssl4gie_block_weights* w,
                      const ssl4gie_block_act* a, const ssl4gie_block_grads* g,
                      const float* x_in, const float* dx_out, const void* dx_out_lp,
                      float* dx_in, void* dx_in_lp, int accumulate, void* workspace,
                      void* stream);
/* Stochastic depth (timm's drop_path with scale_by_keep, main_finetune.py:57; joined ABI 12 as additions).
 * s_attn / s_mlp: fp32 [B] device tables of the per-sample factor, 0 for a dropped sample and 1 / keep_prob for a
 * kept one, or NULL for a branch that runs exactly as in ssl4gie_block_fwd / _bwd (same launches):
 *   x_mid = x_in  + s_attn[b] (proj(attn(ln1 x_in)) + b_proj)
 *   x_out = x_mid + s_mlp[b]  (fc2(gelu(fc1(ln2 x_mid))) + b_fc2)
 * The scaled add runs beside the GEMM (product + bias into an fp32 scratch slot, then ssl4gie_drop_path_add), the
 * backward feeds each branch the operand-type copy s[b] dx (ssl4gie_drop_path_scale_cast) and both LayerNorm
 * backward passes keep the unscaled residual gradient.  A dropped sample's rows are copies: x_out[b] == x_in[b] and
 * dx_in[b] == dx_out[b] bit for bit when both branches drop it.  `workspace` is sized by
 * ssl4gie_block_dp_workspace_bytes (the plain layout plus three [T, D] slots) whether or not a table is NULL; with
 * s_mlp given dx_out_lp is not read and may be NULL. */
size_t ssl4gie_block_dp_workspace_bytes(const ssl4gie_block_dims* d);
int ssl4gie_block_fwd_dp(const ssl4gie_block_dims* d, const ssl4gie_block_weights* w,
                         const ssl4gie_block_act* a, const float* x_in, float* x_out,
                         const float* s_attn, const float* s_mlp, void* workspace, void* stream);
int ssl4gie_block_bwd_dp(const ssl4gie_block_dims* d, const ssl4gie_block_weights* w,
                         const ssl4gie_block_act* a, const ssl4gie_block_grads* g,
                         const float* x_in, const float* dx_out, const void* dx_out_lp,
                         float* dx_in, void* dx_in_lp, const float* s_attn, const float* s_mlp,
                         int accumulate, void* workspace, void* stream);
/* the two element-wise kernels behind them; res / t / dx / out fp32 [B, per_sample] (16-byte aligned, per_sample % 4
 * == 0), s fp32 [B]:  out = s[b] != 0 ? res + s[b] t : res  (t is not read for a dropped sample);
 * out (out_dtype) = s[b] != 0 ? cast(s[b] dx) : 0  (dx is not read for a dropped sample). */
int ssl4gie_drop_path_add(const float* res, const float* t, const float* s, float* out, int B,
                          long long per_sample, void* stream);
int ssl4gie_drop_path_scale_cast(const float* dx, const float* s, void* out, int out_dtype, int B,
                                 long long per_sample, void* stream);
/* Mixup / CutMix of timm.data.Mixup (main_finetune.py:221-226) on a resident fp32 batch x [B, C, H, W], IN PLACE, one
 * launch.  Sample i is mixed with sample B - 1 - i (an odd B's middle sample with itself); per-sample device tables
 * lam fp32 [B], box int32 [B, 4] = (y0, y1, x0, x1), use_cutmix uint8 [B]:
 *   use_cutmix[i] == 0:  x_i = x_i lam_i + x_j (1 - lam_i), each product rounded to fp32, one addition (bit-equal to
 *                        x.mul(lam).add(x.flip(0).mul(1 - lam)));
 *   use_cutmix[i] != 0:  x_i[:, y0:y1, x0:x1] = x_j[:, y0:y1, x0:x1].
 * Both originals are read before either result is written.  A box is only compared against coordinates, never used
 * in an address; one that is not inside the image (or a NaN lam) turns its sample into NaN.
 * ssl4gie_mixup_target: out fp32 [B, C], row i = onehot(target_i) lam_i + onehot(target_{B-1-i}) (1 - lam_i) with
 * one-hot values on / off; a label outside [0, C) gives a NaN row and is never an index. */
int ssl4gie_mixup(float* x, const float* lam, const int* box, const unsigned char* use_cutmix, int B, int C,
                  int H, int W, void* stream);
int ssl4gie_mixup_target(const long long* target, const float* lam, float* out, int B, int C,
                         float on, float off, void* stream);
/* The four weight-gradient products of ssl4gie_block_bwd are enqueued on a library-owned
 * non-blocking side stream (one per device, created on first use) and ordered against `stream`
 * with events only: each waits for its dY producer, and `stream` waits for the last of them
 * before any later work — to the caller the call still behaves as if everything ran on `stream`.
 * on = 0 folds them back onto `stream` (also: environment SSL4GIE_WGRAD_STREAM=0); bench.py does
 * that while it measures per-kernel durations. */
int ssl4gie_set_wgrad_stream(int on);
/* makes `stream` wait for the weight gradients of the latest ssl4gie_block_bwd(SSL4GIE_BWD_NO_JOIN | SSL4GIE_BWD_SLOT(slot));
 * to be issued before anything reads those gradients or rewrites their operands (block workspace, activations). */
int ssl4gie_wgrad_wait(int slot, void* stream);
/* Number of CUs the persistent / one-workgroup-per-CU GEMM grids are sized for (8..256, default 240:
 * the weight-gradient side stream shares the chip; environment SSL4GIE_COMPUTE_CUS).  The 256x256 kernels hold all 160 KiB of a CU's LDS, so an RCCL
 * kernel running beside them needs CUs of its own: ssl4gie_amd.parallel reserves a few in
 * data-parallel runs (and caps RCCL's channel count to match) so that no GEMM workgroup has to
 * wait for a second wave behind a busy CU. */
int ssl4gie_set_compute_cus(int n);

/* ---------------------------------------------------------------- DPT decoder glue (channels-last)
 * Replaces the torch ops around the convolutions of Models/DPT_decoder.py (depth variant): the
 * maps are [B, H, W, C] in the operand type (`dtype`), C % 8 == 0 (bf16) / % 4 == 0 (fp32).  With
 * this layout Conv2d(k=1) and ConvTranspose2d(k=s) are token-major ssl4gie_gemm calls and
 * Conv2d(k=3, pad=1) is ssl4gie_gemm over the patch matrix below.
 *
 * im2col3x3: cols[(b,oy,ox), (dy*3+dx)*C + c] = act(x[b, oy*s+dy-1, ox*s+dx-1, c]) (0 outside),
 *   act = ReLU if `relu` (ResidualConvUnit_custom.forward :225-229 activates the conv INPUT);
 *   row stride ld >= 9C, columns [9C, ld) zero-filled; s in {1, 2} (act_postprocess42.1 :397-403).
 * col2im3x3: gather-form transpose (data gradient of the strided conv). */
/* Operand images of an nn.Conv2d(k = 3) weight [Cout][Cin][3][3] (fp32 parameter) in one launch, cast included:
 * mode 0 out[co][tap Cin + ci] (row stride ld >= 9 Cin: forward / weight-gradient layout), mode 1
 * out[ci][(8 - tap) Cout + co] (ld >= 9 Cout: the flipped kernel of the stride-1 data gradient), mode 2
 * out[tap Cin + ci][co] (ld >= 9 Cin rows: transpose of mode 0); padding is written as zeros.  What cuDNN's
 * filter transforms do behind the reference's nn.Conv2d calls (Models/DPT_decoder.py:212-233,397-447,469-478;
 * torchvision Bottleneck.conv2), once per optimizer step. */
int ssl4gie_conv3x3_weight_pack(const float* w, void* out, int dtype, int Cout, int Cin, int mode, int ld,
                                void* stream);
/* The same for n weights in ONE launch (arrays of n pointers / geometries; all outputs of type `dtype`): every 3x3
 * convolution of a model re-packs its operand images after each optimizer step. */
int ssl4gie_conv3x3_weight_pack_batch(const void* const* w, void* const* out, const int* Cout, const int* Cin,
                                      const int* mode, const int* ld, int n, int dtype, void* stream);
/* ... and back for the weight gradient: dw2 [Cout][ld] fp32 with columns (tap, ci) -> (+)= dW [Cout][Cin][3][3] */
int ssl4gie_conv3x3_wgrad_unpack(const float* dw2, float* dw, int Cout, int Cin, int ld, int accumulate,
                                 void* stream);
int ssl4gie_im2col3x3(const void* x, void* cols, int dtype, int B, int H, int W, int C, int stride,
                      int relu, long long ld, void* stream);
int ssl4gie_col2im3x3(const void* dcols, void* dx, int dtype, int B, int H, int W, int C,
                      int stride, long long ld, void* stream);
/* Direct 3x3 convolution, stride 1, pad 1, bf16, for NARROW channel counts — the DPT output head's
 * nn.Conv2d(128, 32, 3, 1, 1) (output_conv.2, DPT_decoder.py:473-478) and its gradients, where the
 * gathered 256x256 GEMM tiles would be 7/8 padding.  x [B,H,W,Cin], w2 [Cout, 9*Cin] (the layout
 * of the implicit-GEMM path: taps row-major, channels innermost), y [B,H,W,Cout]:
 *     y = conv(relu_in ? relu(x) : x, w2) (+ bias[Cout] fp32)  (then y = relu_mask > 0 ? y : 0, with
 *     relu_mask [B,H,W,Cout] bf16 — the data gradient of a convolution behind a ReLU)
 * colstats (optional, not together with relu_mask): fp32 [ssl4gie_conv3x3_direct_tiles(B,H,W)][2][Cout],
 * per 8 x 32 pixel tile the column sums ([0]) and sums of squares ([1]) of the stored y — the
 * partial statistics ssl4gie_bn_fwd (FROM_PARTIALS) / ssl4gie_bn_stats take (as
 * ssl4gie_gemm_desc.colstats, with one partial per tile instead of per 128 rows).
 * The data gradient is the same call on dy with w2 := weight.flip(2,3) as [Cin, 9*Cout].
 * _ok(): Cin % 32 == 0 and Cout % 8 == 0 (any H, W); otherwise the calls return SSL4GIE_EARG.
 * Meant for Cout <= 128 or Cin == 32 (at 256 -> 256 it merely ties the gathered GEMM). */
int ssl4gie_conv3x3_direct_ok(int B, int H, int W, int Cin, int Cout);
int ssl4gie_conv3x3_direct_tiles(int B, int H, int W);
int ssl4gie_conv3x3_direct_fwd(const void* x, const void* w2, const float* bias,
                               const void* relu_mask, void* y, float* colstats, int B, int H, int W,
                               int Cin, int Cout, int relu_in, void* stream);
/* dW2 [Cout, 9*Cin] fp32 (+)= sum over pixels of dy [B,H,W,Cout] x patch(relu_in ? relu(x) : x);
 * Cout % 32 == 0 (<= 256), Cin % 64 == 0 (<= 512); dbias [Cout] fp32 (+)= sum over pixels of dy, or NULL (it rides on a spare
 * accumulator of the same kernel).  Persistent workgroups write one fp32 partial each into the
 * workspace, a second kernel sums them in a fixed order (deterministic, no atomics). */
int ssl4gie_conv3x3_direct_wgrad_ok(int B, int H, int W, int Cin, int Cout);
size_t ssl4gie_conv3x3_direct_wgrad_workspace_bytes(int B, int H, int W, int Cin, int Cout);
int ssl4gie_conv3x3_direct_wgrad(const void* dy, const void* x, float* dw2, float* dbias,
                                 void* workspace, size_t workspace_bytes, int B, int H, int W, int Cin,
                                 int Cout, int relu_in, int accumulate, void* stream);
/* torchvision ResNet.conv1 = nn.Conv2d(3, 64, 7, stride 2, pad 3, bias=False) (reference
 * Models/models.py:63-69) WITHOUT a patch matrix (ssl4gie_stem_im2col7x7 + GEMM remain for fp32).
 *   pack:  img fp32 [B,3,H,W] -> packed bf16 [B, 2 Ho + 6, 2 Wo + 6, 4] (three channels + a zero,
 *          three pixels / rows of zero padding in front), Ho = (H-1)/2 + 1, Wo likewise; once per
 *          batch, shared by every forward on it and by the weight gradient.
 *   fwd:   y [B,Ho,Wo,64] bf16 = conv(packed, w2s), w2s bf16 [64][8][8][4] = weight[co][c][ky][kx]
 *          at [co][ky][kx][c], zero where ky = 7, kx = 7 or c = 3.  colstats (optional): fp32
 *          [ssl4gie_stem7x7_tiles(B,H,W)][2][64] per-tile BatchNorm partial statistics of y.
 *   wgrad: dw2s fp32 [64][7][8][4] (+)= sum over output pixels of dy [B,Ho,Wo,64] x patch; the
 *          kx = 7 and c = 3 entries are arithmetic by-products, not gradients (their weights do
 *          not exist).  Deterministic: per-workgroup partials + fixed-order reduction. */
size_t ssl4gie_stem7x7_packed_bytes(int B, int H, int W);
int ssl4gie_stem7x7_pack(const float* img, void* packed, int B, int H, int W, void* stream);
int ssl4gie_stem7x7_tiles(int B, int H, int W);
int ssl4gie_stem7x7_fwd(const void* packed, const void* w2s, void* y, float* colstats, int B, int H,
                        int W, void* stream);
size_t ssl4gie_stem7x7_wgrad_workspace_bytes(int B, int H, int W);
int ssl4gie_stem7x7_wgrad(const void* dy, const void* packed, float* dw2s, void* workspace,
                          size_t workspace_bytes, int B, int H, int W, int accumulate, void* stream);
/* MoCo-v3 ConvStem layer 1 = nn.Conv2d(3, C0, 3, stride 2, pad 1, bias=False) (reference
 * Models/moco_v3/vits.py:92-96) on the fp32 NCHW image itself: no patch matrix, no packed copy (ABI 8).
 * C0 % 16 == 0, 16 <= C0 <= 128; H, W >= 2; Ho = (H-1)/2 + 1, Wo likewise.  dtype = type of y / dy:
 * SSL4GIE_BF16 (image and weight rounded to bf16 on the way in, MFMA) or SSL4GIE_F32 (plain fp32 FMA chains).
 *   fwd:   img fp32 [B,3,H,W], weight fp32 [C0][3][3][3] (the parameter) -> y [B,Ho,Wo,C0].  colstats
 *          (optional): fp32 [ssl4gie_stem3x3_tiles(B,H,W)][2][C0], per-tile column sums / sums of squares of
 *          the STORED y, as ssl4gie_bn_fwd (FROM_PARTIALS) / ssl4gie_bn_stats take.
 *   wgrad: dweight fp32 [C0][3][3][3] (+)= sum over output pixels of dy [B,Ho,Wo,C0] x image patch.
 *          Deterministic: one fp32 partial per workgroup in `workspace` + a fixed-order reduction.
 * Any other shape returns SSL4GIE_EARG. */
int ssl4gie_stem3x3_tiles(int B, int H, int W);
int ssl4gie_stem3x3_fwd(const float* img, const float* weight, void* y, float* colstats, int dtype, int B,
                        int H, int W, int C0, void* stream);
size_t ssl4gie_stem3x3_wgrad_workspace_bytes(int dtype, int B, int H, int W, int C0);
int ssl4gie_stem3x3_wgrad(const void* dy, const float* img, float* dweight, void* workspace,
                          size_t workspace_bytes, int dtype, int B, int H, int W, int C0, int accumulate,
                          void* stream);
/* F.interpolate(scale_factor=2, mode="bilinear", align_corners=True) (:293-295, Interpolate :69-104)
 * x [B,H,W,C] -> y [B,2H,2W,C]; backward in gather form (no atomics) */
int ssl4gie_bilinear2x_fwd(const void* x, void* y, int dtype, int B, int H, int W, int C,
                           void* stream);
int ssl4gie_bilinear2x_bwd(const void* dy, void* dx, int dtype, int B, int H, int W, int C,
                           void* stream);
/* ---------------------------------------------------------------- atrous glue of DeepLabV3+ (channels-last)
 * What segmentation_models_pytorch 0.3.2 (not vendored, not installed: restated from its published source) runs
 * around the 1x1 convolutions of smp.DeepLabV3Plus(encoder_name="resnet50").  Maps are [B, H, W, C] in `dtype`,
 * accumulation is fp32, nothing uses float atomics (results repeat bit for bit), and a tap outside the map is never
 * turned into an address.  These entry points joined revision 12 (added symbols, nothing existing changed).
 *
 * im2col3x3_dil: the patch matrix of nn.Conv2d(k = 3, stride 1, padding = dilation = d) — what the encoder's
 *   make_dilated() turns layer4's 3x3 convolutions into at output stride 16 (d = 2).  Same [B H W, ld] layout, (ky, kx, c)
 *   column order and zero pad columns as ssl4gie_im2col3x3, so ssl4gie_conv3x3_weight_pack (modes 0 / 1) and
 *   ssl4gie_gemm give the forward, the data gradient (the same call on dy with the flipped image) and, with
 *   ssl4gie_conv3x3_wgrad_unpack, the weight gradient.  C % 8 == 0 (bf16) / % 4 == 0 (fp32), d >= 1, ld >= 9 C.
 * dwconv3x3_fwd: the depthwise half of the decoder's SeparableConv2d (nn.Conv2d(C, C, 3, padding = dilation = d,
 *   groups = C, bias = False): the three ASPPSeparableConv branches at rates 12 / 24 / 36, aspp.1 and block2.0 at d = 1),
 *   weight fp32 [C, 3, 3] (the parameter's [C, 1, 3, 3]), C % 8 == 0.  flip = 1 reads the weight as w[c, 2-ky, 2-kx]:
 *   the data gradient is this call on dy.
 * dwconv3x3_wgrad: dweight [C, 3, 3] fp32 (+)= sum over pixels of dy[b,y,x,c] x[b, y + (ky-1) d, x + (kx-1) d, c];
 *   fp32 partials in `workspace`, summed in a fixed order by a second kernel.
 * bilinear_up_ac_fwd / _bwd: nn.UpsamplingBilinear2d(scale_factor = s) (align_corners=True; the decoder's `up` and the
 *   SegmentationHead's up-sampling, s = 4): x [B,H,W,C] -> y [B, sH, sW, C], source coordinate o (H-1) / (sH-1);
 *   integer s >= 2, any C >= 1 (16-byte accesses when C allows them); the backward gathers per input pixel.
 * chan_copy: torch.cat((...), dim=1) of ASPP.forward / DeepLabV3PlusDecoder.forward and its gradient:
 *   dst[r, 0:C) = src[r / rep, 0:C) for `rows` rows with row strides lds / ldd in elements (the caller offsets the
 *   pointers to the channel slice); rep = H W broadcasts a per-image row (ASPPPooling's F.interpolate from 1x1). */
int ssl4gie_im2col3x3_dil(const void* x, void* cols, int dtype, int B, int H, int W, int C, int dilation,
                          long long ld, void* stream);
int ssl4gie_dwconv3x3_fwd(const void* x, const float* w, void* y, int dtype, int B, int H, int W, int C,
                          int dilation, int flip, void* stream);
size_t ssl4gie_dwconv3x3_wgrad_workspace_bytes(int dtype, int B, int H, int W, int C);
int ssl4gie_dwconv3x3_wgrad(const void* dy, const void* x, float* dweight, void* workspace, size_t workspace_bytes,
                            int dtype, int B, int H, int W, int C, int dilation, int accumulate, void* stream);
int ssl4gie_bilinear_up_ac_fwd(const void* x, void* y, int dtype, int B, int H, int W, int C, int scale,
                               void* stream);
int ssl4gie_bilinear_up_ac_bwd(const void* dy, void* dx, int dtype, int B, int H, int W, int C, int scale,
                               void* stream);
int ssl4gie_chan_copy(const void* src, long long lds, void* dst, long long ldd, int dtype, long long rows, int C,
                      long long rep, void* stream);
/* ConvTranspose2d(k = s) (:345-354, :371-380) = GEMM + scatter: g [B*H*W, k*k*C] with columns
 * ordered (i, j, c) -> y[b, k*y+i, k*x+j, c] = g + bias[c]; unshuffle is its inverse (gradient) */
int ssl4gie_pixel_shuffle(const void* g, const float* bias, void* y, int dtype, int B, int H, int W,
                          int k, int C, void* stream);
int ssl4gie_pixel_unshuffle(const void* dy, void* dg, int dtype, int B, int H, int W, int k, int C,
                            void* stream);
/* Slice(1) + Transpose + Unflatten (:5-11, :449-459): fp32 tap z [B, 1+L, D] -> x [B*L, D] in
 * `dtype` (cls row dropped); gradient: dz[:,0] = 0, dz[:,1:] = dx */
int ssl4gie_tokens_to_map(const float* z, void* x, int dtype, int B, int L, int D, void* stream);
int ssl4gie_map_to_tokens(const void* dx, float* dz, int dtype, int B, int L, int D, void* stream);
/* op 0: out = a + b (skip_add :233, :290);  op 1: out = (a > 0 ? b : 0) + (c ? c : 0): gradient
 * through the ReLU that precedes a conv (a = the activation's input) plus the skip gradient */
int ssl4gie_eltwise(int op, const void* a, const void* b, const void* c, void* out, int dtype,
                    long long n, void* stream);
/* depth head tail ReLU -> Conv2d(32, 1, 1) -> Sigmoid (:479-481): y[m] = sigmoid(sum_c relu(x[m,c])
 * w[c] + bias[0]), y fp32 [M]; backward gives dx and dw [C], db [1] (two-stage reduction) */
int ssl4gie_depth_head_fwd(const void* x, const float* w, const float* bias, float* y, int dtype,
                           long long M, int C, void* stream);
size_t ssl4gie_depth_head_bwd_workspace_bytes(long long M, int C);
int ssl4gie_depth_head_bwd(const void* x, const float* w, const float* y, const float* dy, void* dx,
                           float* dw, float* db, int accumulate, float* workspace, int dtype,
                           long long M, int C, void* stream);

/* ---------------------------------------------------------------- ResNet50 glue (channels-last)
 * Replaces the torch ops around the convolutions of torchvision ResNet(Bottleneck,[3,4,6,3]) as the
 * reference builds it (Models/models.py:63-152; MoCo: Models/moco_v3/main_moco.py:185-187).  1x1
 * convolutions are token-major ssl4gie_gemm calls, 3x3 ones go through ssl4gie_im2col3x3.
 * stem_im2col7x7: fp32 NCHW image -> conv1 (7x7, s2, p3) patch matrix [B*Ho*Wo, ld], K = 147
 *   ordered (dy, dx, c), columns [147, ld) zero.
 * subsample2: rows of a stride-2 1x1 convolution (downsample.0); backward = 1 scatters zeros. */
int ssl4gie_stem_im2col7x7(const float* img, void* cols, int dtype, int B, int H, int W,
                           long long ld, void* stream);
int ssl4gie_subsample2(const void* x, void* y, int dtype, int B, int H, int W, int C, int backward,
                       void* stream);
/* BatchNorm2d / BatchNorm1d / SyncBatchNorm in training mode over the rows of a channels-last map x [rows, C]
 * (C % 8 == 0), fused with the bottleneck's residual add and ReLU: y = act(xhat gamma + beta (+ res)), statistics in
 * fp32 (biased variance for the normalisation, unbiased for running_var, momentum as nn.BatchNorm: running =
 * (1-m) running + m batch).  Backward: g = masked dy, dgamma = sum g xhat, dbeta = sum g,
 * dx = gamma rstd (g - mean(g) - xhat mean(g xhat)), dres (optional) = g.  Five functions span a small product (and
 * a sixth, ssl4gie_bn_bwd_frozen, is the backward through fixed statistics); a
 * combination outside it (a pointer the form does not use included: pass NULL) is SSL4GIE_EARG.  gamma / beta / res /
 * running_* may be NULL wherever they are used.
 *
 * ssl4gie_bn_fwd: where the normalisation comes from (`source`) x what is written.
 *   FROM_X         statistics pass over x; mean / rstd are OUTPUTS (kept for backward), running_* updated; writes y.
 *   FROM_PARTIALS  the same statistics from `partial` [parts][2][C], the per-128-row sums the producing GEMM wrote
 *                  (ssl4gie_gemm_desc::colstats), instead of a pass over x.  Writes y (+ relu_bits), or — y, x, res
 *                  NULL — only the coefficients coef [2][C] with y = x coef[0][c] + coef[1][c], for a consumer that
 *                  applies them itself: ssl4gie_bn_maxpool3x3s2_fwd, the
 *                  SSL4GIE_EPI_AFFINE_AUX_RELU epilogue (MoCo's momentum encoder, moco/builder.py:127-135).
 *   FROM_STATS     mean / rstd are INPUTS (evaluation, or the GLOBAL statistics of a SyncBatchNorm exchange): no
 *                  reduction runs, running_* must be NULL.  Writes y, or — y, x, res, workspace NULL, only C > 0
 *                  required — coef.
 *   FROM_COEF      coef is an INPUT (as the coefficients-only forms write it): y and relu_bits (both required, bf16,
 *                  relu != 0); mean / rstd / gamma / beta / workspace NULL.
 *   relu_bits (FROM_PARTIALS and FROM_COEF, bf16, relu != 0): bit j of relu_bits[i] = (y[8 i + j] > 0), rows * C / 8
 *   bytes — the backward's ReLU mask at 1/16 of y's bytes (bn3 of a torchvision Bottleneck).
 *
 * ssl4gie_bn_stats: the LOCAL (mean, biased var) of SyncBatchNorm's forward, from a pass over x or (x NULL) from
 *   `partial`; the caller combines the ranks (ssl4gie_bn_combine_stats) and calls ssl4gie_bn_fwd(FROM_STATS).
 *
 * Backward: where the ReLU mask comes from (`mask_kind`, `mask`) x how the pass is split.
 *   MASK_NONE  no ReLU; mask NULL.
 *   MASK_Y     mask = the ReLU output y.
 *   MASK_X     BatchNorm + ReLU WITHOUT a residual input (mask and dres NULL): the mask is rebuilt as x a + b > 0 from
 *              the forward's own coefficients (a = rstd gamma, b = beta - mean a: gamma / beta must be the forward's),
 *              the ReLU output is not read.  Equals MASK_Y exactly unless the forward rounded a positive
 *              pre-activation below the operand type's smallest subnormal to zero.
 *   MASK_BITS  mask = the forward's relu_bits (bf16); dres (required) receives the masked gradient, which the apply
 *              pass reads.  Equals MASK_Y exactly.
 *   beta is read by MASK_X only (NULL otherwise).
 *   ssl4gie_bn_bwd         one rank: reduction, dgamma / dbeta (overwritten or accumulated), dx, dres.
 *   ssl4gie_bn_bwd_reduce  SyncBatchNorm, first half: sums [2][C] = LOCAL (sum g, sum g xhat), and dres; gamma is
 *                          read by MASK_X only.  The caller all-reduces sums.
 *   ssl4gie_bn_bwd_apply   second half: dx from the GLOBAL sums and inv_count = 1 / global row count.  MASK_NONE, _Y
 *                          or _X; after a MASK_BITS (or any residual + ReLU) reduce, apply on its dres with MASK_NONE.
 *   (convert_sync_batchnorm: Depth_estimation/train_depth.py:225, Models/moco_v3/main_moco.py:196.)
 *   ssl4gie_bn_bwd_frozen  backward through FIXED statistics: BatchNorm in evaluation mode, and torchvision's
 *                          FrozenBatchNorm2d of fasterrcnn_resnet50_fpn's trunk (Object_detection/
 *                          train_detection.py:197-202).  mean / rstd are the running ones, so no term depends on a
 *                          sum over the batch: g = masked dy, a = rstd gamma (gamma NULL: 1), dx = a g, dres
 *                          (optional) = g bit for bit, and where given dbeta = sum g, dgamma = sum g xhat (overwritten
 *                          or accumulated).  Without dgamma / dbeta it is ONE flat pass (MASK_Y: dy, y -> dx (, dres);
 *                          MASK_BITS: dy and 1/16 of a map -> dx, dres) and workspace is NULL; with them one reduction
 *                          pass that writes dx and dres as well, then the tail, and workspace is required.  x and
 *                          mean are read by MASK_X or for dgamma only and are NULL otherwise; beta by MASK_X only.
 *                          C % 8 == 0 (bf16) / C % 4 == 0 (fp32).
 *
 * `workspace`: ssl4gie_bn_workspace_bytes(rows, C) bytes, as floats [coef 3C][partials parts x 2C][sums 2C][pivot C]
 * with room for the 64 x 2C fold of caller-supplied partials; the backward reuses the regions (`sums`: the mask
 * coefficients of MASK_X, `pivot`: an aligned copy of mean). */
enum { SSL4GIE_BN_FROM_X = 0, SSL4GIE_BN_FROM_PARTIALS = 1, SSL4GIE_BN_FROM_STATS = 2, SSL4GIE_BN_FROM_COEF = 3 };
enum { SSL4GIE_BN_MASK_NONE = 0, SSL4GIE_BN_MASK_Y = 1, SSL4GIE_BN_MASK_X = 2, SSL4GIE_BN_MASK_BITS = 3 };
size_t ssl4gie_bn_workspace_bytes(long long rows, int C);
int ssl4gie_bn_fwd(int source, const void* x, const float* partial, int parts, const float* gamma,
                   const float* beta, const void* res, void* y, unsigned char* relu_bits, float* coef, float* mean,
                   float* rstd, float* running_mean, float* running_var, float momentum, float eps, int relu,
                   float* workspace, int dtype, long long rows, int C, void* stream);
int ssl4gie_bn_stats(const void* x, const float* partial, int parts, float* mean, float* var, float* workspace,
                     int dtype, long long rows, int C, void* stream);
int ssl4gie_bn_bwd(const void* dy, int mask_kind, const void* mask, const void* x, const float* gamma,
                   const float* beta, const float* mean, const float* rstd, void* dx, void* dres, float* dgamma,
                   float* dbeta, int accumulate, float* workspace, int dtype, long long rows, int C, void* stream);
int ssl4gie_bn_bwd_reduce(const void* dy, int mask_kind, const void* mask, const void* x, const float* gamma,
                          const float* beta, const float* mean, const float* rstd, void* dres, float* sums,
                          float* workspace, int dtype, long long rows, int C, void* stream);
int ssl4gie_bn_bwd_apply(const void* dy, int mask_kind, const void* mask, const void* x, const float* gamma,
                         const float* beta, const float* mean, const float* rstd, const float* sums, float inv_count,
                         void* dx, float* workspace, int dtype, long long rows, int C, void* stream);
int ssl4gie_bn_bwd_frozen(const void* dy, int mask_kind, const void* mask, const void* x, const float* gamma,
                          const float* beta, const float* mean, const float* rstd, void* dx, void* dres, float* dgamma,
                          float* dbeta, int accumulate, float* workspace, int dtype, long long rows, int C,
                          void* stream);
/* The exchange's arithmetic as ONE launch: gathered [world][2C + 1] = every rank's (mean[C], biased var[C],
 * row count) -> pooled mean / rstd (ranks may hold different row counts), the total row count (device
 * scalar) and, if given, the running statistics (unbiased variance, momentum) — what torch.nn.SyncBatchNorm
 * does between its all_gather and its normalisation kernel. */
int ssl4gie_bn_combine_stats(const float* gathered, int world, int C, float eps, float momentum,
                             float* running_mean, float* running_var, float* mean, float* rstd, float* total,
                             void* stream);
/* MoCo._update_momentum_encoder (moco/builder.py:57-61): dst = dst m + src (1 - m), fp32, over a
 * whole parameter-arena slice */
int ssl4gie_ema_update(float* dst, const float* src, float m, long long n, void* stream);
/* MaxPool2d(3, stride 2, pad 1) with the argmax window position saved (first maximum in row-major
 * scan order); backward in gather form.  Global average pool -> fp32 [B, C] and its gradient. */
int ssl4gie_maxpool3x3s2_fwd(const void* x, void* y, unsigned char* arg, int dtype, int B, int H,
                             int W, int C, void* stream);
int ssl4gie_maxpool3x3s2_bwd(const void* dy, const unsigned char* arg, void* dx, int dtype, int B,
                             int H, int W, int C, void* stream);
/* The same pool over act(x coef[0][c] + coef[1][c]), act = ReLU if `relu` (coef [2][C] as the coefficients-only ssl4gie_bn_fwd
 * writes it): torchvision ResNet's bn1 -> relu -> maxpool behind the stem convolution in ONE pass over the
 * convolution's output — the normalised map is never written (the backward rebuilds its ReLU mask from the
 * convolution output: ssl4gie_bn_bwd with MASK_X).  Values and argmax equal ssl4gie_bn_fwd (FROM_PARTIALS) followed by
 * ssl4gie_maxpool3x3s2_fwd bit for bit.  C % 8 == 0 (bf16) / C % 4 == 0 (fp32). */
int ssl4gie_bn_maxpool3x3s2_fwd(const void* x, const float* coef, int relu, void* y, unsigned char* arg,
                                int dtype, int B, int H, int W, int C, void* stream);
int ssl4gie_avgpool_fwd(const void* x, float* y, int dtype, int B, int HW, int C, void* stream);
int ssl4gie_avgpool_bwd(const float* dy, void* dx, int dtype, int B, int HW, int C, void* stream);

/* ---------------------------------------------------------------- optimizer steps over the arena
 * One parameter arena = S segments (one per parameter, 64-element aligned; padding stays zero).
 * Device tables: seg_start [S+1] int64 element offsets, seg_lr [S] (< 0: skip the segment: frozen or
 * without a gradient this step), seg_wd [S], seg_mat [S] (LARS: 1 for p.ndim > 1).
 * lars_arena: Models/moco_v3/moco/optimizer.py:18-43: matrices dp = (g + wd p) trust |p|/|dp|
 *   (1 where a norm is 0), vectors dp = g; mu = momentum mu + dp; p -= lr mu.
 * sgd_arena: torch.optim.SGD(momentum, weight_decay) with dampening 0 and no Nesterov (main_lincls.py:236-238):
 *   d = g + wd p; buf = momentum buf + d; p -= lr buf.  A zero buf reproduces torch's first step (buf = d).
 *   A skipped segment's p and buf (its padding included) stay bit-unchanged; an active segment's zero padding
 *   stays zero (g, p and buf are all zero there).
 * lars_arena and sgd_arena take the n elements (n % 4 == 0) behind the pointers they are given (sgd_arena: 16-byte
 * aligned): a caller may hand them a sub-range of the arena with seg_start rebased to it. */
size_t ssl4gie_lars_workspace_bytes(int S);
int ssl4gie_lars_arena(float* p, const float* g, float* mu, const long long* seg_start,
                       const float* seg_lr, const float* seg_wd, const float* seg_mat, int S,
                       float momentum, float trust, float* workspace, long long n, void* stream);
int ssl4gie_sgd_arena(float* p, const float* g, float* buf, const long long* seg_start, const float* seg_lr,
                      const float* seg_wd, int S, float momentum, long long n, void* stream);
/* ---- the reference's scaler object over the arena (Models/mae/util/misc.py:251-292,
 * NativeScalerWithGradNormCount: unscale_ -> get_grad_norm_ / clip_grad_norm_ -> scaler.step; driven from
 * Models/mae/engine_pretrain.py:39-69 and engine_finetune.py:66 / main_finetune.py --clip_grad).
 * seg_mask [S]: < 0 skips the segment (frozen, or no gradient this step: its slice of g may hold stale
 * values and is not read) — the optimizers' seg_lr table has that meaning already and can be passed.
 * ctl: 4 floats on the device, written by grad_norm_arena and read by the other two:
 *   ctl[0] L2 norm of inv_scale * g over the active segments      (misc.py:280-292 get_grad_norm_)
 *   ctl[1] min(1, max_norm / (ctl[0] + 1e-6)), exactly 1 for max_norm <= 0   (torch clip_grad_norm_, misc.py:263)
 *   ctl[2] 1 if any active element of g is inf or NaN, else 0 — per element, as GradScaler.unscale_'s
 *          _amp_foreach_non_finite_check_and_unscale_ decides it (misc.py:262,265)
 *   ctl[3] 0 (reserved)
 * grad_norm_arena: one pass over g (fixed grid, fixed order, no atomics; four fp32 sums per thread, added
 *   as doubles before the wave shuffle, fp64 from there on):
 *   bit-identical from run to run for the same g, tables and n.  workspace: grad_norm_workspace_bytes(),
 *   8-byte aligned.  n % 4 == 0.
 * grad_scale_arena: g *= ctl[1] over the active segments — clip_grad_norm_'s side effect on p.grad;
 *   writes nothing when ctl[1] is exactly 1. */
size_t ssl4gie_grad_norm_workspace_bytes(void);
int ssl4gie_grad_norm_arena(const float* g, const long long* seg_start, const float* seg_mask, int S,
                            float inv_scale, float max_norm, void* workspace, float* ctl, long long n,
                            void* stream);
int ssl4gie_grad_scale_arena(float* g, const long long* seg_start, const float* seg_mask, int S,
                             const float* ctl, long long n, void* stream);
/* adamw_arena: torch.optim.AdamW's update (main_pretrain.py:179-180, train_depth.py:280) of the arena elements
 * [lo, hi) (multiples of 4, hi >= lo; whole segments in practice; pointers and seg_start are the whole arena's).
 * m / v are the flat moment buffers.  lp_bf16 (may be NULL): the bf16 operand copy of every UPDATED element is
 * written there too (the flat shadow arena the GEMM operands are views of; skipped segments are left as they
 * are), which saves the separate cast pass.  Ranges let the update of a transformer block's parameters be
 * enqueued on a side stream as soon as that block's backward is (optim.ArenaAdamW, overlap_backward); the
 * ranges of one step must cover the arena exactly once.  hi == lo launches no update.
 *   ctl == NULL, host-counted: `step` (> 0) is the 1-based step count of the bias corrections; applied must
 *     be NULL and skip_nonfinite and advance 0.
 *   ctl != NULL, device-counted (misc.py:267 `self._scaler.step(optimizer)` after a clip): the gradient is
 *     ctl[1] * g (g itself is left as it is), and with skip_nonfinite != 0 NOTHING is written while ctl[2] is
 *     set — not p, m, v, nor lp_bf16 — GradScaler.step's skip.  torch does not call optimizer.step() for a
 *     skipped update, so its bias-correction step does not advance either; the host cannot know without
 *     synchronising, so the count of APPLIED updates lives on the device: *applied (one int, caller-owned, not
 *     NULL, 0 for a fresh optimizer) is read by the kernel (step = *applied + 1; `step` is ignored), and with
 *     advance != 0 a one-thread launch behind it adds 1 unless the update was skipped (also when hi == lo).
 *     Pass advance on the last range of a step only.
 * Any other combination returns SSL4GIE_EARG before anything is launched. */
int ssl4gie_adamw_arena(float* p, const float* g, float* m, float* v, const long long* seg_start,
                        const float* seg_lr, const float* seg_wd, int S, float beta1, float beta2, float eps,
                        int step, int* applied, long long lo, long long hi, void* lp_bf16, const float* ctl,
                        int skip_nonfinite, int advance, void* stream);

/* ---------------------------------------------------------------- linear probe: scoring
 * (csrc/probe_ops.hip; joined ABI 12 as additions).  The frozen trunk's forward is the bulk of a probe step
 * (Models/mae/main_linprobe.py, Models/moco_v3/main_lincls.py) and is not touched; the head's SGD step is
 * ssl4gie_sgd_arena above.
 *
 * topk_update  accuracy(output, target, topk) (main_lincls.py:506-520; timm's accuracy at Models/mae/engine_finetune.py:
 *              19,119-124) and the criterion's value for one batch, added into caller-owned device accumulators so
 *              that a loader is scored with ONE read-back instead of one .item() per meter per batch.
 *              logits [B, C] of `dtype` (SSL4GIE_F32 / SSL4GIE_BF16) with row stride ld >= C ELEMENTS; target int64 [B];
 *              ks: HOST array of nk (1..8) strictly ascending values in [1, C].
 *              acc int64 [nk + 2] += (hits at ks[0], ..., hits at ks[nk - 1], rows counted, rows rejected);
 *              loss_sum fp64 [1] += the sum of the counted rows' cross-entropy; rank (int32 [B]) / row_loss (fp32 [B]),
 *              each may be NULL, are overwritten: the row's rank and loss, -1 and 0 for a rejected row.
 *              Rank of a row = the number of columns ordered above the target's logit; equal values are ordered by
 *              lower index first (the rule of ssl4gie_confusion_update's argmax; torch.topk leaves ties open), a NaN
 *              above every number as torch orders it, NaNs among themselves by lower index first.  Hit at k: rank < k.
 *              A target outside [0, C) is never used as an index: the row is counted as rejected and adds to nothing
 *              else.  Loss = logsumexp - target logit in fp32 with the row maximum subtracted (logits of magnitude 1e4
 *              give a finite loss); a row holding a NaN has a NaN loss, which reaches loss_sum.
 *              One wave per row; a row is walked in 16-byte chunks, a chunk inside the row at a 16-byte aligned address
 *              by one load and any other column by column, on the same lane either way: any C, ld and base are
 *              accepted and a row's loss does not depend on its alignment.  The row losses are added in fp64 in a fixed
 *              order (rows in index order over 256 threads, then a tree), no floating-point atomics: the same inputs
 *              give the same bits from run to run and for any grid.  The counts are integer atomics.
 *              workspace: ssl4gie_topk_workspace_bytes(B) bytes (0 for B <= 0), 4-byte aligned.  C <= 2^30. */
size_t ssl4gie_topk_workspace_bytes(int B);
int ssl4gie_topk_update(const void* logits, int dtype, long long ld, const long long* target, const int* ks, int nk,
                        long long* acc, double* loss_sum, int* rank, float* row_loss, int B, int C, void* workspace,
                        void* stream);

/* ---------------------------------------------------------------- input pipeline
 * transforms.ToTensor() + transforms.Normalize(mean, std) (Depth_estimation/Data/dataloaders.py:
 * 55-63) on the device: uint8 HWC [B, H, W, 3] -> fp32 NCHW [B, 3, H, W] = (x / 255 - mean) / std.
 * mean / std are HOST arrays of 3 floats; H*W % 4 == 0. */
int ssl4gie_normalize_u8(const unsigned char* img, float* out, const float* mean, const float* std,
                         int B, int H, int W, void* stream);
/* transforms.RandomResizedCrop(S, scale, interpolation=3) + RandomHorizontalFlip + ToTensor + Normalize
 * (Models/mae/main_pretrain.py:123-127; with SSL4GIE_FILTER_BILINEAR the geometric part of
 * Models/moco_v3/main_moco.py:263,275) out of a uint8 image bank that lives on the device, with the boxes and
 * flips already drawn: sample b is image index[b] of bank [n, Hs, Ws, 3], cropped to box[b] = (top, left,
 * height, width), resampled to S x S by PIL's rule (separable, antialiased: the filter widens by
 * max(1, length / S); taps never leave the box; Keys cubic a = -0.5 or the triangle), mirrored left-right where
 * flip[b] != 0 (flip == NULL: never), clamped to [0, 255] and written as fp32 NCHW out[b] = (v / 255 - mean) /
 * std.  Values are NOT rounded to integer levels between the passes as PIL's 8-bit images are.
 * index / box / flip are DEVICE arrays, so they are checked by the kernel: a sample whose index is outside
 * [0, n) or whose box is not inside the image (height < 1, width < 1, top < 0, left < 0, top + height > Hs,
 * left + width > Ws) comes out all NaN, and no address is formed from its values.  mean / std are HOST arrays
 * of 3 floats.  SSL4GIE_EARG: a null pointer, S % 4 != 0, std <= 0, an unknown filter, or an (Hs, Ws, S) whose
 * whole-image box does not fit one CU's LDS (Hs, Ws <= 1024 at S = 224 do).  fp32 accumulation in a fixed
 * order: bit-identical from run to run. */
#define SSL4GIE_FILTER_BILINEAR 0
#define SSL4GIE_FILTER_BICUBIC 1
int ssl4gie_view_sample_u8(const unsigned char* bank, long long n, int Hs, int Ws, const long long* index,
                           const int* box, const unsigned char* flip, float* out, int B, int S, int filter,
                           const float* mean, const float* std, void* stream);
/* The colour half of MoCo-v3's two-view augmentation (Models/moco_v3/main_moco.py:262-285, moco/loader.py:26-42:
 * RandomApply(ColorJitter) -> RandomGrayscale -> GaussianBlur -> Solarize -> Normalize) with the per-sample
 * parameters already drawn: x fp32 [B, 3, S, S] in [0, 1] (ssl4gie_view_sample_u8 with mean 0, std 1) -> out, the
 * normalised fp32 [B, 3, S, S].  Crop and flip have happened before; every op here is pointwise or a symmetric
 * stencil, so flipping first equals the reference's flipping last.  The rule, per sample b, on clamp(x, 0, 1):
 *   1. jitter: order[b][0..3] are op ids applied left to right, an id at most once, 255 = skip;
 *      blend(a, d, f) = clamp(f a + (1 - f) d, 0, 1), gray(x) = 0.299 r + 0.587 g + 0.114 b (PIL's "L"),
 *      f = factors[b][id] (factors [B, 4] = brightness, contrast, saturation, hue):
 *        0 brightness blend(x, 0, f);  1 contrast blend(x, m, f), m = the mean of gray over the sample's whole image
 *        after the ops that precede contrast in its order;  2 saturation blend(x, gray(x), f);
 *        3 hue: rgb -> hsv, h <- (h + f) mod 1, hsv -> rgb by the colorsys formulas in floating point
 *        (torchvision's tensor path), p, q, t clamped to [0, 1]; a pixel with max == min keeps its value;
 *   2. flags[b] & 1: all three channels <- gray(x);
 *   3. sigma[b] > 0: separable true Gaussian, R = ceil(3 sigma) (supported: R <= 6, sigma <= 2), weights
 *      exp(-k^2 / 2 sigma^2), k in [-R, R], over their sum; horizontal pass, then vertical; symmetric edges
 *      (index -1 - i reads i, S + i reads S - 1 - i).  PIL's GaussianBlur(radius = sigma) is a three-pass box
 *      approximation of this kernel;
 *   4. flags[b] & 2: x >= 128 / 255 -> 1 - x (ImageOps.solarize, threshold 128);
 *   5. (x - mean[c]) / std[c].
 * Values are NOT rounded to integer levels between the ops, as PIL's 8-bit images are.
 * factors / order / flags / sigma are DEVICE arrays, so the host cannot check them: the kernel treats an op id
 * above 3 as a skip and clamps R to 6 (a larger sigma gives a truncated Gaussian; NaN or sigma <= 0: no blur).
 * mean / std are HOST arrays of 3 floats.  workspace: ssl4gie_color_augment_workspace_bytes(B, S) bytes on the
 * device (per-sample partial sums of the contrast mean; 0 for a (B, S) the entry point refuses).
 * SSL4GIE_EARG, before anything is launched: a null pointer, B < 1, S < 8, S % 4 != 0, a std entry equal to 0,
 * out == x (the stencil reads its neighbours' inputs), x or out not 16-byte aligned, a workspace smaller than the
 * query says.
 * Two launches, no atomics, sums in a fixed order: bit-identical from run to run, and a sample's result does not
 * depend on its place in the batch. */
size_t ssl4gie_color_augment_workspace_bytes(int B, int S);
int ssl4gie_color_augment(const float* x, float* out, int B, int S, const float* factors,
                          const unsigned char* order, const unsigned char* flags, const float* sigma,
                          const float* mean, const float* std, void* workspace, size_t workspace_bytes,
                          void* stream);
/* The colour stage of the finetune loaders (Binary_segmentation/Data/dataloaders.py:62-71, Classification/Data/
 * dataloaders.py:62-66: ColorJitter -> GaussianBlur((25, 25), sigma) -> ToTensor -> Normalize).  Arguments, workspace
 * query, steps 1, 2, 4 and 5, guarantees and refusals are ssl4gie_color_augment's; step 3 is
 *   3'. sigma[b] > 0: separable 25-tap Gaussian, k in [-12, 12], weights exp(-k^2 / 2 sigma^2) (sigma the fp32 value it
 *       is) over their sum; horizontal pass, then vertical; reflect edges (index -i reads i, S - 1 + i reads
 *       S - 1 - i): transforms.GaussianBlur((25, 25)) on its tensor path (reflect pad + depthwise conv2d).  The tap
 *       loop stops at ceil(6 sigma) rounded up to even: the taps left out sum to less than 4e-9 of the total weight.
 *       NaN or sigma <= 0: no blur.  At sigma <= 0.05 every weight but the centre's is 0 in fp32 and the result is
 *       the un-blurred one bit for bit (the reference's lower end, 0.001, is such a sigma).
 * SSL4GIE_EARG in addition: S < 16 (a reflect halo of 12 needs S > 12). */
int ssl4gie_color_augment_ft(const float* x, float* out, int B, int S, const float* factors,
                             const unsigned char* order, const unsigned char* flags, const float* sigma,
                             const float* mean, const float* std, void* workspace, size_t workspace_bytes,
                             void* stream);
/* The geometric stage of the finetune loaders (Binary_segmentation/Data/dataset.py:46-63: hflip, vflip, TF.affine on
 * the normalised tensor and its mask; Depth_estimation/Data/dataset.py:47-70: the flips; Classification/Data/
 * dataloaders.py:67-69: flips + RandomRotation) with the parameters already drawn, image and target through the same
 * nearest-neighbour map in one launch.  img / img_out fp32 [B, 3, S, S]; the target of sample b is
 * tgt_bank[index[b]] of a bank [n, S, S] of tgt_dtype (u8 -> v / 255, u16 -> v / 65535, fp32 as it is), written to
 * tgt_out fp32 [B, 1, S, S]; tgt_bank, index and tgt_out are all given or all NULL.  Output pixel (i, j) of sample
 * b, with c = (S - 1) / 2, xo = j - c, yo = i - c and m = matrix[b] (fp32 [B, 6], torchvision's inverse affine
 * matrix; NULL = identity):
 *   sx = m0 xo + m1 yo + m2 + c,  sy = m3 xo + m4 yo + m5 + c,  ix = rint(sx), iy = rint(sy) (half to even) —
 *   F.grid_sample(mode = "nearest", align_corners = False) on torchvision's _gen_affine_grid;
 *   (ix, iy) outside [0, S)^2: fill_img[ch] / fill_tgt;  otherwise ix <- S - 1 - ix where flip[b] & 1, iy <- S - 1 -
 *   iy where flip[b] & 2 (flip uint8 [B] or NULL; the reference flips before the affine, so the source is mirrored),
 *   and the pixel is the source pixel.
 * sx, sy are evaluated in fp32: a source coordinate within 1e-4 of a half-integer may round to either neighbour.
 * index / matrix / flip are DEVICE arrays: an index outside [0, n) gives an all-NaN target sample, a NaN or
 * out-of-range coordinate is the fill, and no address is formed from either.  fill_img is a HOST array of 3 floats.
 * SSL4GIE_EARG, before anything is launched: a null img / img_out / fill_img, S < 4, S % 4 != 0, img_out overlapping
 * img (a gather cannot run in place), a pointer not 16-byte aligned, a target given in part (tgt_out without
 * tgt_bank, ...), an unknown tgt_dtype, n < 1.  A pure gather: bit-identical from run to run. */
#define SSL4GIE_TGT_U8 0
#define SSL4GIE_TGT_U16 1
#define SSL4GIE_TGT_F32 2
int ssl4gie_paired_warp(const float* img, float* img_out, const void* tgt_bank, int tgt_dtype, long n,
                        const int64_t* index, float* tgt_out, const float* matrix, const uint8_t* flip,
                        const float fill_img[3], float fill_tgt, int B, int S, void* stream);
/* The detection loaders (Object_detection/Data/dataloaders.py:75-112 and Data/dataset.py:38-113 with arch != "resnet50",
 * post_process = False) over a RAGGED uint8 bank on the device: image i is the dense HWC bytes at pixels + offsets[i]
 * (pixels [total], offsets int64 [n]), sizes[i] = (H0, W0) (int32 [n, 2]); sample b of a batch is image index[b]
 * (int64 [B]).  All of these are DEVICE arrays and are checked by the kernels: a sample whose index is outside [0, n),
 * whose side is below 13 or above 32768, whose bytes do not lie inside [0, total), whose H0 W0 exceeds plane_stride
 * (where a scratch is involved) or whose image does not fit F x F after step 6 comes out all NaN (its boxes too), and
 * no address is formed from such a value.  These entry points joined revision 12.
 *
 * ssl4gie_det_color: dataloaders.py:77-80, ColorJitter -> GaussianBlur((25, 25), sigma) on the stored H0 x W0 image,
 *   on x = float(v) / 255 (correctly rounded, ToTensor's value): steps 1 and 3' of ssl4gie_color_augment_ft with H0 and
 *   W0 in S's place on the two axes (the contrast mean over the sample's whole image, reflect edges per axis), no
 *   rounding to 8-bit levels between the ops, no grayscale, solarize or normalisation.  factors fp32 [B, 4], order
 *   uint8 [B, 4], sigma fp32 [B] as there.  Writes scratch fp32 [B][3][plane_stride], rows dense at pitch W0.
 *   max_h / max_w: the largest H0 and W0 of THIS batch, which the host knows; they size the grid only (a smaller image's
 *   surplus workgroups exit, a larger one is still covered).  workspace: ssl4gie_det_color_workspace_bytes(B) bytes.
 *   Two launches (statistics, apply), no atomics, sums in a fixed order that the image's size alone decides.
 * ssl4gie_det_geometry: dataset.py:50-52, 64-66, 73-75 and 82-102 in ONE launch that writes out fp32 [B, 3, F, F].
 *   Source: scratch (as written by ssl4gie_det_color, same B, index and plane_stride) or, with scratch == NULL, the bank
 *   itself through float(v) / 255 (dataloaders.py:116-120: the val / test loaders' ToTensor alone).  geom uint8 [B]
 *   (NULL = 0): bit 0 horizontal flip, bit 1 vertical flip, bit 2 rot90.  With S the source image:
 *     3. rot90:  T1[i][j] = S[j][W0 - 1 - i], H1 = W0, W1 = H0;   4. hflip: T2[i][j] = T1[i][W1 - 1 - j];
 *     5. vflip:  T3[i][j] = T2[H1 - 1 - i][j];
 *     6. only when H1 > F or W1 > F: a zero row below if H1 is odd, a zero column to the right if W1 is odd, then
 *        F.interpolate(bicubic, antialias=True, align_corners=False) to half the size: output i reads the inputs
 *        max(0, 2 i - 3) .. min(L, 2 i + 5) - 1 with Keys' a = -0.5 weights w((j - 2 i - 0.5) / 2) over their sum: in
 *        the interior (-3, -9, 29, 111, 111, 29, -9, -3) / 256.  Horizontal pass, then vertical; no clamp;
 *     7. p1 = floor((F - W2) / 2), p2 = floor((F - H2) / 2): out[c][y][x] = (T[y - p2][x - p1] - mean[c]) / std[c]
 *        inside the image and (0 - mean[c]) / std[c] outside.  mean / std are HOST arrays of 3 floats.
 *   Without step 6 the result is the source value moved: bit-equal to the reference for the bank source.
 * ssl4gie_det_boxes: the box statements of dataset.py:53-61, 67-71, 76-80, 97 and 103-106, one fp32 operation each in
 *   that order, hence bit-equal to the reference.  boxes fp32 [m, 4] = (xmin, ymin, xmax, ymax), labels int64 [m], image
 *   i owns rows box_offsets[i] .. box_offsets[i + 1] (int64 [n + 1]).  out_start int64 [B + 1] (device) says where
 *   sample b's rows go in out_boxes fp32 [m_out, 4] / out_labels int64 [m_out]; a sample whose row count there differs
 *   from its bank count is refused like a bad index: NaN boxes, labels -1.  max_boxes: the largest per-sample count of
 *   the batch (sizes the grid).  One launch.
 * SSL4GIE_EARG, before anything is launched: a null pointer (geom and, for the geometry, scratch may be NULL),
 * F % 4 != 0, a std entry equal to 0, scratch / out / out_boxes / boxes not 16-byte aligned, a workspace smaller than the
 * query says, B > 65535, max_h or max_w below 13.  Pure functions of their inputs: bit-identical from run to run, and
 * a sample's result does not depend on its place in the batch. */
size_t ssl4gie_det_color_workspace_bytes(int B);
int ssl4gie_det_color(const unsigned char* pixels, long long total, const long long* offsets, const int* sizes,
                      long long n, const long long* index, int B, int max_h, int max_w, const float* factors,
                      const unsigned char* order, const float* sigma, float* scratch, long long plane_stride,
                      void* workspace, size_t workspace_bytes, void* stream);
int ssl4gie_det_geometry(const float* scratch, long long plane_stride, const unsigned char* pixels, long long total,
                         const long long* offsets, const int* sizes, long long n, const long long* index,
                         const unsigned char* geom, float* out, int B, int F, const float* mean, const float* std,
                         void* stream);
int ssl4gie_det_boxes(const float* boxes, const long long* labels, const long long* box_offsets, long long m,
                      const int* sizes, long long n, const long long* index, const unsigned char* geom,
                      const long long* out_start, float* out_boxes, long long* out_labels, long long m_out, int B, int F,
                      int max_boxes, void* stream);

/* ---------------------------------------------------------------- RandAugment and RandomErasing (joined ABI 12)
 * The input of the MAE fine-tuning recipe (Models/mae/util/datasets.py:37-48: timm.data.create_transform with
 * auto_augment='rand-m9-mstd0.5-inc1', interpolation='bicubic', re_prob=0.25, re_mode='pixel', re_count=1) after the
 * crop and flip of ssl4gie_view_sample_u8, with the op ids, arguments, matrices and boxes already drawn
 * (ssl4gie_amd.data.RandAugment / RandomErasing).  timm is not vendored by the reference and is absent from the build
 * machine: the op list and level maps restate timm 0.3.2's published source (that boundary is unpinned); every PIXEL
 * rule is PIL's, and tests/test_randaug_checks_cpu.py holds the numpy restatement of each rule below to PIL bit for bit.
 * The intermediate image is uint8 NHWC [B, S, S, 3] (the bank's layout), S % 4 == 0.
 *
 * ssl4gie_quantize_u8: x fp32 NCHW [B, 3, S, S] in 0..255 units (ssl4gie_view_sample_u8 with mean 0 and std 1 / 255)
 *   -> out uint8 NHWC: q = (int)(min(max(x, 0), 255) + 0.5f), the sum in fp32; a NaN gives 0.  One launch.  PIL rounds
 *   to 8 bits after EACH resize pass and uses fixed-point weights; here one rounding follows the fp32 resample.
 *
 * ssl4gie_randaug_layer: ONE RandAugment layer, out = op[b] applied to in, per sample; in and out must not overlap.
 *   op uint8 [B], arg fp32 [B], matrix fp64 [B, 6] (read by the geometric ops only), fill: HOST array of 3 bytes.
 *   workspace: ssl4gie_randaug_layer_workspace_bytes(B) bytes (int32 [B, 4, 256]: the R, G, B and L histograms), zeroed
 *   by a memset node, then two launches: the histograms of the samples whose op reads them (ids 0, 1, 8; counts private to
 *   a workgroup in LDS, merged with integer atomics, so the result does not depend on arrival order), and the op.
 *   L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16.
 *   clip8(t) = 0 if t <= 0, 255 if t >= 255, else t truncated.  blend(d, v, f) = clip8(d + f (v - d)) in fp32, the
 *   product and the sum rounded one by one (Image.blend).  n = (int)arg.
 *     0 AutoContrast   per channel, lo / hi the lowest / highest level present: identity if hi <= lo, else
 *                      lut[i] = min(255, max(0, (int)(i s + o))), s = 255.0 / (hi - lo), o = -lo s, fp64
 *     1 Equalize       per channel: identity if at most one level is present; step = (S S - h[hi]) / 255 (integers);
 *                      identity if step == 0; else lut[i] = min(255, (step / 2 + h[0] + .. + h[i - 1]) / step)
 *     2 Invert         255 - v
 *     3 Rotate         the gather below; arg (degrees) is not read
 *     4 Posterize      n >= 8: v;  n <= 0: 0;  else v & ~(2^(8 - n) - 1)
 *     5 Solarize       v if v < n else 255 - v
 *     6 SolarizeAdd    min(255, v + n) if v < 128 else v
 *     7 Color          blend(L of the pixel, v, arg)
 *     8 Contrast       blend(m, v, arg), m = (int)(sum_i i hL[i] / (S S) + 0.5) in fp64, hL the L histogram
 *     9 Brightness     blend(0, v, arg)
 *    10 Sharpness      blend(SMOOTH(v), v, arg).  SMOOTH (ImageFilter.SMOOTH) on pixels not on the one-pixel border:
 *                      fp32, k1 = 1.f / 13.f, k5 = 5.f / 13.f, ss = 0.5f; ss += (a k1 + b k1) + c k1 over the row BELOW
 *                      (left, centre, right), then (a k1 + b k5) + c k1 over the pixel's row, then the row above as the
 *                      first; clip8(ss).  A border pixel is its own SMOOTH.
 *    11 ShearX, 12 ShearY, 13 TranslateX, 14 TranslateY, and 3: Image.transform(AFFINE, matrix, BICUBIC, fillcolor), fp64,
 *                      every operation rounded on its own:  xin = m0 (x + 0.5) + m1 (y + 0.5) + m2, yin likewise from
 *                      m3, m4, m5; unless 0 <= xin < S and 0 <= yin < S (so a NaN too) the pixel is `fill`; else
 *                      xin -= 0.5, x0 = floor(xin), dx = xin - x0 (y alike); taps x0 - 1 .. x0 + 2 and rows y0 - 1 .. y0 + 2,
 *                      indices clamped to [0, S - 1]; cubic(v1..v4, d): p1 = v2, p2 = -v1 + v3, p3 = 2 (v1 - v2) + v3 - v4,
 *                      p4 = -v1 + v2 - v3 + v4, r = p1 + d (p2 + d (p3 + d p4)); the four rows first (d = dx), then the
 *                      column (d = dy); clip8(r) — truncated, no + 0.5.  A coordinate is compared before it is clamped
 *                      and never addresses memory otherwise.
 *    any other id (255 = skip) copies the sample.
 *
 * ssl4gie_normalize_erase_u8: ToTensor + Normalize + timm's RandomErasing in one launch: img uint8 NHWC -> out fp32
 *   NCHW.  box int32 [B, 4] = (top, left, h, w).  Outside the box: fma(float(v), 1 / (255 std[c]), -mean[c] / std[c]),
 *   the bits of ssl4gie_normalize_u8.  h == 0 or w == 0: no erase.  Inside: mode SSL4GIE_ERASE_CONST 0.0;
 *   SSL4GIE_ERASE_PIXEL z(seed, b, c, y, x); SSL4GIE_ERASE_RAND z(seed, b, c, 0, 0).  A box that does not lie inside the
 *   image (a negative entry, top + h > S, left + w > S) makes its sample all NaN; the box is compared with coordinates
 *   and used for nothing else.  mean / std: HOST arrays of 3 floats.
 *   z: Philox4x32-10 (Salmon et al., SC'11; multipliers 0xD2511F53 on word 0 and 0xCD9E8D57 on word 2, key increments
 *   0x9E3779B9 and 0xBB67AE85) with counter (x, y, c, b) and key (seed & 0xffffffff, seed >> 32); k1, k2 = output words 0
 *   and 1 shifted right by 8; u = (k + 1) 2^-24 (exact in fp32, in (0, 1]); z = sqrtf(-2.f logf(u1)) cosf(6.2831855f u2).
 *   A pure function of (seed, b, c, y, x): the result does not depend on B or on the launch geometry.
 * SSL4GIE_EARG: a null pointer, S % 4 != 0, S < 4, S > 2048 (layer) or 16384, B < 0, B > 65535 (layer), in == out, a
 * pointer not 16-byte aligned, a std entry <= 0, an unknown mode.  B == 0 launches nothing. */
#define SSL4GIE_ERASE_CONST 0
#define SSL4GIE_ERASE_RAND 1
#define SSL4GIE_ERASE_PIXEL 2
int ssl4gie_quantize_u8(const float* x, unsigned char* out, int B, int S, void* stream);
size_t ssl4gie_randaug_layer_workspace_bytes(int B);
int ssl4gie_randaug_layer(const unsigned char* in, unsigned char* out, const unsigned char* op, const float* arg,
                          const double* matrix, const unsigned char* fill, void* workspace, int B, int S, void* stream);
int ssl4gie_normalize_erase_u8(const unsigned char* img, float* out, const float* mean, const float* std,
                               const int* box, int mode, unsigned long long seed, int B, int S, void* stream);

/* ---------------------------------------------------------------- detection pyramid glue (channels-last)
 * ViTDet_FPN (Models/models.py:213-259) around its GEMM-shaped convolutions:
 * maxpool2x2: nn.MaxPool2d(2) (:218); backward recomputes the window's first maximum from x.
 * gelu_map: nn.GELU (:241), exact erf form; dy != NULL gives dy * gelu'(x).
 * map_layernorm: nn.LayerNorm((C, H, W)) (:220-222 ...): per-image statistics over all M = H*W*C
 *   elements (biased variance, eps inside the sqrt) and a per-ELEMENT affine; w / bias / dw / db
 *   are fp32 [M] in the map's own (channels-last) element order.  mean / rstd [B] are kept for
 *   backward.  M % 8 == 0. */
int ssl4gie_maxpool2x2_fwd(const void* x, void* y, int dtype, int B, int H, int W, int C,
                           void* stream);
int ssl4gie_maxpool2x2_bwd(const void* x, const void* dy, void* dx, int dtype, int B, int H, int W,
                           int C, void* stream);
int ssl4gie_gelu_map(const void* x, const void* dy, void* out, int dtype, long long n, void* stream);
size_t ssl4gie_map_layernorm_workspace_bytes(int B);
int ssl4gie_map_layernorm_fwd(const void* x, const float* w, const float* bias, void* y, float* mean,
                              float* rstd, float eps, float* workspace, int dtype, int B, long long M,
                              void* stream);
int ssl4gie_map_layernorm_bwd(const void* x, const void* dy, const float* w, const float* mean,
                              const float* rstd, void* dx, float* dw, float* db, int accumulate,
                              float* workspace, int dtype, int B, long long M, void* stream);

/* ---------------------------------------------------------------- launch profiler (bench.py)
 * HIP events on the launch stream around every launch of the heavy kernels, used for the
 * `roofline` object of the bench line.  Process-global, not thread-safe, off by default.
 * kinds: 0 bf16 NT GEMM, 1 bf16 TN GEMM (kernel only, not its slab reduction), 2 fused attention
 * fwd, 3 fused attention bwd, 4 generic f32-MFMA GEMM.  flops are algorithmic (2MNK; attention
 * 4 B H N^2 hd forward, 10 B H N^2 hd backward). */
#define SSL4GIE_PROF_KINDS 7 /* 0 NT GEMM, 1 TN GEMM, 2 / 3 attention fwd / bwd, 4 generic GEMM (FLOPs); 5 BatchNorm, 6 LayerNorm (algorithmic BYTES in the `flops` slot) */
int ssl4gie_prof_begin(int max_launches);
int ssl4gie_prof_collect(double* ms, double* flops, long long* launches);
int ssl4gie_prof_end(void);

/* ---------------------------------------------------------------- finetune losses (value + gradient)
 * ScaleAndShiftInvariantLoss(alpha, scales) of the depth finetune step
 * (Depth_estimation/Metrics/losses.py:120-146; used at train_depth.py:43,280): pred, target fp32
 * [B, H, W] (the [B, 1, H, W] maps), valid pixels = target > 0.  Writes the scalar loss and
 * dpred = dloss/dpred (fp32 [B, H, W]) in five launches; deterministic two-stage reductions.
 * SoftDiceLoss(smooth) of the segmentation step (Binary_segmentation/Metrics/losses.py:5-24): logits,
 * target fp32 [B, n]; loss = 1 - mean_b 2 (sum s t + smooth) / (sum s^2 + sum t^2 + smooth),
 * s = sigmoid(logits); writes the loss and dlogits. */
size_t ssl4gie_ssi_loss_workspace_bytes(int B, int H, int W);
int ssl4gie_ssi_loss(const float* pred, const float* target, float* loss, float* dpred, int B, int H,
                     int W, float alpha, int scales, void* workspace, void* stream);
size_t ssl4gie_dice_loss_workspace_bytes(int B);
int ssl4gie_dice_loss(const float* logits, const float* target, float* loss, float* dlogits, int B,
                      long long n, float smooth, void* workspace, void* stream);

/* ---------------------------------------------------------------- loss heads of the pretraining / classification steps (ABI 10)
 * fp32 arithmetic, two-stage reductions in a fixed order (bit-identical from run to run), no atomics.
 *
 * InfoNCE of MoCo-v3 (Models/moco_v3/moco/builder.py:63-73, `MoCo.contrastive_loss`): q fp32 [N, C] (queries, the only
 * operand with a gradient), k fp32 [M, C] (the keys of all ranks, already gathered); row i's label is
 * label_offset + i.  q^ = q / max(||q||, 1e-12), k^ likewise, logits = q^ k^T / T (fp32 FMA chains, never stored),
 * loss = 2 T mean_i (logsumexp_j logits_ij - logits_i,label); dq (may be NULL) = dloss/dq through the normalisation.
 * The softmax is online (running maximum subtracted before every exp).  At most four launches.
 * SSL4GIE_EARG for N, M, C < 1, C > 1024, T <= 0, label_offset < 0 or label_offset + N > M.
 *
 * nn.CrossEntropyLoss(weight), mean reduction (Classification/train_classification.py:278): logits fp32 [B, C],
 * target int64 [B], weight fp32 [C] or NULL (all ones): loss = sum_i w[t_i] (lse_i - x_i,t_i) / sum_i w[t_i],
 * dlogits (may be NULL) = w[t_i] (p_ij - [j == t_i]) / sum w[t].  sum w[t] = 0 gives NaN, as torch does; a target
 * outside [0, C) is never used as an index: the loss and that row of dlogits are NaN.  Two launches.
 *
 * Barlow Twins loss terms on the reduced D x D fp32 correlation matrix c (ssl4gie_amd/Models/barlow_twins,
 * `cross_corr_loss_terms` and the operand casts of `CrossCorrLossFn.backward`):
 *   bt_loss       loss = sum_i (c_ii - 1)^2 + lambd sum_{i != j} c_ij^2 in one read of c (off-diagonal terms summed
 *                 directly; fp32 block partials, finished in fp64);
 *   bt_loss_grad  one read of c, both GEMM operands of the backward: w[i][j] = round_dtype(dc_ij s), wt[j][i] =
 *                 w[i][j], s = *scale (device scalar), dc_ij = c_ij (float)(2 lambd) off the diagonal and
 *                 2 (c_ii - 1) on it; every product rounded to fp32 in this order, so the operands equal the torch
 *                 ops' bit for bit.  dtype = SSL4GIE_BF16 | SSL4GIE_F32.  One launch. */
size_t ssl4gie_infonce_workspace_bytes(int N, int M, int C);
int ssl4gie_infonce_loss(const float* q, const float* k, float* loss, float* dq, int N, int M, int C, float T,
                         int label_offset, void* workspace, void* stream);
size_t ssl4gie_cross_entropy_workspace_bytes(int B, int C);
int ssl4gie_cross_entropy(const float* logits, const long long* target, const float* weight, float* loss,
                          float* dlogits, int B, int C, void* workspace, void* stream);
/* soft-target cross-entropy (timm's SoftTargetCrossEntropy / LabelSmoothingCrossEntropy, main_finetune.py:292-294;
 * joined ABI 12 as an addition): loss = mean_b sum_c -t[b,c] log_softmax(x[b])[c], dlogits (may be NULL) =
 * (softmax(x[b]) sum_c t[b,c] - t[b]) / B.  Exactly one of soft_target fp32 [B, C] and label int64 [B] is given; with a
 * label t[b,c] = conf [c == label_b] + off (conf = 1 - smoothing, off = smoothing / C), and a label outside [0, C) is
 * never an index: the loss and that row of dlogits are NaN.  One wave per row, per-block partials summed in fp64 in a
 * fixed order, no atomics.  Two launches. */
size_t ssl4gie_soft_cross_entropy_workspace_bytes(int B, int C);
int ssl4gie_soft_cross_entropy(const float* logits, const float* soft_target, const long long* label,
                               float conf, float off, float* loss, float* dlogits, int B, int C,
                               void* workspace, void* stream);
size_t ssl4gie_bt_loss_workspace_bytes(int D);
int ssl4gie_bt_loss(const float* c, float* loss, int D, float lambd, void* workspace, void* stream);
int ssl4gie_bt_loss_grad(const float* c, const float* scale, void* w, void* wt, int dtype, int D, float lambd,
                         void* stream);

/* ---------------------------------------------------------------- evaluation metrics (joined ABI 12)
 * The `test()` loops and eval_*.py CLIs of the three finetune heads.  Integer counts by integer atomics (order-free),
 * floating sums as per-block partials added in a fixed order in fp64, no float atomics: bit-identical from run to run.
 * No allocation, no host synchronisation; every output stays on the device.
 *
 * seg_counts   the thresholding shared by DiceScore / IoU / Precision / Recall (Binary_segmentation/Metrics/
 *              performance.py:13-19, :38-44, :61-67, :82-88): counts int64 [B, 3] = (|m1|, |m2|, |m1 & m2|) per image,
 *              m1 = probs > 0.5, m2 = target > 0.5.  logits [B, Hin, Win] of logits_dtype (SSL4GIE_F32 / SSL4GIE_BF16),
 *              target [B, H, W] of target_dtype (SSL4GIE_TGT_U8 / SSL4GIE_TGT_F32).  Where (Hin, Win) != (H, W) the
 *              logits are resampled per target pixel and never stored: F.interpolate(mode = "bilinear", align_corners =
 *              False) without antialiasing, in fp32 — TF.resize of a tensor at eval_segmentation.py:36-37.  sigmoid != 0:
 *              m1 = logit > 0 (the reference's fp32 sigmoid(x) > 0.5 is false for 0 < x <~ 1.2e-7 as well: DESIGN.md
 *              section 8); sigmoid == 0: m1 = logit > 0.5.  counts is overwritten.  H * W and Hin * Win < 2^31.
 * seg_scores   scores fp32 [4] = batch means of Dice, IoU, precision, recall from counts, each by the reference's fp32
 *              formula in its operation order (performance.py:21-26, :46-49, :69-70, :90-91; an empty prediction on an
 *              empty target scores 2, 1, 1, 1 as there); the sum over the images in fp64.  accum (fp64 [5] or NULL):
 *              accum[0..3] += the four per-image sums, accum[4] += B, in the same launch.
 * confusion_update  conf int64 [C, C] (row = target, column = prediction) += the batch's counts.  input: logits [B, C]
 *              (SSL4GIE_F32 / SSL4GIE_BF16; the prediction is the first maximum, a NaN counting as the largest value:
 *              torch.argmax at Classification/train_classification.py:93,96) or predictions int64 [B]
 *              (SSL4GIE_PRED_I64); target int64 [B].  A target or prediction outside [0, C) is never used as an index:
 *              *rejected (int64) += 1 and the matrix is left alone.
 * confusion_scores  scores fp32 [4] = mean F1, mean precision, mean recall (Classification/Metrics/performance.py:10-22,
 *              :31-39, :48-56: per class tp = conf[i][i], |m1| = column sum, |m2| = row sum, every term in fp32 as the
 *              reference forms it — a class absent from predictions and targets adds 2, 1, 1 —, added in class order in
 *              fp32 as its loops add them, / C: the reference's means bit for bit) and accuracy = trace / total.
 * lower_median_f32  out = the element of rank (n - 1) / 2 of x fp32 [n]: torch.median's lower median
 *              (Depth_estimation/eval_depth.py:24).  Exact: a radix select on the bit pattern (three histogram passes,
 *              11 + 11 + 10 bits, the bin picked on the device), so x must hold non-negative values (sign bit clear;
 *              +inf allowed) — any other entry gives an unspecified, but safe, result.  x is not modified.  n == 0: NaN.
 *              workspace: ssl4gie_lower_median_workspace_bytes() bytes.
 * depth_eval   out fp32 [B, 3] = (rmse, rel_err, abs_err) per image as eval_depth.py:43-61 computes them: pred, target
 *              fp32 [B, S, S] (Sh == Sw), target_og fp32 [B, H, W] (not modified; the reference scales it in place).
 *              (scale, shift) = the 2 x 2 least squares of compute_scale_and_shift over target > 0, sums and solve in
 *              fp64, det == 0 -> (0, 0); one pass over the H x W stored pixels evaluates scale * pred + shift (fp32)
 *              resampled bilinearly (align_corners = False, no antialiasing) to M x M, M = max(H, W), cropped at
 *              torchvision's centre-crop offsets int(round((M - H) / 2.0)), int(round((M - W) / 2.0)) (half to even),
 *              clamped to [0, 1], zero where target_og == 0, both sides times scale_; valid = target_og * scale_ > 0;
 *              rmse = sqrt(mean d^2), abs_err = mean |d| (fp64 sums), rel_err = lower median of |d / t| by the select
 *              above.  An image without a valid pixel gives three NaNs.  workspace: 16-byte aligned,
 *              ssl4gie_depth_eval_workspace_bytes(B, S, H, W) bytes (0 for an invalid shape).
 * SSL4GIE_EARG: a null pointer, B, C or a size <= 0, an unknown dtype / kind, Sh != Sw, B > 65535 (per-image grids). */
#define SSL4GIE_PRED_I64 2
int ssl4gie_seg_counts(const void* logits, int logits_dtype, const void* target, int target_dtype, long long* counts,
                       int B, int Hin, int Win, int H, int W, int sigmoid, void* stream);
int ssl4gie_seg_scores(const long long* counts, int B, float smooth, float* scores, double* accum, void* stream);
int ssl4gie_confusion_update(const void* input, int input_kind, const long long* target, long long* conf,
                             long long* rejected, int B, int C, void* stream);
int ssl4gie_confusion_scores(const long long* conf, int C, float smooth, float* scores, void* stream);
size_t ssl4gie_lower_median_workspace_bytes(void);
int ssl4gie_lower_median_f32(const float* x, long long n, float* out, void* workspace, void* stream);
size_t ssl4gie_depth_eval_workspace_bytes(int B, int S, int H, int W);
int ssl4gie_depth_eval(const float* pred, const float* target, const float* target_og, float* out, int B, int Sh,
                       int Sw, int H, int W, float scale_, void* workspace, void* stream);

/* ---------------------------------------------------------------- detection metric: COCO mAP (joined ABI 12)
 * Object_detection/train_detection.py:113-151 (`test()`, every epoch) and Object_detection/eval_detection.py:21-44 score
 * the detector with torchmetrics.detection.mean_ap.MeanAveragePrecision() (torchmetrics 1.1.2, requirements.txt:9:
 * pycocotools' COCOeval with the default 10 IoU thresholds, 101 recall thresholds, maxDets (1, 10, 100) and the four
 * area ranges) and read ["map"], ["map_50"], ["map_75"].  The rule is written out in ssl4gie_amd/metrics.py
 * (MeanAveragePrecision); csrc/det_map_ops.hip has the kernels.  All detections of a loader lie end to end: det_boxes
 * fp32 [n_det, 4] (xyxy), det_scores fp32 [n_det], det_labels int64 [n_det], image i owning [det_off[i], det_off[i + 1])
 * (det_off, gt_off: int32 [n_img + 1] on the device); gt_boxes fp32 [n_gt, 4], gt_labels int64 [n_gt] likewise.
 *
 * match       one workgroup per image.  rank int32 [n_det]: the stable rank of a detection among the same-label
 *             detections of its image (descending score, insertion order on ties); a rank >= 100 is dropped, and a
 *             detection with a label outside [0, 255] gets rank 1024.  matched / ignored uint64 [n_det]: bit
 *             (area * 10 + threshold) of COCOeval.evaluateImg's dtm != 0 / dtIg, areas in the order all, small, medium,
 *             large, thresholds = iou_thresholds (HOST array of 10 doubles; torch.linspace(0.5, 0.95, 10).tolist()); 0
 *             for a dropped detection.  npig int32 [256, 4]: non-ignored ground truths per class and area; present
 *             int32 [256]: 1 for a class seen in a detection or a ground truth; flag int32 [1]: bit 0 = a label outside
 *             [0, 255] (such an entry takes no part), bit 1 = offsets that are not ascending, leave [0, n] or give an
 *             image more than 1024 entries (such an image is skipped; nothing is read through its offsets).  The three
 *             are zeroed first.  Width and height are fp32 differences; every decision after that is fp64, uncontracted
 *             (csrc/Makefile builds det_map_ops.hip with -ffp-contract=off: -ffp-contract=fast disregards the pragma).
 * order       sorted_idx uint32 [n_det]: the first seg_off[256] entries are the kept detections (rank < 100, label in
 *             range) stably sorted by (label ascending, score descending; -0 == +0), ties in insertion order; seg_off
 *             int32 [257]: class c owns [seg_off[c], seg_off[c + 1]).  A least-significant-digit radix sort, five 8-bit
 *             passes, 15 launches; workspace: 16-byte aligned, ssl4gie_det_map_workspace_bytes(n_img, n_det, n_gt) bytes
 *             (0 where a size is <= 0 or a total exceeds SSL4GIE_DET_MAP_MAX_TOTAL; the size depends on n_det alone).
 * accumulate  COCOeval.accumulate for the six (area, maxDet) pairs the summaries read — (all, 100), (small, 100),
 *             (medium, 100), (large, 100), (all, 1), (all, 10) — one workgroup per (class, pair, threshold): stats fp64
 *             [256, 6, 10, 2] = (sum of the 101 interpolated precisions, final recall), -1 where the class has no
 *             non-ignored ground truth in the area, untouched for a class not present; rec_thresholds: HOST array of 101
 *             doubles (torch.linspace(0, 1, 101).tolist()).  Then COCOeval.summarize: out64 fp64 [12] / out32 fp32 [12]
 *             (the same values rounded) = map, map_50, map_75, map_small, map_medium, map_large, mar_1, mar_10, mar_100,
 *             mar_small, mar_medium, mar_large (the mean over the entries > -1, -1 without any); outi int32 [258] =
 *             number of classes, flag word, the classes ascending (-1 beyond).  With n_det == 0 (or no ground truth)
 *             skip `order` and pass a zeroed seg_off.
 * SSL4GIE_EARG: a null pointer (those of an empty side excepted), n_img <= 0, a negative count, a total above
 * SSL4GIE_DET_MAP_MAX_TOTAL, n_det <= 0 for `order`. */
#define SSL4GIE_DET_MAP_MAX_PER_IMAGE 1024
#define SSL4GIE_DET_MAP_CLASSES 256
#define SSL4GIE_DET_MAP_CHUNK 256            /* detections per scan step of `accumulate` */
#define SSL4GIE_DET_MAP_MAX_TOTAL (1 << 24)
size_t ssl4gie_det_map_workspace_bytes(int n_img, long long n_det, long long n_gt);
int ssl4gie_det_map_match(const float* det_boxes, const float* det_scores, const long long* det_labels,
                          const int* det_off, const float* gt_boxes, const long long* gt_labels, const int* gt_off,
                          int n_img, long long n_det, long long n_gt, const double* iou_thresholds, int* rank,
                          unsigned long long* matched, unsigned long long* ignored, int* npig, int* present, int* flag,
                          void* stream);
int ssl4gie_det_map_order(const float* det_scores, const long long* det_labels, const int* rank, long long n_det,
                          unsigned* sorted_idx, int* seg_off, void* workspace, void* stream);
int ssl4gie_det_map_accumulate(const unsigned* sorted_idx, const int* seg_off, const int* rank,
                               const unsigned long long* matched, const unsigned long long* ignored, const int* npig,
                               const int* present, const int* flag, long long n_det, const double* rec_thresholds,
                               double* stats, double* out64, float* out32, int* outi, void* stream);

/* ---------------------------------------------------------------- Faster R-CNN heads: NMS, box decode, RoIAlign (joined ABI 12)
 * Object_detection/train_detection.py:244-250 and Object_detection/eval_detection.py build
 * torchvision.models.detection.faster_rcnn.FasterRCNN(backbone, num_classes=...); its proposal and detection stages run
 * torchvision's C++ / CUDA ops.  The rules (torchvision 0.10's published source) are written out in
 * ssl4gie_amd/Models/detection.py; csrc/det_head_ops.hip has the kernels, built with -ffp-contract=off.
 *
 * nms_segments  replaces torchvision.ops.nms / batched_nms (rpn.py filter_proposals, roi_heads.py postprocess_detections).
 *               boxes fp32 [n, 4] xyxy, 16-byte aligned, sorted by descending score inside every segment (ties: lower
 *               original index first); segment s owns [seg_off[s], seg_off[s + 1]) (int32 [n_seg + 1] on the device);
 *               valid uint8 [n] or NULL: a box with valid == 0 is never kept and suppresses nothing.  In fp32, inter =
 *               max(0, xx2 - xx1) * max(0, yy2 - yy1), iou = inter / (area_i + area_j - inter); box j is dropped when
 *               iou > thr against a kept box i earlier in its segment.  keep_rank int32 [n]: the position of a kept box
 *               among the kept boxes of its segment, -1 for a dropped one or one outside every segment; count int32
 *               [n_seg].  max_seg: an upper bound of the segment sizes known on the host, <= 4096; of a longer segment
 *               only the first max_seg boxes take part.  Nothing is read through offsets that are not ascending or leave
 *               [0, n] (count 0).  workspace: 8-byte aligned, ssl4gie_nms_workspace_bytes(n, max_seg) bytes (a 64-bit word per box and
 *               64 boxes of max_seg; 0 for n <= 0, n > SSL4GIE_NMS_MAX_TOTAL or max_seg outside [1, 4096]).  No host round trip: torchvision's CUDA nms sweeps its mask on the host.
 * rpn_decode    replaces, for the top-k candidates of every (image, level), AnchorGenerator + BoxCoder.decode_single
 *               (weights 1) + clip_boxes_to_image + remove_small_boxes + sigmoid + the score test of
 *               RegionProposalNetwork.filter_proposals.  head / grids / k_off / base_anchors are HOST arrays: head[l] the
 *               device pointer of level l's fp32 head output [B * grid * grid, ld] (columns [0, A) objectness logits,
 *               [A + 4 a, A + 4 a + 4) the deltas of anchor a), grids[l] its side, candidates [k_off[l], k_off[l + 1]) of
 *               an image belong to level l, base_anchors [L, A, 4] the level's base anchors (round([-w, -h, w, h] / 2));
 *               the anchor of flat index (y * grid + x) * A + a is base + (x, y, x, y) * (F / grid).  topk_idx int64
 *               [B, k_off[L]]: flat indices inside the level (one outside gives a zero box, valid 0).  Outputs boxes fp32
 *               [B * k_off[L], 4], scores fp32 (sigmoid), valid uint8 = w >= min_size && h >= min_size && score >=
 *               score_thresh.  dw, dh are clamped at log(1000 / 16); boxes are clamped to [0, F]^2.
 * roi_decode    replaces RoIHeads.postprocess_detections up to the NMS: proposals fp32 [K, 4], logits rows of C at
 *               ld_logits, deltas rows of 4 C at ld_deltas, weights (wx, wy, ww, wh); boxes fp32 [K, C - 1, 4], scores
 *               fp32 [K, C - 1] (row softmax, background column 0 dropped), valid uint8 [K, C - 1].
 * roi_align     replaces MultiScaleRoIAlign(["0", "1", "2", "3"], 7, 2) (aligned=False, sampling_ratio 2) and its
 *               backward.  maps / map_hw / scales are HOST arrays of the four levels: device pointers of channels-last
 *               fp32 maps [B, H, W, C], (H, W) pairs, spatial scales.  rois fp32 [K, 4] in image coordinates, roi_batch
 *               int32 [K] (a RoI with an image index outside [0, B) gives zeros / adds nothing).  Level per RoI on the
 *               device: floor(4 + log2(sqrt(area) / 224) + 1e-6) clamped to [2, 5]; levels int32 [K] (0 .. 3) or NULL.
 *               fwd writes [K, C * 49] in (c, ph, pw) order in out_dtype.  bwd ADDS into dmaps (zeroed by the caller)
 *               with float atomics: not bitwise reproducible.  C: a multiple of 64, and of 256 above 256.
 * SSL4GIE_EARG: a null pointer, a size <= 0 or above the caps, a misaligned pointer. */
#define SSL4GIE_NMS_MAX_PER_SEGMENT 4096
#define SSL4GIE_NMS_MAX_TOTAL (1 << 24)
#define SSL4GIE_RPN_MAX_LEVELS 8
#define SSL4GIE_RPN_MAX_ANCHORS 3
size_t ssl4gie_nms_workspace_bytes(long long n, int max_seg);
int ssl4gie_nms_segments(const float* boxes, const unsigned char* valid, const int* seg_off, int n_seg, long long n,
                         int max_seg, float thr, int* keep_rank, int* count, void* workspace, void* stream);
int ssl4gie_rpn_decode(const float* const* head, const int* grids, const int* k_off, const float* base_anchors, int L,
                       int A, int ld, const long long* topk_idx, int B, int F, float min_size, float score_thresh,
                       float* boxes, float* scores, unsigned char* valid, void* stream);
int ssl4gie_roi_decode(const float* proposals, const float* logits, int ld_logits, const float* deltas, int ld_deltas,
                       int K, int C, float wx, float wy, float ww, float wh, float W, float H, float min_size,
                       float score_thresh, float* boxes, float* scores, unsigned char* valid, void* stream);
int ssl4gie_roi_align_fwd(const float* const* maps, const int* map_hw, const float* scales, int B, int C,
                          const float* rois, const int* roi_batch, int K, void* out, int out_dtype, int* levels,
                          void* stream);
int ssl4gie_roi_align_bwd(float* const* dmaps, const int* map_hw, const float* scales, int B, int C, const float* rois,
                          const int* roi_batch, int K, const void* dy, int dy_dtype, void* stream);

/* ---------------------------------------------------------------- direct xGMI gradient all-reduce
 * replaces the NCCL bucket all-reduce of DistributedDataParallel (Models/mae/main_pretrain.py:175,
 * Depth_estimation/train_depth.py:226-229, Models/moco_v3/main_moco.py:208) for ONE node of up to 8
 * fully connected GPUs: every rank pushes chunk p of a bucket straight into peer p's memory
 * (reduce-scatter), the owners push the reduced chunks back (all-gather) — one hop, all 7 links at
 * once, instead of a ring bound by one link.  csrc/allreduce.hip has the protocol.
 *   init     allocates this rank's exchange region (the ONE allocation this interface makes; sized for
 *            buckets of up to max_elems fp32) and writes ssl4gie_allreduce_direct_blob_bytes() bytes
 *            of IPC description to export_blob; the caller exchanges the blobs of all ranks by any
 *            out-of-band means (ssl4gie_amd.parallel: torch.distributed.all_gather_object);
 *   connect  maps the peers' regions from the `world` blobs laid end to end in rank order;
 *   enqueue  grad[0 .. n_elems) <- scale * sum over ranks, in place, on `stream` (5 launches, no host
 *            synchronisation).  Every rank must enqueue the same sequence of sizes; sums run in rank
 *            order on every rank, so all ranks end with bitwise identical values;
 *   error    the handle's sticky error word: 0, or (sequence number << 8 | 1 + peer rank) of the first
 *            bucket in which a waiting kernel gave up on a peer (bounded poll: 10 min by default, SSL4GIE_AR_TIMEOUT_S
 *            or set_timeout).  Such a kernel writes NaN instead of stale sums; from then on enqueue
 *            returns SSL4GIE_EPEER (1001) and ssl4gie_amd.parallel.DataParallel raises.  Read without
 *            synchronising (mapped host memory);
 *   destroy  unmaps / frees (after the streams that used the handle have drained).
 * init fails (hipError_t) when fine-grained device memory is not available: peer stores and in-kernel
 * flag polls are not coherent on coarse-grained memory, so there is no fallback to it. */
typedef struct ssl4gie_ar_handle ssl4gie_ar_handle;
size_t ssl4gie_allreduce_direct_blob_bytes(void);
int ssl4gie_allreduce_direct_init(int rank, int world, size_t max_elems, void* export_blob,
                                  ssl4gie_ar_handle** out);
int ssl4gie_allreduce_direct_connect(ssl4gie_ar_handle* h, const void* all_blobs);
int ssl4gie_allreduce_direct_enqueue(ssl4gie_ar_handle* h, float* grad, size_t n_elems, float scale,
                                     void* stream);
/* All-gather of n_elems floats per rank over the same handle (n_elems <= ceil(max_elems / world)):
 * dst[w * n_elems + i] = rank w's src[i], in rank order on every rank; 3 launches, no host synchronisation.
 * Carries nn.SyncBatchNorm's per-layer (mean, var, count) exchange and its backward sums
 * (reference Models/moco_v3/main_moco.py:196, Depth_estimation/train_depth.py:225) without an RCCL launch;
 * use a handle of its own per stream (calls on one handle are ordered by the stream they are enqueued on). */
int ssl4gie_allgather_direct_enqueue(ssl4gie_ar_handle* h, const float* src, size_t n_elems, float* dst,
                                     void* stream);
unsigned ssl4gie_allreduce_direct_error(const ssl4gie_ar_handle* h);
int ssl4gie_allreduce_direct_set_timeout(ssl4gie_ar_handle* h, double seconds);
int ssl4gie_allreduce_direct_destroy(ssl4gie_ar_handle* h);

#ifdef __cplusplus
}
#endif
#endif
