// On-device geometric stage of the finetune loaders: the image and its target through ONE nearest-neighbour map.
//
// What it stands in for, per sample, on the normalised fp32 tensor and its target (mask or depth map):
//   Binary_segmentation/Data/dataset.py:46-63   TF.hflip / TF.vflip (each on a coin), then TF.affine(angle,
//                                               translate, scale, shear, fill = -1.0 | 0.0), nearest
//   Depth_estimation/Data/dataset.py:47-70      the two flips alone
//   Classification/Data/dataloaders.py:67-69    RandomHorizontalFlip, RandomVerticalFlip, RandomRotation(180)
// Flips and a nearest-neighbour affine only permute or drop pixels, so they commute with Normalize (only the fill
// changes) and compose into one gather.
//
// The rule, sample b, output pixel (i, j), c = (S - 1) / 2, xo = j - c, yo = i - c, m = matrix[b] (the INVERSE map,
// torchvision's _get_inverse_affine_matrix; NULL = identity):
//   sx = m0 xo + m1 yo + m2 + c,  sy = m3 xo + m4 yo + m5 + c,  ix = rint(sx), iy = rint(sy)  (half to even:
//   grid_sample(mode = "nearest", align_corners = False) on _gen_affine_grid);
//   (ix, iy) outside [0, S)^2: the pixel is the fill (fill_img[ch], fill_tgt);
//   otherwise the source index is mirrored where the flip bits say so (bit 0: ix <- S - 1 - ix, bit 1: iy <- S - 1 -
//   iy; the reference flips BEFORE the affine, so the flip applies to the source), and the pixel is the source value.
// The target of sample b is tgt_bank[index[b]] (u8 / 255, u16 / 65535 or fp32 as it is); an index outside [0, n)
// gives an all-NaN target and no address is formed from it.
//
// sx, sy are evaluated in fp32 (one multiply, two fused multiply-adds): at |coordinate| < 512 that is within 1e-4 of
// the exact value, so only pixels whose source coordinate lies that close to a half-integer can land on the
// neighbouring source pixel (torchvision's own fp32 grid has the same property).
//
// One lane = 4 neighbouring output pixels of a row, all three channels and the target: the index arithmetic is done
// once for the 4 planes, the stores are 16 bytes per lane and coalesced, the loads are a gather inside ONE sample
// (588 KB of image + at most 196 KB of target at S = 224: L2 serves the re-reads of a rotated row's cache lines).
// A workgroup never spans two samples, so the matrix, flip bits and index are uniform.  Plain vector loads and stores.
#include "common.h"
#include "ssl4gie_hip.h"

#define PW_THREADS 256

DEVI float pw_target(const void* __restrict__ bank, int dtype, size_t off) {
    switch (dtype) {  // (uniform)
    // true divisions, as ToTensor's and the depth loader's: v * (1 / 255) is another fp32 number for 126 of the 256 levels
    case SSL4GIE_TGT_U8: return (float)((const unsigned char*)bank)[off] / 255.f;
    case SSL4GIE_TGT_U16: return (float)((const unsigned short*)bank)[off] / 65535.f;
    default: return ((const float*)bank)[off];
    }
}

__global__ __launch_bounds__(PW_THREADS) void paired_warp_kernel(
    const float* __restrict__ img, float* __restrict__ img_out, const void* __restrict__ tgt_bank, int tgt_dtype,
    long long n, const long long* __restrict__ index, float* __restrict__ tgt_out, const float* __restrict__ matrix,
    const unsigned char* __restrict__ flip, f32x4 fill, int S, int blocks_per_sample) {
    const int b = blockIdx.x / blocks_per_sample;
    const int g = (blockIdx.x - b * blocks_per_sample) * PW_THREADS + threadIdx.x;
    const int S4 = S >> 2;
    if (g >= S * S4) return;
    const int i = g / S4, j0 = 4 * (g - i * S4);
    const size_t plane = (size_t)S * S;

    float m0 = 1.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 1.f, m5 = 0.f;
    if (matrix) {
        const float* m = matrix + 6 * (size_t)b;
        m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5];
    }
    const int fl = flip ? flip[b] : 0;
    const float c = 0.5f * (float)(S - 1), yo = (float)i - c, top = (float)(S - 1);
    const float bx = m1 * yo + m2 + c, by = m4 * yo + m5 + c;

    int off[4];  // source offset inside a plane, -1 = fill
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float xo = (float)(j0 + k) - c;
        const float fx = rintf(m0 * xo + bx), fy = rintf(m3 * xo + by);
        // compared as floats: a NaN or a huge coordinate is "outside" and is never converted to an index
        const bool in = fx >= 0.f && fx <= top && fy >= 0.f && fy <= top;
        int ix = in ? (int)fx : 0, iy = in ? (int)fy : 0;
        ix = (fl & 1) ? S - 1 - ix : ix;
        iy = (fl & 2) ? S - 1 - iy : iy;
        off[k] = in ? iy * S + ix : -1;
    }

    const float* src = img + (size_t)b * 3 * plane;
    float* dst = img_out + (size_t)b * 3 * plane + (size_t)i * S + j0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float f = ch == 0 ? fill[0] : ch == 1 ? fill[1] : fill[2];
        f32x4 v;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = off[k] >= 0 ? src[ch * plane + (size_t)off[k]] : f;
        st4(dst + ch * plane, v);
    }
    if (tgt_out) {
        const long long idx = index[b];
        f32x4 v = {NAN, NAN, NAN, NAN};
        if (idx >= 0 && idx < n) {  // (uniform) otherwise no address is formed from the index
            const size_t base = (size_t)idx * plane;
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = off[k] >= 0 ? pw_target(tgt_bank, tgt_dtype, base + (size_t)off[k]) : fill[3];
        }
        st4(tgt_out + (size_t)b * plane + (size_t)i * S + j0, v);
    }
}

extern "C" int ssl4gie_paired_warp(const float* img, float* img_out, const void* tgt_bank, int tgt_dtype, long n,
                                   const int64_t* index, float* tgt_out, const float* matrix, const uint8_t* flip,
                                   const float* fill_img, float fill_tgt, int B, int S, void* stream) {
    REQUIRE(img && img_out && fill_img);
    REQUIRE(B >= 0 && S >= 4 && S % 4 == 0 && (long long)S * S <= 0x7fffffffLL);
    REQUIRE(((uintptr_t)img | (uintptr_t)img_out | (uintptr_t)tgt_out) % 16 == 0);  // 16-byte stores
    const size_t count = (size_t)B * 3 * S * S;
    REQUIRE(!(img_out < img + count && img < img_out + count));  // a gather cannot run in place
    if (tgt_bank || tgt_out || index) {  // the target comes as a whole or not at all
        REQUIRE(tgt_bank && tgt_out && index && n >= 1);
        REQUIRE(tgt_dtype == SSL4GIE_TGT_U8 || tgt_dtype == SSL4GIE_TGT_U16 || tgt_dtype == SSL4GIE_TGT_F32);
    }
    const int per = S * (S / 4), blocks = (per + PW_THREADS - 1) / PW_THREADS;
    REQUIRE((long long)B * blocks <= 0x7fffffffLL);
    if (B == 0) return 0;
    const f32x4 fill = {fill_img[0], fill_img[1], fill_img[2], fill_tgt};
    hipLaunchKernelGGL(paired_warp_kernel, dim3((unsigned)(B * blocks)), dim3(PW_THREADS), 0, (hipStream_t)stream, img,
                       img_out, tgt_bank, tgt_dtype, (long long)n, (const long long*)index, tgt_out, matrix, flip, fill, S,
                       blocks);
    LAUNCH_CHECK();
    return 0;
}
