// What the channels-last map kernels (dpt_ops, resnet_ops, det_ops, atrous_ops) share: the 16-byte chunk of
// channels <-> fp32 registers, the align-corners source index, the entry points' argument tests and the dtype
// dispatch of a launch.  A new map kernel takes these from here.
#pragma once
#include "common.h"
#include "ssl4gie_hip.h"

// ---- 16 bytes of T (bf16_t: 8 channels, float: 4) as a raw register value, and as fp32 registers
template <typename T> struct V16;
template <> struct V16<bf16_t> { static constexpr int N = 8; typedef u32x4 raw; };
template <> struct V16<float> { static constexpr int N = 4; typedef f32x4 raw; };
template <typename T> DEVI void un(const typename V16<T>::raw& r, float (&f)[V16<T>::N]);
template <> DEVI void un<bf16_t>(const u32x4& r, float (&f)[8]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f[2 * j] = __uint_as_float(r[j] << 16);
        f[2 * j + 1] = __uint_as_float(r[j] & 0xffff0000u);
    }
}
template <> DEVI void un<float>(const f32x4& r, float (&f)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) f[j] = r[j];
}
template <typename T> DEVI typename V16<T>::raw pk(const float (&f)[V16<T>::N]);
template <> DEVI u32x4 pk<bf16_t>(const float (&f)[8]) {
    u32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = pack_bf2(f[2 * j], f[2 * j + 1]);
    return r;
}
template <> DEVI f32x4 pk<float>(const float (&f)[4]) { return f32x4{f[0], f[1], f[2], f[3]}; }

// ---- the pointer form, for kernels that also come in a one-channel width: V = V16<T>::N or 1
template <typename T, int V> struct Chunk {
    static_assert(V == V16<T>::N, "a chunk is 16 bytes or one element");
    static DEVI void ld(const T* p, float (&f)[V]) { un<T>(*(const typename V16<T>::raw*)p, f); }
    static DEVI void st(T* p, const float (&f)[V]) { *(typename V16<T>::raw*)p = pk<T>(f); }
};
template <typename T> struct Chunk<T, 1> {
    static DEVI void ld(const T* p, float (&f)[1]) { f[0] = Elem<T>::ld(p); }
    static DEVI void st(T* p, const float (&f)[1]) { Elem<T>::st(p, f[0]); }
};

// ---- bilinear taps of output index d with align_corners=True: src = d (n_in - 1) / (n_out - 1) in fp32, as ATen's
// area_pixel_compute_source_index does; a one-pixel input has scale 0 (constant map)
DEVI void ac_src(int d, int n_in, int n_out, int& i0, int& i1, float& w1) {
    const float scale = n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : 0.f;
    const float s = scale * (float)d;
    i0 = (int)s;
    i0 = i0 < n_in - 1 ? i0 : n_in - 1;
    i1 = i0 + 1 < n_in ? i0 + 1 : n_in - 1;
    w1 = s - (float)i0;
}

// ---- host side of an entry point
static inline bool dt_ok(int dt) { return dt == SSL4GIE_F32 || dt == SSL4GIE_BF16; }
static inline int vecn(int dt) { return dt == SSL4GIE_BF16 ? 8 : 4; }   // V16<T>::N of the dtype
static inline bool is16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static inline unsigned blocks_of(long long total) { return (unsigned)((total + 255) / 256); }   // of 256 threads

// KERNEL<bf16_t> or KERNEL<float> by dtype on the stream `st` of the calling scope; T names the element type in the
// argument list, for the pointer casts
#define MAP_LAUNCH(dtype, KERNEL, grid, block, ...)                                 \
    do {                                                                            \
        if ((dtype) == SSL4GIE_BF16) {                                              \
            typedef bf16_t T;                                                       \
            hipLaunchKernelGGL(KERNEL<T>, grid, block, 0, st, __VA_ARGS__);         \
        } else {                                                                    \
            typedef float T;                                                        \
            hipLaunchKernelGGL(KERNEL<T>, grid, block, 0, st, __VA_ARGS__);         \
        }                                                                           \
        LAUNCH_CHECK();                                                             \
    } while (0)
// the same for a KERNEL<T, V>: V = V16<T>::N when `wide`, else 1
#define MAP_LAUNCH_V(dtype, wide, KERNEL, grid, block, ...)                         \
    do {                                                                            \
        if ((dtype) == SSL4GIE_BF16) {                                              \
            typedef bf16_t T;                                                       \
            if (wide) hipLaunchKernelGGL((KERNEL<T, 8>), grid, block, 0, st, __VA_ARGS__); \
            else hipLaunchKernelGGL((KERNEL<T, 1>), grid, block, 0, st, __VA_ARGS__);      \
        } else {                                                                    \
            typedef float T;                                                        \
            if (wide) hipLaunchKernelGGL((KERNEL<T, 4>), grid, block, 0, st, __VA_ARGS__); \
            else hipLaunchKernelGGL((KERNEL<T, 1>), grid, block, 0, st, __VA_ARGS__);      \
        }                                                                           \
        LAUNCH_CHECK();                                                             \
    } while (0)
