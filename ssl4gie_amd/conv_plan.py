"""conv3x3_plan: the one place where a Conv2d(k=3, pad=1) layer's kernels are chosen (dpt_engine.Conv3x3Fn executes it).
Families: "direct" = the halo-in-LDS kernels of conv_direct.hip; "gather" = the 256x256 GEMMs that gather the patch
matrix in the kernel (ops.conv3x3_fwd / conv3x3_bwd_weight); "im2col" = a materialised patch matrix through the plain
GEMMs ("col2im": its transpose, the stride-2 data gradient).  LIMITS say what a kernel can take (one function per family,
named after the C check it mirrors), PREFERENCES where it is ahead.  Integers and a dtype only, never a tensor."""
import collections
import functools

import torch

from . import _lib


def conv_out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def k_pad(k, dtype):
    """row stride of a patch matrix: the bf16 MFMA GEMM wants whole 64-deep K-tiles"""
    return (k + 63) // 64 * 64 if dtype == torch.bfloat16 else k


# ------------------------------------------------------------------------------------------------------------- limits
def direct_fwd_ok(B, H, W, Cin, Cout, dtype):
    """ssl4gie_conv3x3_direct_ok: the direct kernel CAN take this stride-1 map (bf16, Cin % 32 == 0, Cout % 8 == 0)"""
    return dtype == torch.bfloat16 and bool(_lib.load().ssl4gie_conv3x3_direct_ok(B, H, W, Cin, Cout))


def direct_wgrad_ok(B, H, W, Cin, Cout, dtype):
    """ssl4gie_conv3x3_direct_wgrad_ok (stride 1, bf16, Cin % 64 == 0, Cout % 32 == 0, both <= 512)"""
    return dtype == torch.bfloat16 and bool(_lib.load().ssl4gie_conv3x3_direct_wgrad_ok(B, H, W, Cin, Cout))


def _gather_geom_ok(B, H, W, C, stride, dtype):
    """ssl4gie_internal_conv_geom_ok (not exported: restated): signed 32-bit byte offsets into the map"""
    return dtype == torch.bfloat16 and stride in (1, 2) and conv_out_hw(H, W, stride)[1] >= 2 and \
        (B * H + 1) * W * C * 2 < 2 ** 31


def gather_fwd_ok(B, H, W, Cin, Cout, stride, dtype):
    """ssl4gie_internal_nt256_ok with a conv geometry: whole 64-channel K-tiles per tap (so no row padding either)"""
    return _gather_geom_ok(B, H, W, Cin, stride, dtype) and Cin % 64 == 0 and Cout % 8 == 0


def gather_wgrad_ok(B, H, W, Cin, Cout, stride, dtype):
    """ssl4gie_internal_tn256_ok with a conv geometry: pixels contracted in whole K-tiles, 32-bit offsets into dy"""
    pixels = B * conv_out_hw(H, W, stride)[0] * conv_out_hw(H, W, stride)[1]
    return _gather_geom_ok(B, H, W, Cin, stride, dtype) and Cin % 8 == 0 and pixels % 64 == 0 and Cout % 8 == 0 and \
        pixels * Cout * 2 < 2 ** 32


def colstats_ok(T, n_out, k_in, dtype):
    """whether the producing GEMM can emit BatchNorm partial statistics (256x256 NT kernel rules)"""
    return dtype == torch.bfloat16 and k_in % 64 == 0 and n_out % 8 == 0 and T > 0


# -------------------------------------------------------------------------------------------------------- preferences
# measured (tools/conv_bench.py): the direct kernel is ahead of the gathered GEMM wherever its 256-wide tiles are
# mostly padding — narrow layers — and on small maps (<= 16 wide: 256 -> 256 @14, 512 -> 512 @7), where the GEMM has
# too few tiles to fill the chip
DIRECT_MAX_COUT, DIRECT_CIN, DIRECT_MAX_W = 128, 32, 16
# direct weight gradient, narrow layers only: from 256 couts on the gathered TN GEMM has full tiles
DIRECT_WGRAD_MAX_COUT = 128
# the gathered NT kernel only exists with 256x256 tiles: below ~100 tiles (ResNet layer4's 7x7 maps) the 128x128
# kernel over a (small) materialised patch matrix keeps more CUs busy
GATHER_MIN_TILES = 96


def _direct_ahead(W, Cin, Cout):
    return Cout <= DIRECT_MAX_COUT or Cin == DIRECT_CIN or W <= DIRECT_MAX_W


def _fills_chip(pixels, n_out):
    return ((pixels + 255) // 256) * ((n_out + 255) // 256) >= GATHER_MIN_TILES


# --------------------------------------------------------------------------------------------------------------- plan
# fwd, wgrad: "direct" | "gather" | "im2col"; dgrad: those or "col2im"; fwd_stats: the BatchNorm partial statistics come
# out of the forward kernel; ld, ld2: row strides of the [Cout, 9 Cin] and (stride-1 data gradient) [Cin, 9 Cout] images
Conv3x3Plan = collections.namedtuple("Conv3x3Plan", "fwd fwd_stats wgrad dgrad ld ld2")


@functools.lru_cache(maxsize=None)
def conv3x3_plan(B, H, W, Cin, Cout, stride, dtype, has_bias, want_stats) -> Conv3x3Plan:
    ld, ld2 = k_pad(9 * Cin, dtype), k_pad(9 * Cout, dtype)
    pixels = B * conv_out_hw(H, W, stride)[0] * conv_out_hw(H, W, stride)[1]
    gather = gather_fwd_ok(B, H, W, Cin, Cout, stride, dtype)
    stats = want_stats and not has_bias
    # direct: where it is ahead of the gathered GEMM (64 -> 64 @56, 128 -> 128 @28, output_conv.2: 128 -> 32), and
    # instead of a materialised patch matrix where that GEMM does not apply (layer1_rn: Cin = 96)
    if stride == 1 and direct_fwd_ok(B, H, W, Cin, Cout, dtype) and (_direct_ahead(W, Cin, Cout) or not gather):
        fwd, fwd_stats = "direct", stats
    elif stats and colstats_ok(pixels, Cout, ld, dtype):
        fwd, fwd_stats = ("gather" if gather else "im2col"), True   # only the 256x256 kernel has them: any tile count
    else:
        fwd, fwd_stats = ("gather" if gather and _fills_chip(pixels, Cout) else "im2col"), False
    if stride == 1 and Cout <= DIRECT_WGRAD_MAX_COUT and direct_wgrad_ok(B, H, W, Cin, Cout, dtype):
        wgrad = "direct"
    else:
        wgrad = "gather" if gather_wgrad_ok(B, H, W, Cin, Cout, stride, dtype) else "im2col"
    if stride != 1:
        dgrad = "col2im"   # the product against the weight, scattered back through the patch-matrix transpose
    elif _direct_ahead(W, Cout, Cin) and direct_fwd_ok(B, H, W, Cout, Cin, dtype):
        dgrad = "direct"   # stride 1: the same convolution on dy [B, H, W, Cout] with the flipped weight
    else:
        dgrad = "gather" if _fills_chip(B * H * W, Cin) and gather_fwd_ok(B, H, W, Cout, Cin, 1, dtype) else "im2col"
    return Conv3x3Plan(fwd, fwd_stats, wgrad, dgrad, ld, ld2)
