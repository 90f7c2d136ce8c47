"""Host-side wrappers of the single-op C-ABI entry points (raw device pointers + current stream).

Every wrapper validates shapes / dtypes / contiguity on the host before the launch — a kernel is
never started on operands whose layout it does not assume.  Tensors are only containers for
device memory here; no torch arithmetic happens in this module.
"""
from __future__ import annotations

import ctypes as C

import os

import torch

from . import _lib
from ._lib import BF16, F32, GemmDesc
from .conv_plan import colstats_ok, conv_out_hw, gather_fwd_ok, gather_wgrad_ok, k_pad  # noqa: F401 (ops.k_pad, ...)

_TORCH2CODE = {torch.float32: F32, torch.bfloat16: BF16}
_CODE2TORCH = {F32: torch.float32, BF16: torch.bfloat16}


def code(dtype) -> int:
    try:
        return _TORCH2CODE[dtype]
    except KeyError:
        raise TypeError(f"unsupported dtype {dtype}; the HIP path computes in fp32 or bf16")


def torch_dtype(c: int):
    return _CODE2TORCH[c]


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def ptr(t) -> int:
    return 0 if t is None else t.data_ptr()


def _dev(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("ssl4gie_amd ops need tensors on the HIP device (no CPU fallback)")
        if not t.is_contiguous():
            raise RuntimeError("ssl4gie_amd ops need contiguous tensors")


def _f32(*ts):
    for t in ts:
        if t is not None and t.dtype != torch.float32:
            raise TypeError(f"expected float32, got {t.dtype}")


# ------------------------------------------------------------------ LayerNorm
def layernorm_fwd(x, gamma, beta, eps, out_dtype, save_stats=True):
    _dev(x, gamma, beta)
    _f32(x, gamma, beta)
    cols = x.shape[-1]
    rows = x.numel() // cols
    assert gamma.numel() == cols and beta.numel() == cols and cols % 4 == 0
    y = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device) if save_stats else None
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device) if save_stats else None
    L = _lib.load()
    _lib.check(L.ssl4gie_layernorm_fwd(ptr(x), ptr(gamma), ptr(beta), ptr(y), code(out_dtype),
                                       ptr(mean), ptr(rstd), rows, cols, float(eps), stream()),
               "layernorm_fwd")
    return y, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, dres=None, want_lp=False, dgamma=None, dbeta=None,
                  accumulate=False):
    _dev(dy, x, gamma, mean, rstd, dres, dgamma, dbeta)
    _f32(x, gamma, mean, rstd, dres, dgamma, dbeta)
    cols = x.shape[-1]
    rows = x.numel() // cols
    assert dy.shape == x.shape and mean.numel() == rows and rstd.numel() == rows
    assert dres is None or dres.shape == x.shape
    L = _lib.load()
    dx = torch.empty_like(x)
    dx_lp = torch.empty(x.shape, dtype=dy.dtype, device=x.device) if want_lp else None
    if dgamma is None:
        dgamma = torch.empty(cols, dtype=torch.float32, device=x.device)
        dbeta = torch.empty(cols, dtype=torch.float32, device=x.device)
    ws = torch.empty(L.ssl4gie_layernorm_bwd_workspace_bytes(rows, cols), dtype=torch.uint8,
                     device=x.device)
    _lib.check(L.ssl4gie_layernorm_bwd(ptr(dy), code(dy.dtype), ptr(x), ptr(gamma), ptr(mean),
                                       ptr(rstd), ptr(dres), ptr(dx), ptr(dx_lp), code(dy.dtype),
                                       ptr(dgamma), ptr(dbeta), int(accumulate), ptr(ws), rows,
                                       cols, stream()), "layernorm_bwd")
    return dx, dx_lp, dgamma, dbeta


def colsum(x2d, out=None, accumulate=False):
    _dev(x2d, out)
    rows, cols = x2d.shape
    L = _lib.load()
    if out is None:
        out = torch.empty(cols, dtype=torch.float32, device=x2d.device)
    assert out.numel() == cols and out.dtype == torch.float32
    ws = torch.empty(max(1, L.ssl4gie_colsum_workspace_bytes(rows, cols)), dtype=torch.uint8,
                     device=x2d.device)
    _lib.check(L.ssl4gie_colsum(ptr(x2d), code(x2d.dtype), ptr(out), int(accumulate), ptr(ws),
                                rows, cols, cols, stream()), "colsum")
    return out


# ------------------------------------------------------------------ GEMM
def gemm_raw(desc: GemmDesc, device):
    L = _lib.load()
    nbytes = L.ssl4gie_gemm_workspace_bytes(C.byref(desc))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes else None
    _lib.check(L.ssl4gie_gemm(C.byref(desc), ptr(ws), nbytes, stream()), "gemm")


def _desc(M, N, K, dt_ab, dt_c):
    d = GemmDesc()
    d.M, d.N, d.K, d.batch1, d.batch2 = M, N, K, 1, 1
    d.dtype_ab, d.dtype_c, d.alpha, d.epilogue = dt_ab, dt_c, 1.0, _lib.EPI_NONE
    return d


def linear_fwd(x2d, w, bias=None, out_dtype=None, epilogue=None, residual=None, colstats=False):
    """y[T, n_out] = x2d[T, k_in] @ w[n_out, k_in]^T (+bias | +bias+residual | gelu pair).
    colstats=True (bf16, no bias): also returns the per-128-row column sums / sums of squares of y
    ([ceil(T/128), 2, n_out] fp32) for the BatchNorm that follows."""
    _dev(x2d, w, bias, residual)
    T, k_in = x2d.shape
    n_out, k2 = w.shape
    assert k2 == k_in and x2d.dtype == w.dtype, (x2d.shape, w.shape, x2d.dtype, w.dtype)
    out_dtype = out_dtype or x2d.dtype
    d = _desc(T, n_out, k_in, code(x2d.dtype), code(out_dtype))
    d.A, d.sAm, d.sAk = ptr(x2d), k_in, 1
    d.B, d.sBk, d.sBn = ptr(w), 1, k_in
    y = torch.empty(T, n_out, dtype=out_dtype, device=x2d.device)
    d.C, d.ldc = ptr(y), n_out
    out2 = None
    if epilogue is None:
        epilogue = _lib.EPI_BIAS if bias is not None else _lib.EPI_NONE
    d.epilogue = epilogue
    if bias is not None:
        _f32(bias)
        assert bias.numel() == n_out
        d.bias = ptr(bias)
    if epilogue == _lib.EPI_BIAS_RESIDUAL:
        _f32(residual)
        assert residual.shape == (T, n_out)
        d.residual, d.ldr = ptr(residual), n_out
    if epilogue in (_lib.EPI_BIAS_GELU, _lib.EPI_BIAS_GELU_GRAD):
        out2 = torch.empty_like(y)  # (u, gelu(u)) resp. (gelu'(u), gelu(u))
        d.out2 = ptr(out2)
    if colstats:
        assert bias is None and epilogue == _lib.EPI_NONE and colstats_ok(T, n_out, k_in, x2d.dtype)
        stats = torch.empty((T + 127) // 128, 2, n_out, dtype=torch.float32, device=x2d.device)
        d.colstats = ptr(stats)
        gemm_raw(d, x2d.device)
        return y, stats
    gemm_raw(d, x2d.device)
    return (y, out2) if out2 is not None else y


def linear_fwd_kblocks(x2d, w, block):
    """y = x2d @ w^T in fp32, the contraction taken `block` columns at a time and the partial products added in
    fp32 (accumulate): a rounding chain of k_in / block + block / 4 steps instead of k_in / 4 — the parity mode's
    product over a 3x3 patch matrix, one tap per block"""
    _dev(x2d, w)
    _f32(x2d, w)
    T, k_in = x2d.shape
    n_out = w.shape[0]
    assert w.shape[1] == k_in and block >= 1 and k_in % block == 0, (x2d.shape, w.shape, block)
    y = torch.empty(T, n_out, dtype=torch.float32, device=x2d.device)
    for k0 in range(0, k_in, block):
        d = _desc(T, n_out, block, F32, F32)
        d.A, d.sAm, d.sAk = ptr(x2d) + 4 * k0, k_in, 1
        d.B, d.sBk, d.sBn = ptr(w) + 4 * k0, 1, k_in
        d.C, d.ldc = ptr(y), n_out
        d.accumulate = int(k0 > 0)
        gemm_raw(d, x2d.device)
    return y


def linear_colstats_only(x2d, w):
    """the BatchNorm partial statistics [ceil(T/128), 2, n_out] of y = x2d @ w^T (of its bf16-rounded values, as
    linear_fwd(colstats=True) returns them) WITHOUT writing y: the first half of the BatchNorm-fused 1x1
    convolution (linear_affine_fwd is the second)"""
    _dev(x2d, w)
    T, k_in = x2d.shape
    n_out = w.shape[0]
    assert w.shape[1] == k_in and x2d.dtype == w.dtype and colstats_ok(T, n_out, k_in, x2d.dtype)
    d = _desc(T, n_out, k_in, code(x2d.dtype), code(x2d.dtype))
    d.A, d.sAm, d.sAk = ptr(x2d), k_in, 1
    d.B, d.sBk, d.sBn = ptr(w), 1, k_in
    d.C, d.ldc = None, n_out
    d.epilogue = _lib.EPI_NONE
    stats = torch.empty((T + 127) // 128, 2, n_out, dtype=torch.float32, device=x2d.device)
    d.colstats = ptr(stats)
    gemm_raw(d, x2d.device)
    return stats


def linear_affine_fwd(x2d, w, scale, shift, aux=None, relu=False):
    """act((x2d @ w^T) * scale[n] + shift[n] (+ aux)), act = ReLU if `relu` (EPI_AFFINE_AUX_RELU): bf16 operands
    and output, the affine map applied to the fp32 accumulators"""
    _dev(x2d, w, scale, shift, aux)
    _f32(scale); _f32(shift)
    T, k_in = x2d.shape
    n_out = w.shape[0]
    assert w.shape[1] == k_in and x2d.dtype == w.dtype == torch.bfloat16
    assert scale.numel() == n_out and shift.numel() == n_out and scale.is_contiguous() and shift.is_contiguous()
    d = _desc(T, n_out, k_in, code(x2d.dtype), code(x2d.dtype))
    d.A, d.sAm, d.sAk = ptr(x2d), k_in, 1
    d.B, d.sBk, d.sBn = ptr(w), 1, k_in
    y = torch.empty(T, n_out, dtype=x2d.dtype, device=x2d.device)
    d.C, d.ldc = ptr(y), n_out
    d.epilogue, d.scale, d.bias, d.relu = _lib.EPI_AFFINE_AUX_RELU, ptr(scale), ptr(shift), int(bool(relu))
    if aux is not None:
        assert aux.shape == (T, n_out) and aux.dtype == x2d.dtype and aux.is_contiguous()
        d.aux = ptr(aux)
    gemm_raw(d, x2d.device)
    return y


def bn_coef_partials(partials, rows, gamma, beta, running_mean, running_var, momentum, eps):
    """training-mode BatchNorm statistics from GEMM-epilogue partials -> (coef [2, C]: y = x coef[0] + coef[1],
    mean, rstd); running statistics updated"""
    _, _, coef, mean, rstd = _bn_fwd(_lib.BN_FROM_PARTIALS, None, rows, partials.shape[2], partials, gamma, beta,
                                     running=(running_mean, running_var), momentum=momentum, eps=eps)
    return coef, mean, rstd


def add_aux_ok(T, k_in, n_out, dtype, has_wt):
    """whether linear_bwd_data can join a second gradient contribution in its epilogue"""
    return dtype == torch.bfloat16 and has_wt and n_out % 64 == 0 and k_in % 8 == 0 and T > 0


def linear_bwd_data(dy2d, w, w_t=None, out_dtype=None, dgelu_aux=None, mul_aux=None, add_aux=None):
    """dx[T, k_in] = dy[T, n_out] @ w[n_out, k_in]; uses w_t[k_in, n_out] (NT fast path) if given.
    `dgelu_aux` = u: dx *= gelu'(u);  `mul_aux` = m: dx *= m (m = gelu'(u) saved by the forward);
    `add_aux` = g: dx += g (another gradient contribution of the same tensor; see add_aux_ok)."""
    _dev(dy2d, w, w_t, dgelu_aux, mul_aux, add_aux)
    T, n_out = dy2d.shape
    k_in = w.shape[1]
    assert w.shape[0] == n_out
    out_dtype = out_dtype or dy2d.dtype
    d = _desc(T, k_in, n_out, code(dy2d.dtype), code(out_dtype))
    d.A, d.sAm, d.sAk = ptr(dy2d), n_out, 1
    if w_t is not None:
        assert w_t.shape == (k_in, n_out) and w_t.dtype == dy2d.dtype
        d.B, d.sBk, d.sBn = ptr(w_t), 1, n_out
    else:
        assert w.dtype == dy2d.dtype
        d.B, d.sBk, d.sBn = ptr(w), k_in, 1
    dx = torch.empty(T, k_in, dtype=out_dtype, device=dy2d.device)
    d.C, d.ldc = ptr(dx), k_in
    if dgelu_aux is not None:
        assert dgelu_aux.shape == dx.shape and dgelu_aux.dtype == out_dtype
        d.epilogue, d.aux = _lib.EPI_DGELU, ptr(dgelu_aux)
    if mul_aux is not None:
        assert dgelu_aux is None and mul_aux.shape == dx.shape and mul_aux.dtype == out_dtype
        d.epilogue, d.aux = _lib.EPI_MUL_AUX, ptr(mul_aux)
    if add_aux is not None:
        assert dgelu_aux is None and mul_aux is None and add_aux.dtype == out_dtype and \
            add_aux.numel() == dx.numel() and add_aux.is_contiguous() and \
            add_aux_ok(T, k_in, n_out, dy2d.dtype, w_t is not None)
        d.epilogue, d.aux = _lib.EPI_ADD_AUX, ptr(add_aux)
    gemm_raw(d, dy2d.device)
    return dx


def _wgrad_desc(dy, x, out, bias_out, accumulate):
    """descriptor of out[n_out, k_in] (+)= dy[T, n_out]^T @ x[T, k_in] (fp32), bias_out[n_out] = column sums of dy"""
    (T, n_out), k_in = dy.shape, x.shape[1]
    d = _desc(n_out, k_in, T, code(dy.dtype), F32)
    d.A, d.sAm, d.sAk = ptr(dy), 1, n_out
    d.B, d.sBk, d.sBn = ptr(x), k_in, 1
    d.C, d.ldc = ptr(out), k_in
    d.accumulate = int(accumulate)
    if bias_out is not None:
        assert bias_out.dtype == torch.float32 and bias_out.numel() == n_out
        d.colsum_a = ptr(bias_out)
    return d


def linear_bwd_weight(dy2d, x2d, out=None, accumulate=False, bias_out=None):
    """dW[n_out, k_in] = dy[T, n_out]^T @ x[T, k_in]  (fp32 output); with `bias_out` [n_out] the
    bias gradient (column sums of dy) is produced by the same call."""
    _dev(dy2d, x2d, out, bias_out)
    T, n_out = dy2d.shape
    T2, k_in = x2d.shape
    assert T == T2 and dy2d.dtype == x2d.dtype
    if out is None:
        out = torch.empty(n_out, k_in, dtype=torch.float32, device=x2d.device)
    assert out.dtype == torch.float32 and out.numel() == n_out * k_in
    gemm_raw(_wgrad_desc(dy2d, x2d, out, bias_out, accumulate), x2d.device)
    return out


def linear_bwd_weight_pair(dy_a, x_a, dy_b, x_b, bias_a=None, bias_b=None):
    """two weight-gradient products with the same token count in ONE launch (ssl4gie_gemm_tn_pair):
    (dW_a [n_a, k_a], dW_b [n_b, k_b]) = (dy_a^T x_a, dy_b^T x_b); optional fused bias gradients"""
    _dev(dy_a, x_a, dy_b, x_b, bias_a, bias_b)
    T = dy_a.shape[0]
    assert dy_b.shape[0] == T and x_a.shape[0] == T and x_b.shape[0] == T
    outs, descs = [], []
    for dy, x, b in ((dy_a, x_a, bias_a), (dy_b, x_b, bias_b)):
        outs.append(torch.empty(dy.shape[1], x.shape[1], dtype=torch.float32, device=x.device))
        descs.append(_wgrad_desc(dy, x, outs[-1], b, False))
    L = _lib.load()
    nbytes = L.ssl4gie_gemm_tn_pair_workspace_bytes(C.byref(descs[0]), C.byref(descs[1]))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dy_a.device) if nbytes else None
    _lib.check(L.ssl4gie_gemm_tn_pair(C.byref(descs[0]), C.byref(descs[1]), ptr(ws), nbytes, stream()),
               "gemm_tn_pair")
    return outs[0], outs[1]


def linear_bwd_weight_group(pairs, accumulate_into=None):
    """n weight-gradient products with the same token count in ONE launch (ssl4gie_gemm_tn_group).
    pairs: [(dy [T, n_i], x [T, k_i], bias_out or None), ...] -> [dW_i [n_i, k_i]].
    accumulate_into: optional list of existing fp32 dW tensors to accumulate into (C += dY^T X)."""
    T = pairs[0][0].shape[0]
    n = len(pairs)
    descs = (GemmDesc * n)()
    outs = []
    for i, (dy, x, b) in enumerate(pairs):
        _dev(dy, x, b)
        assert dy.shape[0] == T and x.shape[0] == T
        n_out, k_in = dy.shape[1], x.shape[1]
        if accumulate_into is not None:
            out = accumulate_into[i]
            assert out.shape == (n_out, k_in) and out.dtype == torch.float32
        else:
            out = torch.empty(n_out, k_in, dtype=torch.float32, device=x.device)
        descs[i] = _wgrad_desc(dy, x, out, b, accumulate_into is not None)
        outs.append(out)
    L = _lib.load()
    nbytes = L.ssl4gie_gemm_tn_group_workspace_bytes(descs, n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=pairs[0][0].device) if nbytes else None
    _lib.check(L.ssl4gie_gemm_tn_group(descs, n, ptr(ws), nbytes, stream()), "gemm_tn_group")
    return outs


# ------------------------------------------------------------------ attention
def attn_fwd(qkv, B, N, H, hd):
    _dev(qkv)
    D = H * hd
    assert qkv.numel() == B * N * 3 * D
    L = _lib.load()
    out = torch.empty(B, N, D, dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty(B, H, N, dtype=torch.float32, device=qkv.device)
    nb = L.ssl4gie_attn_workspace_bytes(code(qkv.dtype), B, N, H, hd)
    ws = torch.empty(nb, dtype=torch.uint8, device=qkv.device) if nb else None
    _lib.check(L.ssl4gie_attn_fwd(ptr(qkv), ptr(out), ptr(lse), code(qkv.dtype), B, N, H, hd,
                                  ptr(ws), stream()), "attn_fwd")
    return out, lse


def attn_bwd(qkv, out, dout, lse, B, N, H, hd):
    _dev(qkv, out, dout, lse)
    assert out.dtype == qkv.dtype and dout.dtype == qkv.dtype and lse.dtype == torch.float32
    assert out.numel() == B * N * H * hd and dout.numel() == out.numel()
    L = _lib.load()
    dqkv = torch.empty_like(qkv)
    nb = L.ssl4gie_attn_workspace_bytes(code(qkv.dtype), B, N, H, hd)
    ws = torch.empty(nb, dtype=torch.uint8, device=qkv.device) if nb else None
    _lib.check(L.ssl4gie_attn_bwd(ptr(qkv), ptr(out), ptr(dout), ptr(lse), ptr(dqkv),
                                  code(qkv.dtype), B, N, H, hd, ptr(ws), stream()), "attn_bwd")
    return dqkv


# ------------------------------------------------------------------ casts
def cast(src, dtype, out=None):
    _dev(src, out)
    _f32(src)
    if out is None:
        out = torch.empty(src.shape, dtype=dtype, device=src.device)
    assert out.numel() == src.numel() and out.dtype == dtype
    _lib.check(_lib.load().ssl4gie_cast(ptr(src), ptr(out), code(dtype), src.numel(), stream()),
               "cast")
    return out


def cast_transpose(src2d, dtype, out=None):
    _dev(src2d, out)
    _f32(src2d)
    r, c = src2d.shape
    if out is None:
        out = torch.empty(c, r, dtype=dtype, device=src2d.device)
    assert out.numel() == r * c and out.dtype == dtype
    _lib.check(_lib.load().ssl4gie_cast_transpose(ptr(src2d), ptr(out), code(dtype), r, c,
                                                  stream()), "cast_transpose")
    return out


def bt_loss(c, lambd):
    """Barlow Twins loss of the fp32 [D, D] correlation matrix: sum_i (c_ii - 1)^2 + lambd sum_{i != j} c_ij^2"""
    _dev(c)
    _f32(c)
    D = c.shape[0]
    assert c.shape == (D, D)
    L = _lib.load()
    ws = torch.empty(L.ssl4gie_bt_loss_workspace_bytes(D), dtype=torch.uint8, device=c.device)
    loss = torch.empty((), dtype=torch.float32, device=c.device)
    _lib.check(L.ssl4gie_bt_loss(ptr(c), ptr(loss), D, float(lambd), ptr(ws), stream()), "bt_loss")
    return loss


def bt_loss_grad(c, scale, dtype, lambd):
    """(w, wt): dL/dc of the Barlow Twins loss times the device scalar `scale`, rounded to `dtype`, and its
    transpose — the two operands of the backward GEMMs from one read of c"""
    _dev(c)
    _f32(c)
    D = c.shape[0]
    assert c.shape == (D, D)
    scale = scale.to(device=c.device, dtype=torch.float32).reshape(()).contiguous()
    w = torch.empty(D, D, dtype=dtype, device=c.device)
    wt = torch.empty(D, D, dtype=dtype, device=c.device)
    _lib.check(_lib.load().ssl4gie_bt_loss_grad(ptr(c), ptr(scale), ptr(w), ptr(wt), code(dtype), D, float(lambd),
                                                stream()), "bt_loss_grad")
    return w, wt


def add_cast(a, b=None, want_f32=True, lp_dtype=None):
    """out = a + b on the fp32 gradient stream; optionally also its operand-type copy."""
    _dev(a, b)
    _f32(a, b)
    assert b is None or b.shape == a.shape
    out = torch.empty_like(a) if want_f32 else None
    out_lp = torch.empty(a.shape, dtype=lp_dtype, device=a.device) if lp_dtype is not None else None
    _lib.check(_lib.load().ssl4gie_add_cast(ptr(a), ptr(b), ptr(out), ptr(out_lp),
                                            code(lp_dtype) if lp_dtype is not None else 0,
                                            a.numel(), stream()), "add_cast")
    return out, out_lp


# ------------------------------------------------------------------ MAE glue
def mask_argsort(noise, len_keep):
    _dev(noise)
    _f32(noise)
    B, Lp = noise.shape
    ids_shuffle = torch.empty(B, Lp, dtype=torch.int64, device=noise.device)
    ids_restore = torch.empty_like(ids_shuffle)
    mask = torch.empty(B, Lp, dtype=torch.float32, device=noise.device)
    _lib.check(_lib.load().ssl4gie_mask_argsort(ptr(noise), ptr(ids_shuffle), ptr(ids_restore),
                                                ptr(mask), B, Lp, int(len_keep), stream()),
               "mask_argsort")
    return ids_shuffle, ids_restore, mask


def patch_gather(img, p, ids=None, nsel=None, out_dtype=torch.float32, order=0):
    _dev(img, ids)
    _f32(img)
    B, Cc, H, W = img.shape
    npatch = (H // p) * (W // p)
    if ids is not None:
        assert ids.dtype == torch.int64 and ids.shape[0] == B and ids.dim() == 2
        ids_stride = ids.shape[1]
        nsel = nsel if nsel is not None else ids.shape[1]
        assert nsel <= ids.shape[1]
    else:
        ids_stride, nsel = 0, npatch
    out = torch.empty(B * nsel, Cc * p * p, dtype=out_dtype, device=img.device)
    _lib.check(_lib.load().ssl4gie_patch_gather(ptr(img), ptr(ids), ptr(out), code(out_dtype), B,
                                                Cc, H, W, p, nsel, ids_stride, order, stream()),
               "patch_gather")
    return out


def tokens_assemble(y2d, cls, pos, B, nsel, ids=None):
    _dev(y2d, cls, pos, ids)
    _f32(cls, pos)
    D = y2d.shape[1]
    assert y2d.shape[0] == B * nsel and cls.numel() == D and pos.shape[-1] == D
    ids_stride = 0
    if ids is not None:
        assert ids.dtype == torch.int64 and ids.shape[0] == B and ids.shape[1] >= nsel
        ids_stride = ids.shape[1]
        assert pos.numel() // D >= 1 + ids.shape[1]
    else:
        assert pos.numel() // D >= 1 + nsel
    x = torch.empty(B, nsel + 1, D, dtype=torch.float32, device=y2d.device)
    _lib.check(_lib.load().ssl4gie_tokens_assemble(ptr(y2d), code(y2d.dtype), ptr(cls), ptr(pos),
                                                   ptr(ids), ids_stride, ptr(x), B, nsel, D,
                                                   stream()), "tokens_assemble")
    return x


def tokens_assemble_bwd(dx, lp_dtype, dcls_out=None, accumulate=False):
    """dy[b*nsel+j] = dx[b,1+j] (operand type); dcls_out (+)= sum_b dx[b,0] if given."""
    _dev(dx, dcls_out)
    _f32(dx, dcls_out)
    B, n1, D = dx.shape
    assert dcls_out is None or dcls_out.numel() == D
    dy = torch.empty(B * (n1 - 1), D, dtype=lp_dtype, device=dx.device)
    _lib.check(_lib.load().ssl4gie_tokens_assemble_bwd(ptr(dx), ptr(dy), code(lp_dtype),
                                                       ptr(dcls_out), int(accumulate), B, n1 - 1,
                                                       D, stream()), "tokens_assemble_bwd")
    return dy


def decoder_assemble(y, mask_token, dpos, ids_restore, nkeep):
    _dev(y, mask_token, dpos, ids_restore)
    _f32(mask_token, dpos)
    B, Lp = ids_restore.shape
    D = y.shape[-1]
    assert y.numel() == B * (nkeep + 1) * D and mask_token.numel() == D
    assert dpos.numel() == (Lp + 1) * D and ids_restore.dtype == torch.int64
    xd = torch.empty(B, Lp + 1, D, dtype=torch.float32, device=y.device)
    _lib.check(_lib.load().ssl4gie_decoder_assemble(ptr(y), code(y.dtype), ptr(mask_token),
                                                    ptr(dpos), ptr(ids_restore), ptr(xd), B, Lp,
                                                    nkeep, D, stream()), "decoder_assemble")
    return xd


def decoder_assemble_bwd(dxd, ids_shuffle, nkeep, lp_dtype, dmask_out, accumulate=False):
    _dev(dxd, ids_shuffle, dmask_out)
    _f32(dxd, dmask_out)
    B, L1, D = dxd.shape
    Lp = L1 - 1
    assert ids_shuffle.shape == (B, Lp) and ids_shuffle.dtype == torch.int64
    assert dmask_out.numel() == D
    L = _lib.load()
    dy = torch.empty(B, nkeep + 1, D, dtype=lp_dtype, device=dxd.device)
    ws = torch.empty(L.ssl4gie_decoder_assemble_bwd_workspace_bytes(B, Lp, D), dtype=torch.uint8,
                     device=dxd.device)
    _lib.check(L.ssl4gie_decoder_assemble_bwd(ptr(dxd), ptr(ids_shuffle), ptr(dy), code(lp_dtype),
                                              ptr(dmask_out), int(accumulate), ptr(ws), B, Lp,
                                              nkeep, D, stream()), "decoder_assemble_bwd")
    return dy


def _loss_geom(pred, img, mask, p):
    B, Cc, H, W = img.shape
    Lp = (H // p) * (W // p)
    assert mask.shape == (B, Lp) and pred.dim() == 3 and pred.shape[0] == B
    assert pred.shape[2] == Cc * p * p and pred.shape[1] in (Lp, Lp + 1)
    return B, Cc, H, W, int(pred.shape[1] == Lp + 1)


def mae_loss_fwd(pred, img, mask, p, norm_pix):
    """per_patch[B, L] = mask * mean((pred - target)^2); pred is [B, L, P] or [B, 1+L, P]."""
    _dev(pred, img, mask)
    _f32(pred, img, mask)
    B, Cc, H, W, has_cls = _loss_geom(pred, img, mask, p)
    per_patch = torch.empty_like(mask)
    _lib.check(_lib.load().ssl4gie_mae_loss(ptr(pred), ptr(img), ptr(mask), ptr(per_patch), 0, 0,
                                            1.0, int(norm_pix), has_cls, B, Cc, H, W, p, stream()),
               "mae_loss")
    return per_patch


def mae_loss_bwd(pred, img, mask, p, norm_pix, gpp, gscale_host=1.0):
    _dev(pred, img, mask, gpp)
    _f32(pred, img, mask, gpp)
    assert gpp is None or gpp.shape == mask.shape
    B, Cc, H, W, has_cls = _loss_geom(pred, img, mask, p)
    dpred = torch.empty_like(pred)
    _lib.check(_lib.load().ssl4gie_mae_loss(ptr(pred), ptr(img), ptr(mask), 0, ptr(dpred),
                                            ptr(gpp), float(gscale_host), int(norm_pix), has_cls,
                                            B, Cc, H, W, p, stream()), "mae_loss(bwd)")
    return dpred


# ------------------------------------------------------------------ DPT decoder glue (channels-last)
def _nhwc(x):
    _dev(x)
    assert x.dim() == 4, "expected [B, H, W, C]"
    return x.shape


def im2col3x3(x, stride=1, relu=False, ld=None):
    B, H, W, C = _nhwc(x)
    Ho, Wo = conv_out_hw(H, W, stride)
    ld = ld or k_pad(9 * C, x.dtype)
    cols = torch.empty(B * Ho * Wo, ld, dtype=x.dtype, device=x.device)
    _lib.check(_lib.load().ssl4gie_im2col3x3(ptr(x), ptr(cols), code(x.dtype), B, H, W, C, stride,
                                             int(relu), ld, stream()), "im2col3x3")
    return cols


def conv3x3_implicit_ok(x, stride, n_out=None, wgrad=False):
    """whether the gathered 256x256 GEMM kernels take this map: conv_plan's limits for a tensor"""
    return x.is_contiguous() and (gather_wgrad_ok if wgrad else gather_fwd_ok)(*x.shape, n_out, stride, x.dtype)


def _geom(x, stride, relu):
    B, H, W, C_ = x.shape
    g = _lib.Conv3x3Geom()
    g.B, g.H, g.W, g.C, g.stride, g.relu = B, H, W, C_, stride, int(relu)
    return g


def conv3x3_fwd(x, w2, bias=None, stride=1, relu=False, relu_mask=None, colstats=False):
    """y[(b,oy,ox), co] = sum_k P[(b,oy,ox), k] w2[co, k] (+ bias), P = implicit patch matrix of the
    bf16 map x [B,H,W,C] (never materialised; ssl4gie_gemm_desc.conv), w2 [Cout, 9C].
    `relu_mask` [B,Ho,Wo,Cout]: y = relu_mask > 0 ? y : 0 in the epilogue (the data gradient of a
    convolution whose input went through a ReLU; no bias, no relu)."""
    _dev(x, w2, bias, relu_mask)
    B, H, W, Cin = _nhwc(x)
    Cout, K = w2.shape
    assert K == 9 * Cin and w2.dtype == x.dtype and w2.is_contiguous()
    assert conv3x3_implicit_ok(x, stride, Cout)
    Ho, Wo = conv_out_hw(H, W, stride)
    M = B * Ho * Wo
    d = _desc(M, Cout, K, code(x.dtype), code(x.dtype))
    g = _geom(x, stride, relu)
    d.conv = C.pointer(g)
    d.A, d.sAm, d.sAk = ptr(x), K, 1
    d.B, d.sBk, d.sBn = ptr(w2), 1, K
    y = torch.empty(M, Cout, dtype=x.dtype, device=x.device)
    d.C, d.ldc = ptr(y), Cout
    if bias is not None:
        _f32(bias)
        assert bias.numel() == Cout
        d.epilogue, d.bias = _lib.EPI_BIAS, ptr(bias)
    if relu_mask is not None:
        assert bias is None and not relu and relu_mask.dtype == x.dtype and relu_mask.is_contiguous() \
            and relu_mask.numel() == M * Cout
        d.epilogue, d.aux = _lib.EPI_RELU_MASK_AUX, ptr(relu_mask)
    if colstats:  # BatchNorm partial statistics of y (see linear_fwd)
        assert bias is None and relu_mask is None
        stats = torch.empty((M + 127) // 128, 2, Cout, dtype=torch.float32, device=x.device)
        d.colstats = ptr(stats)
        gemm_raw(d, x.device)
        return y.view(B, Ho, Wo, Cout), stats
    gemm_raw(d, x.device)
    return y.view(B, Ho, Wo, Cout)


def conv3x3_bwd_weight(dy2d, x, stride=1, relu=False, bias_out=None):
    """dW2[co, k] = sum_pixels dy[(b,oy,ox), co] P[(b,oy,ox), k] (fp32 [Cout, 9C]); with `bias_out`
    the bias gradient rides on the same product."""
    _dev(dy2d, x, bias_out)
    B, H, W, Cin = _nhwc(x)
    T, Cout = dy2d.shape
    Ho, Wo = conv_out_hw(H, W, stride)
    assert T == B * Ho * Wo and dy2d.dtype == x.dtype and dy2d.is_contiguous()
    assert conv3x3_implicit_ok(x, stride, Cout, wgrad=True)
    out = torch.empty(Cout, 9 * Cin, dtype=torch.float32, device=x.device)
    d = _desc(Cout, 9 * Cin, T, code(x.dtype), F32)
    g = _geom(x, stride, relu)
    d.conv = C.pointer(g)
    d.A, d.sAm, d.sAk = ptr(dy2d), 1, Cout
    d.B, d.sBk, d.sBn = ptr(x), 9 * Cin, 1
    d.C, d.ldc = ptr(out), 9 * Cin
    if bias_out is not None:
        assert bias_out.dtype == torch.float32 and bias_out.numel() == Cout
        d.colsum_a = ptr(bias_out)
    gemm_raw(d, x.device)
    return out


def conv3x3_direct_fwd(x, w2, bias=None, relu=False, relu_mask=None, colstats=False):
    """stride-1 3x3 convolution of the bf16 map x [B,H,W,Cin] with w2 [Cout, 9 Cin] on the direct
    kernel; semantics of conv3x3_fwd (bias and relu_mask may be combined with relu here).
    colstats: also return the BatchNorm partial statistics [tiles, 2, Cout] of y."""
    _dev(x, w2, bias, relu_mask)
    B, H, W, Cin = _nhwc(x)
    Cout, K = w2.shape
    assert K == 9 * Cin and w2.dtype == x.dtype == torch.bfloat16 and w2.is_contiguous() and x.is_contiguous()
    if bias is not None:
        _f32(bias)
        assert bias.numel() == Cout
    if relu_mask is not None:
        assert relu_mask.dtype == x.dtype and relu_mask.is_contiguous() and relu_mask.numel() == B * H * W * Cout
    y = torch.empty(B, H, W, Cout, dtype=x.dtype, device=x.device)
    L = _lib.load()
    stats = None
    if colstats:
        assert relu_mask is None
        stats = torch.empty(L.ssl4gie_conv3x3_direct_tiles(B, H, W), 2, Cout, dtype=torch.float32, device=x.device)
    _lib.check(L.ssl4gie_conv3x3_direct_fwd(ptr(x), ptr(w2), ptr(bias), ptr(relu_mask), ptr(y), ptr(stats),
                                            B, H, W, Cin, Cout, int(relu), stream()), "conv3x3_direct_fwd")
    return (y, stats) if colstats else y


def conv3x3_direct_wgrad(dy, x, relu=False, bias_out=None):
    """dW2 [Cout, 9 Cin] fp32 of the direct convolution: dy [B,H,W,Cout] (or [B*H*W, Cout], Cout % 32 == 0),
    x [B,H,W,Cin]; with `bias_out` [Cout] fp32 the bias gradient is produced by the same kernel"""
    _dev(dy, x, bias_out)
    if bias_out is not None:
        assert bias_out.dtype == torch.float32 and bias_out.numel() == dy.shape[-1]
    B, H, W, Cin = _nhwc(x)
    Cout = dy.shape[-1]
    assert dy.numel() == B * H * W * Cout and dy.dtype == x.dtype and dy.is_contiguous()
    lib = _lib.load()
    nbytes = lib.ssl4gie_conv3x3_direct_wgrad_workspace_bytes(B, H, W, Cin, Cout)
    assert nbytes > 0, "conv3x3_direct_wgrad: unsupported geometry"
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    out = torch.empty(Cout, 9 * Cin, dtype=torch.float32, device=x.device)
    _lib.check(lib.ssl4gie_conv3x3_direct_wgrad(ptr(dy), ptr(x), ptr(out), ptr(bias_out), ptr(ws), nbytes, B, H, W, Cin,
                                                Cout, int(relu), 0, stream()), "conv3x3_direct_wgrad")
    return out


def stem7x7_pack(imgs):
    """fp32 NCHW [B,3,H,W] -> the padded 4-channel bf16 image the direct stem kernels read"""
    _dev(imgs)
    _f32(imgs)
    B, Cc, H, W = imgs.shape
    assert Cc == 3 and imgs.is_contiguous()
    L = _lib.load()
    nb = L.ssl4gie_stem7x7_packed_bytes(B, H, W)
    assert nb > 0, "stem7x7: unsupported image size"
    out = torch.empty(nb // 2, dtype=torch.bfloat16, device=imgs.device)
    _lib.check(L.ssl4gie_stem7x7_pack(ptr(imgs), ptr(out), B, H, W, stream()), "stem7x7_pack")
    return out


def _pack_shape(w, mode, ld):
    """(Cout, Cin, row length, shape) of the mode-`mode` operand image of w [Cout, Cin, 3, 3]; ld None = unpadded"""
    Cout, Cin = w.shape[:2]
    ld = 9 * (Cout if mode == 1 else Cin) if ld is None else ld
    return Cout, Cin, ld, ((Cout, ld) if mode == 0 else ((Cin, ld) if mode == 1 else (ld, Cout)))


def conv3x3_weight_pack(weight, dtype, mode, ld=None):
    """operand image of a Conv2d(k=3) weight [Cout, Cin, 3, 3] fp32 in one launch (cast included):
    mode 0 -> [Cout, ld] rows (tap, ci); mode 1 -> [Cin, ld] rows (flipped tap, co); mode 2 -> [ld, Cout]"""
    _dev(weight)
    assert weight.dtype == torch.float32 and weight.dim() == 4 and weight.shape[2:] == (3, 3)
    w = weight.contiguous()
    Cout, Cin, ld, shape = _pack_shape(w, mode, ld)
    out = torch.empty(shape, dtype=dtype, device=w.device)
    _lib.check(_lib.load().ssl4gie_conv3x3_weight_pack(ptr(w), ptr(out), code(dtype), Cout, Cin, mode, ld, stream()),
               "conv3x3_weight_pack")
    return out


def conv3x3_weight_pack_batch(weights, dtype, modes, lds):
    """conv3x3_weight_pack for a list of weights in one launch (ssl4gie_conv3x3_weight_pack_batch); lds[i] None =
    the unpadded row length"""
    n = len(weights)
    if n == 0:
        return []
    outs, geo = [], []
    for w, mode, ld in zip(weights, modes, lds):
        _dev(w)
        assert w.dtype == torch.float32 and w.dim() == 4 and w.shape[2:] == (3, 3) and w.is_contiguous()
        Cout, Cin, ld, shape = _pack_shape(w, mode, ld)
        outs.append(torch.empty(shape, dtype=dtype, device=w.device))
        geo.append((Cout, Cin, mode, ld))
    vp_arr = C.c_void_p * n
    i_arr = C.c_int * n
    _lib.check(_lib.load().ssl4gie_conv3x3_weight_pack_batch(
        vp_arr(*[ptr(w) for w in weights]), vp_arr(*[ptr(o) for o in outs]), i_arr(*[g[0] for g in geo]),
        i_arr(*[g[1] for g in geo]), i_arr(*[g[2] for g in geo]), i_arr(*[g[3] for g in geo]), n, code(dtype),
        stream()), "conv3x3_weight_pack_batch")
    return outs


def conv3x3_wgrad_unpack(dw2, target, accumulate=False):
    """dw2 [Cout, ld >= 9 Cin] fp32, columns (tap, ci) -> (+)= target [Cout, Cin, 3, 3] (contiguous) in one launch"""
    _dev(dw2, target)
    Cout, Cin = target.shape[:2]
    assert dw2.dtype == torch.float32 and target.dtype == torch.float32 and target.is_contiguous()
    assert dw2.stride(1) == 1 and dw2.shape[0] == Cout and dw2.shape[1] >= 9 * Cin
    _lib.check(_lib.load().ssl4gie_conv3x3_wgrad_unpack(ptr(dw2), ptr(target), Cout, Cin, dw2.stride(0),
                                                         int(accumulate), stream()), "conv3x3_wgrad_unpack")
    return target


def stem7x7_weight(weight):
    """[64, 3, 7, 7] fp32 -> [64, 256] in the kernels' layout [co][ky (8)][kx (8)][c (4)], zeros in the padding"""
    w = torch.zeros(weight.shape[0], 8, 8, 4, dtype=weight.dtype, device=weight.device)
    w[:, :7, :7, :3] = weight.permute(0, 2, 3, 1)
    return w.reshape(weight.shape[0], 256)


def stem7x7_fwd(packed, w2s, B, H, W, colstats=False):
    """y [B,Ho,Wo,64] bf16 (+ BatchNorm partial statistics [tiles, 2, 64])"""
    _dev(packed, w2s)
    assert w2s.shape == (64, 256) and w2s.dtype == torch.bfloat16 and w2s.is_contiguous()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    L = _lib.load()
    y = torch.empty(B, Ho, Wo, 64, dtype=torch.bfloat16, device=packed.device)
    stats = torch.empty(L.ssl4gie_stem7x7_tiles(B, H, W), 2, 64, dtype=torch.float32, device=packed.device) \
        if colstats else None
    _lib.check(L.ssl4gie_stem7x7_fwd(ptr(packed), ptr(w2s), ptr(y), ptr(stats), B, H, W, stream()), "stem7x7_fwd")
    return (y, stats) if colstats else y


def stem7x7_wgrad(dy, packed, B, H, W):
    """weight gradient [64, 3, 7, 7] fp32 of the stem from dy [B,Ho,Wo,64] bf16 and the packed image"""
    _dev(dy, packed)
    assert dy.dtype == torch.bfloat16 and dy.is_contiguous() and dy.shape[-1] == 64
    L = _lib.load()
    nb = L.ssl4gie_stem7x7_wgrad_workspace_bytes(B, H, W)
    ws = torch.empty(nb, dtype=torch.uint8, device=dy.device)
    out = torch.empty(64, 7, 8, 4, dtype=torch.float32, device=dy.device)
    _lib.check(L.ssl4gie_stem7x7_wgrad(ptr(dy), ptr(packed), ptr(out), ptr(ws), nb, B, H, W, 0, stream()),
               "stem7x7_wgrad")
    return out[:, :, :7, :3].permute(0, 3, 1, 2)  # [co, c, ky, kx]


def stem3x3_ok(imgs, C0):
    """whether ssl4gie_stem3x3_{fwd,wgrad} take this image batch / width (ConvStem layer 1)"""
    return imgs.dim() == 4 and imgs.shape[1] == 3 and imgs.shape[2] >= 2 and imgs.shape[3] >= 2 \
        and C0 % 16 == 0 and 16 <= C0 <= 128


def stem3x3_fwd(imgs, weight, dtype, colstats=False):
    """nn.Conv2d(3, C0, 3, stride 2, pad 1, bias=False) on the fp32 NCHW image -> y [B,Ho,Wo,C0] in `dtype`
    (+ BatchNorm partial statistics [tiles, 2, C0]); weight = the fp32 parameter [C0, 3, 3, 3]"""
    _dev(imgs, weight)
    _f32(imgs, weight)
    assert imgs.dim() == 4 and imgs.shape[1] == 3 and imgs.is_contiguous(), "stem3x3: fp32 NCHW image, 3 channels"
    assert weight.dim() == 4 and weight.shape[1:] == (3, 3, 3) and weight.is_contiguous()
    B, _, H, W = imgs.shape
    C0 = weight.shape[0]
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    L = _lib.load()
    y = torch.empty(B, Ho, Wo, C0, dtype=dtype, device=imgs.device)
    stats = torch.empty(max(L.ssl4gie_stem3x3_tiles(B, H, W), 1), 2, C0, dtype=torch.float32, device=imgs.device) \
        if colstats else None
    _lib.check(L.ssl4gie_stem3x3_fwd(ptr(imgs), ptr(weight), ptr(y), ptr(stats), code(dtype), B, H, W, C0, stream()),
               "stem3x3_fwd")
    return (y, stats) if colstats else y


def stem3x3_wgrad(dy, imgs, out=None, accumulate=False):
    """weight gradient [C0, 3, 3, 3] fp32 (+)= of the 3x3 stride-2 stem from dy [B,Ho,Wo,C0] and the fp32 image"""
    _dev(dy, imgs, out)
    _f32(imgs)
    assert imgs.dim() == 4 and imgs.shape[1] == 3 and imgs.is_contiguous()
    B, _, H, W = imgs.shape
    C0 = dy.shape[-1]
    assert dy.is_contiguous() and dy.shape == (B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C0), dy.shape
    if out is None:
        assert not accumulate
        out = torch.empty(C0, 3, 3, 3, dtype=torch.float32, device=dy.device)
    assert out.dtype == torch.float32 and out.shape == (C0, 3, 3, 3) and out.is_contiguous()
    L = _lib.load()
    nb = L.ssl4gie_stem3x3_wgrad_workspace_bytes(code(dy.dtype), B, H, W, C0)
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=dy.device)
    _lib.check(L.ssl4gie_stem3x3_wgrad(ptr(dy), ptr(imgs), ptr(out), ptr(ws), nb, code(dy.dtype), B, H, W, C0,
                                       int(accumulate), stream()), "stem3x3_wgrad")
    return out


def col2im3x3(dcols, B, H, W, C, stride):
    _dev(dcols)
    dx = torch.empty(B, H, W, C, dtype=dcols.dtype, device=dcols.device)
    _lib.check(_lib.load().ssl4gie_col2im3x3(ptr(dcols), ptr(dx), code(dcols.dtype), B, H, W, C,
                                             stride, dcols.shape[1], stream()), "col2im3x3")
    return dx


def bilinear2x_fwd(x):
    B, H, W, C = _nhwc(x)
    y = torch.empty(B, 2 * H, 2 * W, C, dtype=x.dtype, device=x.device)
    _lib.check(_lib.load().ssl4gie_bilinear2x_fwd(ptr(x), ptr(y), code(x.dtype), B, H, W, C,
                                                  stream()), "bilinear2x_fwd")
    return y


def bilinear2x_bwd(dy):
    B, Ho, Wo, C = _nhwc(dy)
    dx = torch.empty(B, Ho // 2, Wo // 2, C, dtype=dy.dtype, device=dy.device)
    _lib.check(_lib.load().ssl4gie_bilinear2x_bwd(ptr(dy), ptr(dx), code(dy.dtype), B, Ho // 2,
                                                  Wo // 2, C, stream()), "bilinear2x_bwd")
    return dx


# ------------------------------------------------------------------ atrous glue of DeepLabV3+ (channels-last)
def _map(x, what):
    B, H, W, C = _nhwc(x)
    code(x.dtype)
    if C % (8 if x.dtype == torch.bfloat16 else 4):
        raise ValueError(f"{what}: {C} channels are not a whole number of 16-byte chunks of {x.dtype}")
    return B, H, W, C


def im2col3x3_dil(x, dilation, ld=None):
    """patch matrix [B H W, ld] of a Conv2d(k=3, stride 1, padding = dilation): im2col3x3's layout"""
    B, H, W, C = _map(x, "im2col3x3_dil")
    assert int(dilation) >= 1, dilation
    ld = ld or k_pad(9 * C, x.dtype)
    assert ld >= 9 * C and ld % (8 if x.dtype == torch.bfloat16 else 4) == 0, ld
    cols = torch.empty(B * H * W, ld, dtype=x.dtype, device=x.device)
    _lib.check(_lib.load().ssl4gie_im2col3x3_dil(ptr(x), ptr(cols), code(x.dtype), B, H, W, C, int(dilation), ld,
                                                 stream()), "im2col3x3_dil")
    return cols


def _dw_weight(w, C):
    _f32(w)
    if w.numel() != 9 * C or w.shape[0] != C or tuple(w.shape[-2:]) != (3, 3):
        raise ValueError(f"depthwise weight {tuple(w.shape)} does not fit {C} channels ([C, 1, 3, 3] or [C, 3, 3])")


def dwconv3x3_fwd(x, w, dilation, flip=False):
    """depthwise Conv2d(C, C, 3, padding = dilation, groups = C, bias=False) on x [B,H,W,C]; w fp32 [C,1,3,3] / [C,3,3];
    flip: with the weight rotated by 180 degrees (the data gradient, called on dy)"""
    _dev(w)
    B, H, W, C = _map(x, "dwconv3x3_fwd")
    assert C % 8 == 0 and int(dilation) >= 1, (C, dilation)
    _dw_weight(w, C)
    y = torch.empty_like(x)
    _lib.check(_lib.load().ssl4gie_dwconv3x3_fwd(ptr(x), ptr(w), ptr(y), code(x.dtype), B, H, W, C, int(dilation),
                                                 int(bool(flip)), stream()), "dwconv3x3_fwd")
    return y


def dwconv3x3_wgrad(dy, x, dilation, out=None, accumulate=False):
    """weight gradient [C, 1, 3, 3] fp32 (+)= of the depthwise convolution from dy and x [B,H,W,C]; deterministic"""
    _dev(dy, out)
    B, H, W, C = _map(x, "dwconv3x3_wgrad")
    assert C % 8 == 0 and int(dilation) >= 1 and dy.shape == x.shape and dy.dtype == x.dtype, (dy.shape, x.shape)
    if out is None:
        assert not accumulate
        out = torch.empty(C, 1, 3, 3, dtype=torch.float32, device=x.device)
    _dw_weight(out, C)
    L = _lib.load()
    nb = L.ssl4gie_dwconv3x3_wgrad_workspace_bytes(code(x.dtype), B, H, W, C)
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=x.device)
    _lib.check(L.ssl4gie_dwconv3x3_wgrad(ptr(dy), ptr(x), ptr(out), ptr(ws), nb, code(x.dtype), B, H, W, C,
                                         int(dilation), int(bool(accumulate)), stream()), "dwconv3x3_wgrad")
    return out


def _up_scale(scale):
    if int(scale) != scale or int(scale) < 2:
        raise ValueError(f"bilinear_up_ac: integer scale >= 2, got {scale}")
    return int(scale)


def bilinear_up_ac_fwd(x, scale):
    """nn.UpsamplingBilinear2d(scale_factor=scale) (align_corners=True): [B,H,W,C] -> [B, scale H, scale W, C]; any C"""
    B, H, W, C = _nhwc(x)
    s = _up_scale(scale)
    y = torch.empty(B, s * H, s * W, C, dtype=x.dtype, device=x.device)
    _lib.check(_lib.load().ssl4gie_bilinear_up_ac_fwd(ptr(x), ptr(y), code(x.dtype), B, H, W, C, s, stream()),
               "bilinear_up_ac_fwd")
    return y


def bilinear_up_ac_bwd(dy, scale):
    """gradient of bilinear_up_ac_fwd: dy [B, scale H, scale W, C] -> dx [B,H,W,C] (gather form, no atomics)"""
    B, Ho, Wo, C = _nhwc(dy)
    s = _up_scale(scale)
    assert Ho % s == 0 and Wo % s == 0, (dy.shape, s)
    dx = torch.empty(B, Ho // s, Wo // s, C, dtype=dy.dtype, device=dy.device)
    _lib.check(_lib.load().ssl4gie_bilinear_up_ac_bwd(ptr(dy), ptr(dx), code(dy.dtype), B, Ho // s, Wo // s, C, s,
                                                      stream()), "bilinear_up_ac_bwd")
    return dx


def chan_write(dst, offset, src):
    """dst[..., offset : offset + C] = src: one operand of a channel concatenation.  dst [B,H,W,Ct] contiguous; src
    [B,H,W,C], or [B,C] — then every pixel of image b gets row b (the up-sampling of a 1x1 map)"""
    _dev(dst, src)
    B, H, W, Ct = _nhwc(dst)
    C = src.shape[-1]
    assert src.dtype == dst.dtype and 0 <= offset and offset + C <= Ct, (src.shape, dst.shape, offset)
    assert tuple(src.shape) in ((B, H, W, C), (B, C)), (src.shape, dst.shape)
    rep = H * W if src.dim() == 2 else 1
    _lib.check(_lib.load().ssl4gie_chan_copy(ptr(src), C, dst.data_ptr() + offset * dst.element_size(), Ct,
                                             code(dst.dtype), B * H * W, C, rep, stream()), "chan_copy")
    return dst


def chan_read(src, offset, C):
    """src[..., offset : offset + C] of a contiguous [B,H,W,Ct] map as a dense [B,H,W,C] one"""
    _dev(src)
    B, H, W, Ct = _nhwc(src)
    assert 0 <= offset and offset + C <= Ct, (src.shape, offset, C)
    out = torch.empty(B, H, W, C, dtype=src.dtype, device=src.device)
    _lib.check(_lib.load().ssl4gie_chan_copy(src.data_ptr() + offset * src.element_size(), Ct, ptr(out), C,
                                             code(src.dtype), B * H * W, C, 1, stream()), "chan_copy")
    return out


def pixel_shuffle(g, bias, B, H, W, k, C):
    _dev(g, bias)
    assert g.shape == (B * H * W, k * k * C)
    y = torch.empty(B, k * H, k * W, C, dtype=g.dtype, device=g.device)
    _lib.check(_lib.load().ssl4gie_pixel_shuffle(ptr(g), ptr(bias), ptr(y), code(g.dtype), B, H, W,
                                                 k, C, stream()), "pixel_shuffle")
    return y


def pixel_unshuffle(dy, k):
    B, Ho, Wo, C = _nhwc(dy)
    H, W = Ho // k, Wo // k
    dg = torch.empty(B * H * W, k * k * C, dtype=dy.dtype, device=dy.device)
    _lib.check(_lib.load().ssl4gie_pixel_unshuffle(ptr(dy), ptr(dg), code(dy.dtype), B, H, W, k, C,
                                                   stream()), "pixel_unshuffle")
    return dg


def tokens_to_map(z, dtype):
    _dev(z)
    _f32(z)
    B, L1, D = z.shape
    x = torch.empty(B * (L1 - 1), D, dtype=dtype, device=z.device)
    _lib.check(_lib.load().ssl4gie_tokens_to_map(ptr(z), ptr(x), code(dtype), B, L1 - 1, D, stream()),
               "tokens_to_map")
    return x


def map_to_tokens(dx, B, L, D):
    _dev(dx)
    dz = torch.empty(B, L + 1, D, dtype=torch.float32, device=dx.device)
    _lib.check(_lib.load().ssl4gie_map_to_tokens(ptr(dx), ptr(dz), code(dx.dtype), B, L, D, stream()),
               "map_to_tokens")
    return dz


def eltwise_add(a, b):
    _dev(a, b)
    assert a.shape == b.shape and a.dtype == b.dtype
    out = torch.empty_like(a)
    _lib.check(_lib.load().ssl4gie_eltwise(0, ptr(a), ptr(b), None, ptr(out), code(a.dtype), a.numel(),
                                           stream()), "eltwise add")
    return out


def relu_bwd(x, g, skip=None):
    """(x > 0 ? g : 0) + skip"""
    _dev(x, g, skip)
    assert x.shape == g.shape and x.dtype == g.dtype
    out = torch.empty_like(g)
    _lib.check(_lib.load().ssl4gie_eltwise(1, ptr(x), ptr(g), ptr(skip), ptr(out), code(g.dtype),
                                           g.numel(), stream()), "relu_bwd")
    return out


def depth_head_fwd(x2d, w, bias):
    _dev(x2d, w, bias)
    _f32(w, bias)
    M, C = x2d.shape
    y = torch.empty(M, dtype=torch.float32, device=x2d.device)
    _lib.check(_lib.load().ssl4gie_depth_head_fwd(ptr(x2d), ptr(w), ptr(bias), ptr(y), code(x2d.dtype),
                                                  M, C, stream()), "depth_head_fwd")
    return y


def depth_head_bwd(x2d, w, y, dy, dw, db, accumulate):
    _dev(x2d, w, y, dy, dw, db)
    _f32(w, y, dy, dw, db)
    M, C = x2d.shape
    L = _lib.load()
    ws = torch.empty(L.ssl4gie_depth_head_bwd_workspace_bytes(M, C), dtype=torch.uint8,
                     device=x2d.device)
    dx = torch.empty_like(x2d)
    _lib.check(L.ssl4gie_depth_head_bwd(ptr(x2d), ptr(w), ptr(y), ptr(dy), ptr(dx), ptr(dw), ptr(db),
                                        int(accumulate), ptr(ws), code(x2d.dtype), M, C, stream()),
               "depth_head_bwd")
    return dx


# ------------------------------------------------------------------ ResNet glue (channels-last)
def stem_im2col7x7(imgs, dtype):
    _dev(imgs)
    _f32(imgs)
    B, C, H, W = imgs.shape
    assert C == 3
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    ld = k_pad(147, dtype) if dtype == torch.bfloat16 else 152  # multiple of 8 columns
    cols = torch.empty(B * Ho * Wo, ld, dtype=dtype, device=imgs.device)
    _lib.check(_lib.load().ssl4gie_stem_im2col7x7(ptr(imgs), ptr(cols), code(dtype), B, H, W, ld,
                                                  stream()), "stem_im2col7x7")
    return cols, Ho, Wo


def subsample2(x):
    B, H, W, C = _nhwc(x)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty(B, Ho, Wo, C, dtype=x.dtype, device=x.device)
    _lib.check(_lib.load().ssl4gie_subsample2(ptr(x), ptr(y), code(x.dtype), B, H, W, C, 0, stream()),
               "subsample2")
    return y


def subsample2_bwd(dy, H, W):
    B, Ho, Wo, C = _nhwc(dy)
    dx = torch.empty(B, H, W, C, dtype=dy.dtype, device=dy.device)
    _lib.check(_lib.load().ssl4gie_subsample2(ptr(dy), ptr(dx), code(dy.dtype), B, H, W, C, 1, stream()),
               "subsample2_bwd")
    return dx


# ------------------------------------------------------------------ BatchNorm: one binder per C entry point
# (workspace, outputs, pointers and the error tag live here; the public wrappers below only choose the source of the
# normalisation / of the ReLU mask)
def _bn_ws(rows, C, dev):
    return torch.empty(_lib.load().ssl4gie_bn_workspace_bytes(rows, C), dtype=torch.uint8, device=dev)


def _bn_fwd(source, x2d, rows, C, partials=None, gamma=None, beta=None, res=None, mean=None, rstd=None,
            running=(None, None), momentum=0.0, eps=0.0, relu=False, coef=None, want_bits=False):
    """ssl4gie_bn_fwd -> (y, bits, coef, mean, rstd).  x2d None: the coefficients-only forms (coef is the output);
    mean / rstd are allocated unless given (FROM_STATS) or unused (FROM_COEF)"""
    _dev(x2d, partials, gamma, beta, res, mean, rstd, coef, *running)
    dev = (x2d if x2d is not None else partials if partials is not None else mean).device
    y = bits = ws = None
    parts = 0
    if partials is not None:
        assert partials.dtype == torch.float32 and partials.shape[1:] == (2, C) and partials.is_contiguous()
        parts = partials.shape[0]
    if source in (_lib.BN_FROM_X, _lib.BN_FROM_PARTIALS):
        mean = torch.empty(C, dtype=torch.float32, device=dev)
        rstd = torch.empty(C, dtype=torch.float32, device=dev)
    if x2d is not None:
        y = torch.empty_like(x2d)
    else:
        coef = torch.empty(2, C, dtype=torch.float32, device=dev)
    if want_bits:
        assert x2d.dtype == torch.bfloat16
        bits = torch.empty(rows * C // 8, dtype=torch.uint8, device=dev)
    if source != _lib.BN_FROM_COEF and not (source == _lib.BN_FROM_STATS and x2d is None):
        ws = _bn_ws(rows, C, dev)
    _lib.check(_lib.load().ssl4gie_bn_fwd(
        source, ptr(x2d), ptr(partials), parts, ptr(gamma), ptr(beta), ptr(res), ptr(y), ptr(bits), ptr(coef),
        ptr(mean), ptr(rstd), ptr(running[0]), ptr(running[1]), float(momentum), float(eps), int(relu), ptr(ws),
        code(x2d.dtype) if x2d is not None else F32, rows, C, stream()), "bn_fwd")
    return y, bits, coef, mean, rstd


def _bn_stats(x2d, partials, rows, C):
    _dev(x2d, partials)
    dev = (x2d if x2d is not None else partials).device
    parts = 0
    if partials is not None:
        assert partials.dtype == torch.float32 and partials.shape[1:] == (2, C) and partials.is_contiguous()
        parts = partials.shape[0]
    mean = torch.empty(C, dtype=torch.float32, device=dev)
    var = torch.empty(C, dtype=torch.float32, device=dev)
    _lib.check(_lib.load().ssl4gie_bn_stats(ptr(x2d), ptr(partials), parts, ptr(mean), ptr(var),
                                            ptr(_bn_ws(rows, C, dev)), code(x2d.dtype) if x2d is not None else F32,
                                            rows, C, stream()), "bn_stats")
    return mean, var


def _bn_mask(kind, mask, x2d):
    _dev(mask)
    if kind == _lib.BN_MASK_BITS:
        assert mask.dtype == torch.uint8 and mask.numel() == x2d.numel() // 8
    return ptr(mask)


def _bn_bwd(dy2d, kind, mask, x2d, gamma, beta, mean, rstd, want_dres, dgamma, dbeta, accumulate):
    """ssl4gie_bn_bwd -> (dx, dres)"""
    _dev(dy2d, x2d, gamma, beta, mean, rstd, dgamma, dbeta)
    rows, C = x2d.shape
    dx = torch.empty_like(x2d)
    dres = torch.empty_like(x2d) if want_dres else None
    _lib.check(_lib.load().ssl4gie_bn_bwd(
        ptr(dy2d), kind, _bn_mask(kind, mask, x2d), ptr(x2d), ptr(gamma), ptr(beta), ptr(mean), ptr(rstd), ptr(dx),
        ptr(dres), ptr(dgamma), ptr(dbeta), int(accumulate), ptr(_bn_ws(rows, C, x2d.device)), code(x2d.dtype), rows,
        C, stream()), "bn_bwd")
    return dx, dres


def _bn_bwd_reduce(dy2d, kind, mask, x2d, gamma, beta, mean, rstd, want_dres):
    """ssl4gie_bn_bwd_reduce -> (LOCAL sums [2, C], dres)"""
    _dev(dy2d, x2d, gamma, beta, mean, rstd)
    rows, C = x2d.shape
    sums = torch.empty(2, C, dtype=torch.float32, device=x2d.device)
    dres = torch.empty_like(x2d) if want_dres else None
    _lib.check(_lib.load().ssl4gie_bn_bwd_reduce(
        ptr(dy2d), kind, _bn_mask(kind, mask, x2d), ptr(x2d), ptr(gamma), ptr(beta), ptr(mean), ptr(rstd), ptr(dres),
        ptr(sums), ptr(_bn_ws(rows, C, x2d.device)), code(x2d.dtype), rows, C, stream()), "bn_bwd_reduce")
    return sums, dres


def _bn_bwd_apply(dy2d, kind, mask, x2d, gamma, beta, mean, rstd, sums, inv_count):
    """ssl4gie_bn_bwd_apply -> dx from the GLOBAL sums and 1 / (global row count)"""
    _dev(dy2d, x2d, gamma, beta, mean, rstd, sums)
    rows, C = x2d.shape
    dx = torch.empty_like(x2d)
    _lib.check(_lib.load().ssl4gie_bn_bwd_apply(
        ptr(dy2d), kind, _bn_mask(kind, mask, x2d), ptr(x2d), ptr(gamma), ptr(beta), ptr(mean), ptr(rstd), ptr(sums),
        float(inv_count), ptr(dx), ptr(_bn_ws(rows, C, x2d.device)), code(x2d.dtype), rows, C, stream()),
        "bn_bwd_apply")
    return dx


def _relu_mask(relu, y2d):
    return (_lib.BN_MASK_Y, y2d) if relu else (_lib.BN_MASK_NONE, None)


def bn_fwd(x2d, gamma, beta, res, running_mean, running_var, momentum, eps, relu, training,
           mean=None, rstd=None, partials=None):
    """`partials` [parts, 2, C]: training-mode statistics from the producing GEMM's epilogue
    (linear_fwd / conv3x3_fwd with colstats=True) instead of a pass over x2d; not training: mean / rstd are inputs"""
    rows, C = x2d.shape
    if not training:
        y = _bn_fwd(_lib.BN_FROM_STATS, x2d, rows, C, None, gamma, beta, res, mean, rstd, eps=eps, relu=relu)[0]
        return y, mean, rstd
    y, _, _, mean, rstd = _bn_fwd(_lib.BN_FROM_X if partials is None else _lib.BN_FROM_PARTIALS, x2d, rows, C,
                                  partials, gamma, beta, res, running=(running_mean, running_var),
                                  momentum=momentum, eps=eps, relu=relu)
    return y, mean, rstd


def bn_fwd_bits(x2d, gamma, beta, res, running_mean, running_var, momentum, eps, partials):
    """training-mode BatchNorm (+ residual) + ReLU from GEMM-epilogue partials that also writes the ReLU mask as
    a bit map [rows * C / 8] (bf16): -> (y, bits, mean, rstd)"""
    y, bits, _, mean, rstd = _bn_fwd(_lib.BN_FROM_PARTIALS, x2d, *x2d.shape, partials, gamma, beta, res,
                                     running=(running_mean, running_var), momentum=momentum, eps=eps, relu=True,
                                     want_bits=True)
    return y, bits, mean, rstd


def bn_coef_stats(mean, rstd, gamma, beta):
    """coef [2, C] (y = x coef[0] + coef[1]) of a BatchNorm whose statistics are given — the GLOBAL ones a
    SyncBatchNorm exchange returned"""
    return _bn_fwd(_lib.BN_FROM_STATS, None, 0, mean.numel(), None, gamma, beta, None, mean, rstd)[2]


def bn_apply_bits(x2d, coef, res):
    """relu(x coef[0] + coef[1] (+ res)) + the ReLU bit map (bf16): the apply half of bn_fwd_bits with given
    coefficients -> (y, bits)"""
    rows, C = x2d.shape
    assert coef.shape == (2, C) and coef.is_contiguous()
    return _bn_fwd(_lib.BN_FROM_COEF, x2d, rows, C, res=res, relu=True, coef=coef, want_bits=True)[:2]


def bn_bwd(dy2d, y2d, x2d, gamma, mean, rstd, relu, want_dres, dgamma, dbeta, accumulate):
    return _bn_bwd(dy2d, *_relu_mask(relu, y2d), x2d, gamma, None, mean, rstd, want_dres, dgamma, dbeta, accumulate)


def bn_bwd_bits(dy2d, bits, x2d, gamma, mean, rstd, dgamma, dbeta, accumulate):
    """backward of bn_fwd_bits: -> (dx, dres = the masked gradient)"""
    return _bn_bwd(dy2d, _lib.BN_MASK_BITS, bits, x2d, gamma, None, mean, rstd, True, dgamma, dbeta, accumulate)


def bn_bwd_xmask(dy2d, x2d, gamma, beta, mean, rstd, dgamma, dbeta, accumulate):
    """BatchNorm + ReLU without a residual input: the mask is rebuilt from x and the forward's coefficients, the
    ReLU output is not read"""
    return _bn_bwd(dy2d, _lib.BN_MASK_X, None, x2d, gamma, beta, mean, rstd, False, dgamma, dbeta, accumulate)[0]


def bn_bwd_frozen(dy2d, mask_kind, mask, x2d, gamma, beta, mean, rstd, want_dres, dgamma, dbeta, accumulate):
    """ssl4gie_bn_bwd_frozen: backward through FIXED statistics (evaluation mode, FrozenBatchNorm2d) -> (dx, dres):
    dx = rstd gamma g with g the masked dy, dres = g; dgamma / dbeta (targets, or None) overwritten or accumulated.
    x2d and mean are passed for MASK_X or with dgamma only, beta for MASK_X only (None otherwise, as the C ABI asks);
    without parameter gradients it is one flat pass and there is no workspace"""
    _dev(dy2d, x2d, gamma, beta, mean, rstd, dgamma, dbeta)
    _f32(gamma, beta, mean, rstd, dgamma, dbeta)
    rows, C = dy2d.shape
    assert x2d is None or (x2d.shape == dy2d.shape and x2d.dtype == dy2d.dtype)
    if mask_kind == _lib.BN_MASK_Y:
        assert mask.shape == dy2d.shape and mask.dtype == dy2d.dtype
    dx = torch.empty_like(dy2d)
    dres = torch.empty_like(dy2d) if want_dres else None
    ws = _bn_ws(rows, C, dy2d.device) if (dgamma is not None or dbeta is not None) else None
    _lib.check(_lib.load().ssl4gie_bn_bwd_frozen(
        ptr(dy2d), mask_kind, _bn_mask(mask_kind, mask, dy2d), ptr(x2d), ptr(gamma), ptr(beta), ptr(mean), ptr(rstd),
        ptr(dx), ptr(dres), ptr(dgamma), ptr(dbeta), int(accumulate), ptr(ws), code(dy2d.dtype), rows, C, stream()),
        "bn_bwd_frozen")
    return dx, dres


def maxpool3x3s2_fwd(x, coef=None, relu=False):
    """coef [2, C] (ops.bn_coef_partials): the pool runs over act(x coef[0] + coef[1]) — BatchNorm (+ ReLU) applied
    on the way in (ssl4gie_bn_maxpool3x3s2_fwd)"""
    B, H, W, C = _nhwc(x)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty(B, Ho, Wo, C, dtype=x.dtype, device=x.device)
    arg = torch.empty(B, Ho, Wo, C, dtype=torch.uint8, device=x.device)
    if coef is not None:
        _dev(coef); _f32(coef)
        assert coef.shape == (2, C) and coef.is_contiguous()
        _lib.check(_lib.load().ssl4gie_bn_maxpool3x3s2_fwd(ptr(x), ptr(coef), int(bool(relu)), ptr(y), ptr(arg),
                                                           code(x.dtype), B, H, W, C, stream()), "bn_maxpool_fwd")
        return y, arg
    _lib.check(_lib.load().ssl4gie_maxpool3x3s2_fwd(ptr(x), ptr(y), ptr(arg), code(x.dtype), B, H, W, C,
                                                    stream()), "maxpool_fwd")
    return y, arg


def maxpool3x3s2_bwd(dy, arg, H, W):
    B, Ho, Wo, C = _nhwc(dy)
    dx = torch.empty(B, H, W, C, dtype=dy.dtype, device=dy.device)
    _lib.check(_lib.load().ssl4gie_maxpool3x3s2_bwd(ptr(dy), ptr(arg), ptr(dx), code(dy.dtype), B, H, W,
                                                    C, stream()), "maxpool_bwd")
    return dx


def avgpool_fwd(x):
    B, H, W, C = _nhwc(x)
    y = torch.empty(B, C, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().ssl4gie_avgpool_fwd(ptr(x), ptr(y), code(x.dtype), B, H * W, C, stream()),
               "avgpool_fwd")
    return y


def avgpool_bwd(dy, H, W, dtype):
    _dev(dy)
    _f32(dy)
    B, C = dy.shape
    dx = torch.empty(B, H, W, C, dtype=dtype, device=dy.device)
    _lib.check(_lib.load().ssl4gie_avgpool_bwd(ptr(dy), ptr(dx), code(dtype), B, H * W, C, stream()),
               "avgpool_bwd")
    return dx


# ------------------------------------------------------------------ SyncBatchNorm pieces / MoCo EMA
def bn_stats(x2d, partials=None):
    """local batch statistics (mean, biased variance) of the rows of x2d, fp32 [C] each; from the
    producing GEMM's `partials` [parts, 2, C] when given"""
    return _bn_stats(x2d if partials is None else None, partials, *x2d.shape)


def bn_stats_from_partials(partials, rows):
    """local (mean, biased variance) of a map known only through its producer's partials [parts, 2, C] (the
    statistics-only product of linear_colstats_only: the map itself is never written)"""
    return _bn_stats(None, partials, rows, partials.shape[2])


def bn_bwd_reduce(dy2d, y2d, x2d, mean, rstd, relu, want_dres):
    return _bn_bwd_reduce(dy2d, *_relu_mask(relu, y2d), x2d, None, None, mean, rstd, want_dres)


def bn_bwd_reduce_bits(dy2d, bits, x2d, mean, rstd):
    """SyncBatchNorm + residual + ReLU backward, first half with the mask from the forward's bit map:
    -> (LOCAL sums [2, C], dres = the masked gradient)"""
    return _bn_bwd_reduce(dy2d, _lib.BN_MASK_BITS, bits, x2d, None, None, mean, rstd, True)


def bn_bwd_reduce_xmask(dy2d, x2d, gamma, beta, mean, rstd):
    """SyncBatchNorm + ReLU (no residual) backward, first half with the mask rebuilt from x: LOCAL sums [2, C]"""
    return _bn_bwd_reduce(dy2d, _lib.BN_MASK_X, None, x2d, gamma, beta, mean, rstd, False)[0]


def bn_bwd_apply_xmask(dy2d, x2d, gamma, beta, mean, rstd, sums, inv_count):
    """... second half: dx from the GLOBAL sums and 1 / (global row count)"""
    return _bn_bwd_apply(dy2d, _lib.BN_MASK_X, None, x2d, gamma, beta, mean, rstd, sums, inv_count)


def bn_bwd_apply(dy2d, y2d, x2d, gamma, mean, rstd, sums, inv_count, relu):
    return _bn_bwd_apply(dy2d, *_relu_mask(relu, y2d), x2d, gamma, None, mean, rstd, sums, inv_count)


def ema_update(dst, src, m):
    """dst = dst * m + src * (1 - m) on flat fp32 tensors"""
    _dev(dst, src)
    _f32(dst, src)
    assert dst.numel() == src.numel()
    _lib.check(_lib.load().ssl4gie_ema_update(ptr(dst), ptr(src), float(m), dst.numel(), stream()),
               "ema_update")


# ------------------------------------------------------------------ detection pyramid glue (channels-last)
def maxpool2x2_fwd(x):
    B, H, W, C_ = _nhwc(x)
    y = torch.empty(B, H // 2, W // 2, C_, dtype=x.dtype, device=x.device)
    _lib.check(_lib.load().ssl4gie_maxpool2x2_fwd(ptr(x), ptr(y), code(x.dtype), B, H, W, C_, stream()),
               "maxpool2x2_fwd")
    return y


def maxpool2x2_bwd(x, dy):
    B, H, W, C_ = _nhwc(x)
    _dev(dy)
    dx = torch.empty_like(x)
    _lib.check(_lib.load().ssl4gie_maxpool2x2_bwd(ptr(x), ptr(dy), ptr(dx), code(x.dtype), B, H, W, C_,
                                                  stream()), "maxpool2x2_bwd")
    return dx


def gelu_map(x, dy=None):
    """gelu(x) (exact erf form), or dy * gelu'(x) when dy is given"""
    _dev(x, dy)
    out = torch.empty_like(x)
    _lib.check(_lib.load().ssl4gie_gelu_map(ptr(x), ptr(dy), ptr(out), code(x.dtype), x.numel(), stream()),
               "gelu_map")
    return out


def map_layernorm_fwd(x, w, bias, eps=1e-5):
    """nn.LayerNorm over everything but the batch axis; w / bias fp32 in x's element order"""
    _dev(x, w, bias)
    _f32(w)
    _f32(bias)
    B = x.shape[0]
    M = x.numel() // B
    assert w.numel() == M and bias.numel() == M and x.is_contiguous()
    L = _lib.load()
    y = torch.empty_like(x)
    mean = torch.empty(B, dtype=torch.float32, device=x.device)
    rstd = torch.empty(B, dtype=torch.float32, device=x.device)
    ws = torch.empty(L.ssl4gie_map_layernorm_workspace_bytes(B), dtype=torch.uint8, device=x.device)
    _lib.check(L.ssl4gie_map_layernorm_fwd(ptr(x), ptr(w), ptr(bias), ptr(y), ptr(mean), ptr(rstd), eps,
                                           ptr(ws), code(x.dtype), B, M, stream()), "map_layernorm_fwd")
    return y, mean, rstd


def map_layernorm_bwd(x, dy, w, mean, rstd, dw=None, db=None, accumulate=False):
    _dev(x, dy, w, mean, rstd, dw, db)
    B = x.shape[0]
    M = x.numel() // B
    L = _lib.load()
    dx = torch.empty_like(x)
    ws = torch.empty(L.ssl4gie_map_layernorm_workspace_bytes(B), dtype=torch.uint8, device=x.device)
    _lib.check(L.ssl4gie_map_layernorm_bwd(ptr(x), ptr(dy), ptr(w), ptr(mean), ptr(rstd), ptr(dx), ptr(dw),
                                           ptr(db), int(accumulate), ptr(ws), code(x.dtype), B, M,
                                           stream()), "map_layernorm_bwd")
    return dx


IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def normalize_u8(img_u8, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """uint8 HWC batch [B, H, W, 3] on the device -> fp32 NCHW, (x / 255 - mean) / std
    (ToTensor + Normalize of the reference's dataloaders, without the PIL / CPU round trip)"""
    _dev(img_u8)
    assert img_u8.dtype == torch.uint8 and img_u8.dim() == 4 and img_u8.shape[3] == 3 and img_u8.is_contiguous()
    B, H, W, _ = img_u8.shape
    out = torch.empty(B, 3, H, W, dtype=torch.float32, device=img_u8.device)
    m = (C.c_float * 3)(*mean)
    s = (C.c_float * 3)(*std)
    _lib.check(_lib.load().ssl4gie_normalize_u8(ptr(img_u8), ptr(out), m, s, B, H, W, stream()), "normalize_u8")
    return out


_FILTERS = {"bilinear": _lib.FILTER_BILINEAR, "bicubic": _lib.FILTER_BICUBIC}


def view_sample_u8(bank, index, box, flip, S, filter="bicubic", mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """Random-resized-crop views out of a uint8 image bank [n, Hs, Ws, 3] on the device -> fp32 NCHW [B, 3, S, S]:
    sample b is image index[b] (int64 [B]) cropped to box[b] = (top, left, height, width) (int32 [B, 4]), resampled
    to S x S with PIL's antialiased `filter`, mirrored where flip[b] != 0 (uint8 [B] or None), clamped to
    [0, 255], (v / 255 - mean) / std  (RandomResizedCrop + RandomHorizontalFlip + ToTensor + Normalize of
    main_pretrain.py:123-127 once the boxes are drawn).  An index or box that does not lie inside the bank
    gives an all-NaN sample; `filter` may also be the C ABI's integer code."""
    _dev(bank, index, box, flip)
    assert bank.dtype == torch.uint8 and bank.dim() == 4 and bank.shape[3] == 3
    assert index.dtype == torch.int64 and index.dim() == 1
    B = index.shape[0]
    assert box.dtype == torch.int32 and tuple(box.shape) == (B, 4)
    assert flip is None or (flip.dtype == torch.uint8 and tuple(flip.shape) == (B,))
    n, Hs, Ws, _ = bank.shape
    f = _FILTERS[filter] if isinstance(filter, str) else int(filter)
    out = torch.empty(B, 3, S, S, dtype=torch.float32, device=bank.device)
    if B == 0:
        return out
    m = (C.c_float * 3)(*mean)
    s = (C.c_float * 3)(*std)
    _lib.check(_lib.load().ssl4gie_view_sample_u8(ptr(bank), n, Hs, Ws, ptr(index), ptr(box), ptr(flip), ptr(out),
                                                  B, S, f, m, s, stream()), "view_sample_u8")
    return out


def _u8_images(name, img):
    if not (img.dtype == torch.uint8 and img.dim() == 4 and img.shape[3] == 3 and img.shape[1] == img.shape[2]
            and img.is_contiguous()):
        raise ValueError(f"{name} needs contiguous uint8 images [B, S, S, 3], got {img.dtype} {tuple(img.shape)}")
    if img.shape[1] < 4 or img.shape[1] % 4:
        raise ValueError(f"{name} needs S >= 4 and a multiple of 4, got {img.shape[1]}")


def quantize_u8(x, out=None):
    """fp32 NCHW [B, 3, S, S] in 0..255 units (view_sample_u8 with mean 0, std 1 / 255) -> uint8 NHWC [B, S, S, 3]:
    clamp to [0, 255], add 0.5 in fp32, truncate; a NaN gives 0.  The one rounding between the engine's fp32 resample and
    the uint8 ops of RandAugment (PIL rounds after each resize pass)."""
    _dev(x, out)
    _f32(x)
    if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3] or x.shape[2] % 4 or not x.is_contiguous():
        raise ValueError(f"quantize_u8 needs contiguous x [B, 3, S, S] with S a multiple of 4, got {tuple(x.shape)}")
    B, _, S, _ = x.shape
    if out is None:
        out = torch.empty(B, S, S, 3, dtype=torch.uint8, device=x.device)
    _u8_images("quantize_u8 (out)", out)
    assert tuple(out.shape) == (B, S, S, 3)
    _lib.check(_lib.load().ssl4gie_quantize_u8(ptr(x), ptr(out), B, S, stream()), "quantize_u8")
    return out


def randaug_layer_workspace(B, device):
    """the histogram workspace of randaug_layer for up to B samples"""
    return torch.empty(_lib.load().ssl4gie_randaug_layer_workspace_bytes(B), dtype=torch.uint8, device=device)


def randaug_layer(img, op, arg, matrix, fill, out=None, workspace=None):
    """One RandAugment layer on uint8 NHWC images [B, S, S, 3]: out[b] = op[b] applied to img[b].  op uint8 [B] holds
    timm's op ids (0 AutoContrast, 1 Equalize, 2 Invert, 3 Rotate, 4 Posterize, 5 Solarize, 6 SolarizeAdd, 7 Color,
    8 Contrast, 9 Brightness, 10 Sharpness, 11 ShearX, 12 ShearY, 13 TranslateX, 14 TranslateY; any other id, 255 by
    convention, copies), arg fp32 [B] the bits / threshold / addend / factor, matrix fp64 [B, 6] PIL's AFFINE
    coefficients of the geometric ops (bicubic, `fill` = three byte values where the source lies outside).  PIL's rules,
    bit for bit (include/ssl4gie_hip.h spells them out).  `out` must not share memory with img; `workspace`: a uint8
    buffer from randaug_layer_workspace, allocated when None."""
    _dev(img, op, arg, matrix, out, workspace)
    _u8_images("randaug_layer", img)
    B, S = img.shape[0], img.shape[1]
    if op.dtype != torch.uint8 or tuple(op.shape) != (B,) or not op.is_contiguous():
        raise ValueError(f"op must be contiguous uint8 [{B}], got {op.dtype} {tuple(op.shape)}")
    if arg.dtype != torch.float32 or tuple(arg.shape) != (B,) or not arg.is_contiguous():
        raise ValueError(f"arg must be contiguous float32 [{B}], got {arg.dtype} {tuple(arg.shape)}")
    if matrix.dtype != torch.float64 or tuple(matrix.shape) != (B, 6) or not matrix.is_contiguous():
        raise ValueError(f"matrix must be contiguous float64 [{B}, 6], got {matrix.dtype} {tuple(matrix.shape)}")
    if out is None:
        out = torch.empty_like(img)
    _u8_images("randaug_layer (out)", out)
    if tuple(out.shape) != tuple(img.shape) or out.data_ptr() == img.data_ptr():
        raise ValueError("out must have img's shape and must not be img")
    L = _lib.load()
    if workspace is None:
        workspace = randaug_layer_workspace(B, img.device)
    assert workspace.dtype == torch.uint8 and workspace.numel() >= L.ssl4gie_randaug_layer_workspace_bytes(B)
    f = (C.c_ubyte * 3)(*(int(v) for v in fill))
    _lib.check(L.ssl4gie_randaug_layer(ptr(img), ptr(out), ptr(op), ptr(arg), ptr(matrix), f, ptr(workspace), B, S,
                                       stream()), "randaug_layer")
    return out


_ERASE_MODES = {"const": _lib.ERASE_CONST, "rand": _lib.ERASE_RAND, "pixel": _lib.ERASE_PIXEL}


def normalize_erase_u8(img_u8, box, mode="pixel", seed=0, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """ToTensor + Normalize + timm's RandomErasing in one pass: uint8 NHWC [B, S, S, 3] -> fp32 NCHW.  box int32 [B, 4] =
    (top, left, h, w); h == 0 or w == 0 erases nothing; outside the box the result has normalize_u8's bits.  Inside:
    `pixel` N(0, 1) noise per element, `rand` one N(0, 1) value per channel, `const` zeros.  The noise is a pure
    function of (seed, b, c, y, x) — Philox4x32-10 and a fp32 Box-Muller, include/ssl4gie_hip.h — so the same seed gives
    the same bits whatever B is.  A box that does not lie inside the image gives an all-NaN sample."""
    _dev(img_u8, box)
    _u8_images("normalize_erase_u8", img_u8)
    B, S = img_u8.shape[0], img_u8.shape[1]
    if box.dtype != torch.int32 or tuple(box.shape) != (B, 4) or not box.is_contiguous():
        raise ValueError(f"box must be contiguous int32 [{B}, 4], got {box.dtype} {tuple(box.shape)}")
    if mode not in _ERASE_MODES:
        raise ValueError(f"mode must be 'const', 'rand' or 'pixel', got {mode!r}")
    out = torch.empty(B, 3, S, S, dtype=torch.float32, device=img_u8.device)
    m = (C.c_float * 3)(*mean)
    s = (C.c_float * 3)(*std)
    _lib.check(_lib.load().ssl4gie_normalize_erase_u8(ptr(img_u8), ptr(out), m, s, ptr(box), _ERASE_MODES[mode],
                                                      int(seed) & 0xffffffffffffffff, B, S, stream()),
               "normalize_erase_u8")
    return out


def color_augment(x, factors, order, flags, sigma, mean=IMAGENET_MEAN, std=IMAGENET_STD, out=None):
    """The colour half of MoCo-v3's augmentation on fp32 [B, 3, S, S] images in [0, 1] (view_sample_u8 with
    mean 0, std 1), per-sample parameters given as device arrays (data.ColorAugment draws them): colour jitter —
    order uint8 [B, 4] holds the op ids 0 brightness, 1 contrast, 2 saturation, 3 hue in the order they apply, 255 =
    skip; factors fp32 [B, 4] = (b, c, s, h) —, grayscale where flags[b] & 1, a true Gaussian blur of sigma[b]
    (fp32 [B]; 0 = none, R = ceil(3 sigma) <= 6, symmetric edges), solarize at 128 / 255 where flags[b] & 2
    (flags uint8 [B]), then (x - mean) / std.  The rule is spelled out in include/ssl4gie_hip.h.  Returns the new
    fp32 [B, 3, S, S]; `out`, if given, must not share memory with x (the blur reads its neighbours' inputs)."""
    return _color_stage("color_augment", 8, x, factors, order, flags, sigma, mean, std, out)


def color_augment_ft(x, factors, order, flags, sigma, mean=IMAGENET_MEAN, std=IMAGENET_STD, out=None):
    """The colour stage of the finetune loaders (ColorJitter -> GaussianBlur((25, 25), sigma) -> Normalize): the
    arguments and rule of color_augment, but the blur is torchvision's tensor-path one — 25 taps, k in [-12, 12],
    weights exp(-k^2 / 2 sigma^2) over their sum, REFLECT edges (index -i reads i) — hence S >= 16.  sigma[b] = 0: none.
    `out`, if given, must not share memory with x."""
    return _color_stage("color_augment_ft", 16, x, factors, order, flags, sigma, mean, std, out)


def _color_stage(name, s_min, x, factors, order, flags, sigma, mean, std, out):
    _dev(x, factors, order, flags, sigma, out)
    _f32(x, factors, sigma, out)
    if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3]:
        raise ValueError(f"{name} needs x [B, 3, S, S], got {tuple(x.shape)}")
    B, _, S, _ = x.shape
    if S < s_min or S % 4:
        raise ValueError(f"{name} needs S >= {s_min} and a multiple of 4, got {S}")
    if order.dtype != torch.uint8 or flags.dtype != torch.uint8:
        raise TypeError(f"order and flags must be uint8, got {order.dtype} and {flags.dtype}")
    if tuple(factors.shape) != (B, 4) or tuple(order.shape) != (B, 4) or tuple(flags.shape) != (B,) \
            or tuple(sigma.shape) != (B,):
        raise ValueError(f"{name} needs factors [B, 4], order [B, 4], flags [B], sigma [B]")
    if any(t.device != x.device for t in (factors, order, flags, sigma)):
        raise ValueError(f"{name} needs all its tensors on one device")
    if out is None:
        out = torch.empty_like(x)
    else:
        if out.shape != x.shape or out.device != x.device:
            raise ValueError("out must have x's shape and device")
        nbytes = x.numel() * 4
        if out.data_ptr() < x.data_ptr() + nbytes and x.data_ptr() < out.data_ptr() + nbytes:
            raise ValueError(f"{name} cannot run in place: out shares memory with x")
    if B == 0:
        return out
    L = _lib.load()
    ws = torch.empty(L.ssl4gie_color_augment_workspace_bytes(B, S), dtype=torch.uint8, device=x.device)
    m = (C.c_float * 3)(*mean)
    s = (C.c_float * 3)(*std)
    _lib.check(getattr(L, "ssl4gie_" + name)(ptr(x), ptr(out), B, S, ptr(factors), ptr(order), ptr(flags), ptr(sigma), m, s,
                                              ptr(ws), ws.numel(), stream()), name)
    return out


_TGT_CODES = {torch.uint8: _lib.TGT_U8, torch.uint16: _lib.TGT_U16, torch.int16: _lib.TGT_U16,
              torch.float32: _lib.TGT_F32}


def paired_warp(img, matrix, flip, fill_img, tgt_bank=None, index=None, fill_tgt=0.0):
    """Flips + nearest-neighbour affine of the finetune loaders on a device batch and, through the same map in the
    same launch, on its targets.  img fp32 [B, 3, S, S]; matrix fp32 [B, 6] (data.affine_matrices: torchvision's
    inverse matrix) or None = identity; flip uint8 [B] (bit 0 horizontal, bit 1 vertical) or None; fill_img three
    floats, the value of the image where the map leaves it.  With tgt_bank ([n, S, S] uint8, uint16 — int16 storage
    is read as uint16 — or fp32) and index (int64 [B]) the target of sample b is tgt_bank[index[b]] scaled by 1 / 255,
    1 / 65535 or 1, filled with fill_tgt; an index outside the bank gives an all-NaN target.  The rule is spelled
    out in include/ssl4gie_hip.h.  Returns img_out, or (img_out, tgt_out fp32 [B, 1, S, S])."""
    _dev(img, matrix, flip, tgt_bank, index)
    _f32(img, matrix)
    if img.dim() != 4 or img.shape[1] != 3 or img.shape[2] != img.shape[3]:
        raise ValueError(f"paired_warp needs img [B, 3, S, S], got {tuple(img.shape)}")
    B, _, S, _ = img.shape
    if S < 4 or S % 4:
        raise ValueError(f"paired_warp needs S >= 4 and a multiple of 4, got {S}")
    if matrix is not None and tuple(matrix.shape) != (B, 6):
        raise ValueError(f"matrix must be [{B}, 6], got {tuple(matrix.shape)}")
    if flip is not None and (flip.dtype != torch.uint8 or tuple(flip.shape) != (B,)):
        raise ValueError(f"flip must be uint8 [{B}]")
    if len(fill_img) != 3:
        raise ValueError("fill_img must hold three values")
    if (tgt_bank is None) != (index is None):
        raise ValueError("tgt_bank and index come together")
    tgt_out, dtype, n = None, 0, 0
    if tgt_bank is not None:
        if tgt_bank.dtype not in _TGT_CODES:
            raise TypeError(f"tgt_bank must be uint8, uint16, int16 or float32, got {tgt_bank.dtype}")
        if tgt_bank.dim() != 3 or tuple(tgt_bank.shape[1:]) != (S, S) or tgt_bank.shape[0] < 1:
            raise ValueError(f"tgt_bank must be [n, {S}, {S}], got {tuple(tgt_bank.shape)}")
        if index.dtype != torch.int64 or tuple(index.shape) != (B,):
            raise ValueError(f"index must be int64 [{B}]")
        dtype, n = _TGT_CODES[tgt_bank.dtype], tgt_bank.shape[0]
        tgt_out = torch.empty(B, 1, S, S, dtype=torch.float32, device=img.device)
    if any(t is not None and t.device != img.device for t in (matrix, flip, tgt_bank, index)):
        raise ValueError("paired_warp needs all its tensors on one device")
    img_out = torch.empty_like(img)
    if B:
        fill = (C.c_float * 3)(*fill_img)
        _lib.check(_lib.load().ssl4gie_paired_warp(ptr(img), ptr(img_out), ptr(tgt_bank), dtype, n, ptr(index),
                                                   ptr(tgt_out), ptr(matrix), ptr(flip), fill, float(fill_tgt), B, S,
                                                   stream()), "paired_warp")
    return img_out if tgt_out is None else (img_out, tgt_out)


# ------------------------------------------------------------------ detection input pipeline (csrc/color_ops.hip)
def _det_bank(name, pixels, offsets, sizes, index):
    _dev(pixels, offsets, sizes, index)
    if pixels.dtype != torch.uint8 or pixels.dim() != 1 or not pixels.is_contiguous() or pixels.numel() < 1:
        raise ValueError(f"{name} needs pixels as a contiguous uint8 vector")
    if sizes.dtype != torch.int32 or sizes.dim() != 2 or sizes.shape[1] != 2 or sizes.shape[0] < 1 \
            or not sizes.is_contiguous():
        raise ValueError(f"{name} needs sizes int32 [n, 2]")
    n = sizes.shape[0]
    if offsets.dtype != torch.int64 or tuple(offsets.shape) != (n,) or not offsets.is_contiguous():
        raise ValueError(f"{name} needs offsets int64 [{n}]")
    if index.dtype != torch.int64 or index.dim() != 1 or not index.is_contiguous():
        raise ValueError(f"{name} needs index as a contiguous int64 vector")
    if any(t.device != pixels.device for t in (offsets, sizes, index)):
        raise ValueError(f"{name} needs all its tensors on one device")
    return n, index.shape[0]


def det_color(pixels, offsets, sizes, index, factors, order, sigma, max_hw, scratch=None):
    """The colour stage of the detection train loader (ColorJitter -> GaussianBlur((25, 25), sigma)) on the stored
    H0 x W0 rectangles of a ragged uint8 bank (data.RaggedImageBank's pixels / offsets / sizes): sample b is image
    index[b]; factors fp32 [B, 4], order uint8 [B, 4], sigma fp32 [B] as in color_augment_ft.  max_hw = (largest H0,
    largest W0) of this batch, which the caller knows on the host.  Returns the scratch fp32 [B, 3, plane_stride]
    (rows dense at pitch W0, values in [0, 1] up to the blur's rounding, not normalised) that det_geometry reads;
    `scratch`, if given, is written instead and decides plane_stride: it must be >= the largest H0 * W0 of the batch
    (which can be less than max_hw's product); the kernels check it per sample, one that does not fit comes out NaN."""
    n, B = _det_bank("det_color", pixels, offsets, sizes, index)
    _dev(factors, order, sigma, scratch)
    _f32(factors, sigma, scratch)
    if order.dtype != torch.uint8:
        raise TypeError(f"order must be uint8, got {order.dtype}")
    if tuple(factors.shape) != (B, 4) or tuple(order.shape) != (B, 4) or tuple(sigma.shape) != (B,):
        raise ValueError("det_color needs factors [B, 4], order [B, 4], sigma [B]")
    max_h, max_w = int(max_hw[0]), int(max_hw[1])
    if min(max_h, max_w) < 13:
        raise ValueError(f"det_color needs max_hw >= (13, 13), got {(max_h, max_w)}")
    if scratch is None:
        scratch = torch.empty(B, 3, (max_h * max_w + 3) & ~3, dtype=torch.float32, device=pixels.device)
    elif scratch.dim() != 3 or tuple(scratch.shape[:2]) != (B, 3) or scratch.shape[2] < 169 or not scratch.is_contiguous():
        raise ValueError(f"scratch must be contiguous fp32 [{B}, 3, plane_stride], got {tuple(scratch.shape)}")
    if any(t.device != pixels.device for t in (factors, order, sigma, scratch)):
        raise ValueError("det_color needs all its tensors on one device")
    if B == 0:
        return scratch
    L = _lib.load()
    ws = torch.empty(L.ssl4gie_det_color_workspace_bytes(B), dtype=torch.uint8, device=pixels.device)
    _lib.check(L.ssl4gie_det_color(ptr(pixels), pixels.numel(), ptr(offsets), ptr(sizes), n, ptr(index), B, max_h, max_w,
                                   ptr(factors), ptr(order), ptr(sigma), ptr(scratch), scratch.shape[2], ptr(ws),
                                   ws.numel(), stream()), "det_color")
    return scratch


def det_geometry(pixels, offsets, sizes, index, geom, F, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), scratch=None):
    """rot90 / hflip / vflip, the antialiased bicubic halving when a side exceeds F, the centre pad to F x F and
    (x - mean) / std of the detection loaders, in one launch: fp32 [B, 3, F, F].  geom uint8 [B] (bit 0 hflip, bit 1
    vflip, bit 2 rot90) or None.  The source is `scratch` (det_color's result for the same index) or, without it, the
    uint8 bank itself through v / 255 — the val / test loaders' path.  The padding is the normalised value of black.
    A sample whose index is outside the bank, or whose image does not fit F x F after the halving, is all NaN."""
    n, B = _det_bank("det_geometry", pixels, offsets, sizes, index)
    _dev(geom, scratch)
    _f32(scratch)
    F = int(F)
    if F < 4 or F % 4:
        raise ValueError(f"det_geometry needs F >= 4 and a multiple of 4, got {F}")
    if geom is not None and (geom.dtype != torch.uint8 or tuple(geom.shape) != (B,) or geom.device != pixels.device):
        raise ValueError(f"geom must be uint8 [{B}] on the bank's device")
    if len(mean) != 3 or len(std) != 3 or any(float(v) == 0.0 for v in std):
        raise ValueError("mean and std must hold three values, std none equal to 0")
    stride = 0
    if scratch is not None:
        if scratch.dim() != 3 or tuple(scratch.shape[:2]) != (B, 3) or not scratch.is_contiguous() \
                or scratch.device != pixels.device:
            raise ValueError(f"scratch must be contiguous fp32 [{B}, 3, plane_stride] on the bank's device")
        stride = scratch.shape[2]
    out = torch.empty(B, 3, F, F, dtype=torch.float32, device=pixels.device)
    if B:
        m = (C.c_float * 3)(*mean)
        s = (C.c_float * 3)(*std)
        _lib.check(_lib.load().ssl4gie_det_geometry(ptr(scratch), stride, ptr(pixels), pixels.numel(), ptr(offsets),
                                                    ptr(sizes), n, ptr(index), ptr(geom), ptr(out), B, F, m, s,
                                                    stream()), "det_geometry")
    return out


def det_boxes(boxes, labels, box_offsets, sizes, index, geom, out_start, m_out, max_boxes, F):
    """The boxes of a batch through det_geometry's decisions, in the reference's order of fp32 operations.  boxes fp32
    [m, 4], labels int64 [m], box_offsets int64 [n + 1], sizes int32 [n, 2]: the bank's; out_start int64 [B + 1] on
    the device: sample b's rows are out_start[b] .. out_start[b + 1] of the result; m_out = out_start[-1] and max_boxes
    = the largest per-sample count, both known on the host.  Returns (boxes fp32 [m_out, 4], labels int64 [m_out]);
    a sample with a bad index, or whose count in out_start is not its bank count, gets NaN boxes and labels -1."""
    _dev(boxes, labels, box_offsets, sizes, index, geom, out_start)
    _f32(boxes)
    if boxes.dim() != 2 or boxes.shape[1] != 4 or not boxes.is_contiguous():
        raise ValueError(f"boxes must be contiguous fp32 [m, 4], got {tuple(boxes.shape)}")
    m = boxes.shape[0]
    if labels.dtype != torch.int64 or tuple(labels.shape) != (m,) or not labels.is_contiguous():
        raise ValueError(f"labels must be int64 [{m}]")
    if sizes.dtype != torch.int32 or sizes.dim() != 2 or sizes.shape[1] != 2 or not sizes.is_contiguous():
        raise ValueError("sizes must be int32 [n, 2]")
    n = sizes.shape[0]
    if box_offsets.dtype != torch.int64 or tuple(box_offsets.shape) != (n + 1,) or not box_offsets.is_contiguous():
        raise ValueError(f"box_offsets must be int64 [{n + 1}]")
    if index.dtype != torch.int64 or index.dim() != 1 or not index.is_contiguous():
        raise ValueError("index must be a contiguous int64 vector")
    B = index.shape[0]
    if out_start.dtype != torch.int64 or tuple(out_start.shape) != (B + 1,) or not out_start.is_contiguous():
        raise ValueError(f"out_start must be int64 [{B + 1}]")
    if geom is not None and (geom.dtype != torch.uint8 or tuple(geom.shape) != (B,)):
        raise ValueError(f"geom must be uint8 [{B}]")
    if any(t is not None and t.device != boxes.device for t in (labels, box_offsets, sizes, index, geom, out_start)):
        raise ValueError("det_boxes needs all its tensors on one device")
    F, m_out, max_boxes = int(F), int(m_out), int(max_boxes)
    if F < 4 or F % 4 or m_out < 0 or max_boxes < 0:
        raise ValueError("det_boxes needs F a multiple of 4, m_out >= 0 and max_boxes >= 0")
    out_boxes = torch.empty(m_out, 4, dtype=torch.float32, device=boxes.device)
    out_labels = torch.empty(m_out, dtype=torch.int64, device=boxes.device)
    if B and m_out:
        _lib.check(_lib.load().ssl4gie_det_boxes(ptr(boxes), ptr(labels), ptr(box_offsets), m, ptr(sizes), n, ptr(index),
                                                 ptr(geom), ptr(out_start), ptr(out_boxes), ptr(out_labels), m_out, B, F,
                                                 max_boxes, stream()), "det_boxes")
    return out_boxes, out_labels


# ------------------------------------------------------------------ evaluation metrics (csrc/metric_ops.hip)
def _same_device(*ts):
    ts = [t for t in ts if t is not None]
    if any(t.device != ts[0].device for t in ts):
        raise ValueError("the metric ops need all their tensors on one device")


def seg_counts(logits, target, sigmoid=True):
    """int64 [B, 3] = (|m1|, |m2|, |m1 & m2|) per image, m1 = probs > 0.5 and m2 = target > 0.5: the thresholding the
    reference's DiceScore / IoU / Precision / Recall share.  logits fp32 / bf16 [B, Hin, Win], target fp32 / uint8
    [B, H, W]; where the sizes differ the logits are resampled bilinearly (align_corners=False) inside the kernel."""
    _dev(logits, target)
    _same_device(logits, target)
    if logits.dim() != 3 or target.dim() != 3 or logits.shape[0] != target.shape[0]:
        raise ValueError(f"seg_counts needs logits [B, Hin, Win] and target [B, H, W], got {tuple(logits.shape)}, "
                         f"{tuple(target.shape)}")
    if target.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"target must be uint8 or float32, got {target.dtype}")
    B, Hin, Win = logits.shape
    counts = torch.empty(B, 3, dtype=torch.int64, device=logits.device)
    _lib.check(_lib.load().ssl4gie_seg_counts(ptr(logits), code(logits.dtype), ptr(target),
                                              _lib.TGT_U8 if target.dtype == torch.uint8 else _lib.TGT_F32, ptr(counts),
                                              B, Hin, Win, target.shape[1], target.shape[2], int(bool(sigmoid)),
                                              stream()), "seg_counts")
    return counts


def seg_scores(counts, smooth, accum=None):
    """fp32 [4] = batch means of Dice, IoU, precision, recall from seg_counts' output; accum (fp64 [5]) += the four
    per-image sums and the image count, in the same launch."""
    _dev(counts, accum)
    _same_device(counts, accum)
    if counts.dtype != torch.int64 or counts.dim() != 2 or counts.shape[1] != 3 or counts.shape[0] < 1:
        raise ValueError("counts must be int64 [B, 3], B >= 1")
    if accum is not None and (accum.dtype != torch.float64 or accum.numel() != 5):
        raise ValueError("accum must be float64 [5]")
    scores = torch.empty(4, dtype=torch.float32, device=counts.device)
    _lib.check(_lib.load().ssl4gie_seg_scores(ptr(counts), counts.shape[0], float(smooth), ptr(scores), ptr(accum),
                                              stream()), "seg_scores")
    return scores


def confusion_update(conf, x, target):
    """conf (int64 [C * C + 1]: the C x C matrix, row = target, column = prediction, then the rejected counter) += the
    counts of one batch.  x: logits fp32 / bf16 [B, C] (first maximum) or predictions int64 [B]; target int64 [B]."""
    _dev(conf, x, target)
    _same_device(conf, x, target)
    if conf.dtype != torch.int64 or conf.dim() != 1:
        raise ValueError("conf must be int64 [C * C + 1]")
    Cn = int(round((conf.numel() - 1) ** 0.5))
    if Cn < 1 or Cn * Cn + 1 != conf.numel():
        raise ValueError("conf must be int64 [C * C + 1]")
    if target.dtype != torch.int64 or target.dim() != 1:
        raise ValueError("target must be int64 [B]")
    B = target.shape[0]
    if x.dtype == torch.int64:
        if tuple(x.shape) != (B,):
            raise ValueError(f"predictions must be int64 [{B}]")
        kind = _lib.PRED_I64
    else:
        if tuple(x.shape) != (B, Cn):
            raise ValueError(f"logits must be [{B}, {Cn}], got {tuple(x.shape)}")
        kind = code(x.dtype)
    if B:
        _lib.check(_lib.load().ssl4gie_confusion_update(ptr(x), kind, ptr(target), ptr(conf), conf.data_ptr() + 8 * Cn * Cn,
                                                        B, Cn, stream()), "confusion_update")
    return conf


def confusion_scores(conf, smooth):
    """fp32 [4] = mean F1, mean precision, mean recall, accuracy from confusion_update's matrix"""
    _dev(conf)
    Cn = int(round((conf.numel() - 1) ** 0.5))
    if conf.dtype != torch.int64 or conf.dim() != 1 or Cn < 1 or Cn * Cn + 1 != conf.numel():
        raise ValueError("conf must be int64 [C * C + 1]")
    scores = torch.empty(4, dtype=torch.float32, device=conf.device)
    _lib.check(_lib.load().ssl4gie_confusion_scores(ptr(conf), Cn, float(smooth), ptr(scores), stream()),
               "confusion_scores")
    return scores


def topk_workspace(B, device):
    return torch.empty(max(1, _lib.load().ssl4gie_topk_workspace_bytes(int(B))), dtype=torch.uint8, device=device)


def topk_update(acc, loss_sum, logits, target, topk, rank=None, row_loss=None, workspace=None):
    """acc (int64 [len(topk) + 2]: hits per k, rows counted, rows rejected) and loss_sum (fp64 [1]: summed cross-entropy)
    += one batch.  logits fp32 / bf16 [B, C], unit stride along C, any row stride >= C; target int64 [B]; topk strictly
    ascending, each in [1, C].  rank (int32 [B]) / row_loss (fp32 [B]) are overwritten when given.  The rank of a row is
    the number of columns ordered above the target's logit, equal values by lower index first, a NaN above every number."""
    _dev(acc, loss_sum, target, rank, row_loss)
    _same_device(acc, loss_sum, logits, target, rank, row_loss)
    if not logits.is_cuda:
        raise RuntimeError("ssl4gie_amd ops need tensors on the HIP device (no CPU fallback)")
    if logits.dim() != 2 or target.dim() != 1 or target.dtype != torch.int64 or logits.shape[0] != target.shape[0]:
        raise ValueError(f"topk_update needs logits [B, C] and int64 target [B], got {tuple(logits.shape)}, "
                         f"{tuple(target.shape)} {target.dtype}")
    B, Cn = logits.shape
    ks = [int(k) for k in topk]
    if not 1 <= len(ks) <= 8 or any(b <= a for a, b in zip(ks, ks[1:])):
        raise ValueError(f"topk must hold 1 to 8 strictly ascending values, got {tuple(topk)}")
    if ks[0] < 1 or ks[-1] > Cn:
        raise ValueError(f"topk={tuple(topk)} needs every k in [1, C = {Cn}]")
    if acc.dtype != torch.int64 or acc.numel() != len(ks) + 2 or loss_sum.dtype != torch.float64 or loss_sum.numel() != 1:
        raise ValueError("acc must be int64 [len(topk) + 2] and loss_sum fp64 [1]")
    if (rank is not None and (rank.dtype != torch.int32 or rank.numel() != B)) or \
            (row_loss is not None and (row_loss.dtype != torch.float32 or row_loss.numel() != B)):
        raise ValueError(f"rank must be int32 [{B}] and row_loss fp32 [{B}]")
    if B == 0:
        return acc
    if logits.stride(1) != 1 or (B > 1 and logits.stride(0) < Cn):
        logits = logits.contiguous()
    ld = logits.stride(0) if B > 1 else Cn
    L = _lib.load()
    nbytes = L.ssl4gie_topk_workspace_bytes(B)
    if workspace is None or workspace.numel() < nbytes or workspace.device != logits.device:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=logits.device)
    _lib.check(L.ssl4gie_topk_update(ptr(logits), code(logits.dtype), ld, ptr(target), (C.c_int * len(ks))(*ks), len(ks),
                                     ptr(acc), ptr(loss_sum), ptr(rank), ptr(row_loss), B, Cn, ptr(workspace), stream()),
               "topk_update")
    return acc


def lower_median(x):
    """0-dim fp32: the element of rank (n - 1) // 2 of the non-negative fp32 values x (torch.median's lower median),
    by an exact radix select; NaN for an empty x.  x is not modified."""
    _dev(x)
    _f32(x)
    L = _lib.load()
    out = torch.empty((), dtype=torch.float32, device=x.device)
    ws = torch.empty(L.ssl4gie_lower_median_workspace_bytes(), dtype=torch.uint8, device=x.device)
    _lib.check(L.ssl4gie_lower_median_f32(ptr(x), x.numel(), ptr(out), ptr(ws), stream()), "lower_median_f32")
    return out


def depth_eval(pred, target, target_og, scale_):
    """fp32 [B, 3] = (rmse, rel_err, abs_err) per image of the depth evaluation (eval_depth.py:43-61): pred, target
    fp32 [B, S, S], target_og fp32 [B, H, W].  An image without a valid pixel gives three NaNs."""
    _dev(pred, target, target_og)
    _f32(pred, target, target_og)
    _same_device(pred, target, target_og)
    if pred.dim() != 3 or pred.shape[1] != pred.shape[2] or pred.shape != target.shape:
        raise ValueError(f"depth_eval needs pred and target [B, S, S], got {tuple(pred.shape)}, {tuple(target.shape)}")
    if target_og.dim() != 3 or target_og.shape[0] != pred.shape[0]:
        raise ValueError(f"target_og must be [B, H, W], got {tuple(target_og.shape)}")
    B, S, _ = pred.shape
    H, W = target_og.shape[1:]
    L = _lib.load()
    nb = L.ssl4gie_depth_eval_workspace_bytes(B, S, H, W)
    if nb == 0:
        raise ValueError(f"depth_eval: invalid shape B={B} S={S} H={H} W={W}")
    ws = torch.empty(nb, dtype=torch.uint8, device=pred.device)
    out = torch.empty(B, 3, dtype=torch.float32, device=pred.device)
    _lib.check(L.ssl4gie_depth_eval(ptr(pred), ptr(target), ptr(target_og), ptr(out), B, S, S, H, W, float(scale_),
                                    ptr(ws), stream()), "depth_eval")
    return out


# ------------------------------------------------------------------ detection metric (csrc/det_map_ops.hip)
DET_MAP_IOU_THRESHOLDS = torch.linspace(0.5, 0.95, 10).tolist()   # fp32 values widened: as torchmetrics builds them
DET_MAP_REC_THRESHOLDS = torch.linspace(0.0, 1.0, 101).tolist()
DET_MAP_NAMES = ("map", "map_50", "map_75", "map_small", "map_medium", "map_large", "mar_1", "mar_10", "mar_100",
                 "mar_small", "mar_medium", "mar_large")


def _det_map_side(boxes, labels, off, n_img, what):
    if boxes.dtype != torch.float32 or boxes.dim() != 2 or boxes.shape[1] != 4:
        raise ValueError(f"{what} boxes must be float32 [n, 4], got {boxes.dtype} {tuple(boxes.shape)}")
    if labels.dtype != torch.int64 or tuple(labels.shape) != (boxes.shape[0],):
        raise ValueError(f"{what} labels must be int64 [{boxes.shape[0]}]")
    if off.dtype != torch.int32 or tuple(off.shape) != (n_img + 1,):
        raise ValueError(f"{what} offsets must be int32 [{n_img + 1}]")


def det_map_match(det_boxes, det_scores, det_labels, det_off, gt_boxes, gt_labels, gt_off):
    """COCOeval.evaluateImg for every image, class, area range and IoU threshold in one launch.  The detections of all
    images end to end (boxes fp32 [N, 4] xyxy, scores fp32 [N], labels int64 [N]), image i owning [det_off[i],
    det_off[i + 1]) (int32 [n_img + 1] on the device); ground truths likewise.  Returns rank int32 [N], matched and
    ignored int64 [N] (bit = area * 10 + threshold), npig int32 [256, 4], present int32 [256], flag int32 [1]."""
    ts = (det_boxes, det_scores, det_labels, det_off, gt_boxes, gt_labels, gt_off)
    _dev(*ts)
    _same_device(*ts)
    n_img = det_off.numel() - 1
    if n_img < 1:
        raise ValueError("det_map_match needs at least one image")
    _det_map_side(det_boxes, det_labels, det_off, n_img, "detection")
    _det_map_side(gt_boxes, gt_labels, gt_off, n_img, "ground-truth")
    N, G = det_boxes.shape[0], gt_boxes.shape[0]
    if det_scores.dtype != torch.float32 or tuple(det_scores.shape) != (N,):
        raise ValueError(f"scores must be float32 [{N}]")
    dev = det_off.device
    rank = torch.zeros(N, dtype=torch.int32, device=dev)
    matched = torch.zeros(N, dtype=torch.int64, device=dev)
    ignored = torch.zeros(N, dtype=torch.int64, device=dev)
    npig = torch.empty(_lib.DET_MAP_CLASSES, 4, dtype=torch.int32, device=dev)
    present = torch.empty(_lib.DET_MAP_CLASSES, dtype=torch.int32, device=dev)
    flag = torch.empty(1, dtype=torch.int32, device=dev)
    thr = (C.c_double * 10)(*DET_MAP_IOU_THRESHOLDS)
    _lib.check(_lib.load().ssl4gie_det_map_match(ptr(det_boxes) if N else 0, ptr(det_scores) if N else 0,
                                                 ptr(det_labels) if N else 0, ptr(det_off), ptr(gt_boxes) if G else 0,
                                                 ptr(gt_labels) if G else 0, ptr(gt_off), n_img, N, G, thr, ptr(rank),
                                                 ptr(matched), ptr(ignored), ptr(npig), ptr(present), ptr(flag),
                                                 stream()), "det_map_match")
    return rank, matched, ignored, npig, present, flag


def det_map_order(det_scores, det_labels, rank):
    """The kept detections (rank < 100, label in [0, 255]) stably sorted by (label ascending, score descending), ties
    in insertion order: sorted_idx int32 [N] (the first seg_off[256] entries count) and seg_off int32 [257]."""
    _dev(det_scores, det_labels, rank)
    _same_device(det_scores, det_labels, rank)
    N = det_scores.numel()
    if det_scores.dtype != torch.float32 or det_labels.dtype != torch.int64 or rank.dtype != torch.int32 or \
            det_scores.dim() != 1 or tuple(det_labels.shape) != (N,) or tuple(rank.shape) != (N,):
        raise ValueError("det_map_order needs scores float32 [N], labels int64 [N], rank int32 [N]")
    L = _lib.load()
    nb = L.ssl4gie_det_map_workspace_bytes(1, N, 1)   # the size depends on the number of detections alone
    if nb == 0:
        raise ValueError(f"det_map_order: invalid number of detections {N}")
    ws = torch.empty(nb, dtype=torch.uint8, device=det_scores.device)
    sorted_idx = torch.zeros(N, dtype=torch.int32, device=det_scores.device)
    seg_off = torch.empty(_lib.DET_MAP_CLASSES + 1, dtype=torch.int32, device=det_scores.device)
    _lib.check(L.ssl4gie_det_map_order(ptr(det_scores), ptr(det_labels), ptr(rank), N, ptr(sorted_idx), ptr(seg_off),
                                       ptr(ws), stream()), "det_map_order")
    return sorted_idx, seg_off


def det_map_accumulate(sorted_idx, seg_off, rank, matched, ignored, npig, present, flag):
    """COCOeval.accumulate and .summarize: stats fp64 [256, 6, 10, 2] (101-point precision sum, final recall; pairs
    (all, 100), (small, 100), (medium, 100), (large, 100), (all, 1), (all, 10)), out64 fp64 [12] and out32 fp32 [12]
    in DET_MAP_NAMES' order, outi int32 [258] = number of classes, flag word, classes ascending."""
    ts = (sorted_idx, seg_off, rank, matched, ignored, npig, present, flag)
    _dev(*ts)
    _same_device(*ts)
    N = rank.numel()
    if sorted_idx.dtype != torch.int32 or rank.dtype != torch.int32 or matched.dtype != torch.int64 or \
            ignored.dtype != torch.int64 or sorted_idx.numel() != N or matched.numel() != N or ignored.numel() != N:
        raise ValueError("det_map_accumulate needs sorted_idx, rank int32 [N] and matched, ignored int64 [N]")
    if any(t.dtype != torch.int32 for t in (seg_off, npig, present, flag)) or seg_off.numel() != 257 or \
            npig.numel() != 1024 or present.numel() != 256 or flag.numel() != 1:
        raise ValueError("det_map_accumulate needs seg_off int32 [257], npig int32 [256, 4], present int32 [256], "
                         "flag int32 [1]")
    dev = rank.device
    stats = torch.zeros(_lib.DET_MAP_CLASSES, 6, 10, 2, dtype=torch.float64, device=dev)
    out64 = torch.empty(12, dtype=torch.float64, device=dev)
    out32 = torch.empty(12, dtype=torch.float32, device=dev)
    outi = torch.empty(2 + _lib.DET_MAP_CLASSES, dtype=torch.int32, device=dev)
    rec = (C.c_double * 101)(*DET_MAP_REC_THRESHOLDS)
    _lib.check(_lib.load().ssl4gie_det_map_accumulate(ptr(sorted_idx) if N else 0, ptr(seg_off), ptr(rank) if N else 0,
                                                      ptr(matched) if N else 0, ptr(ignored) if N else 0, ptr(npig),
                                                      ptr(present), ptr(flag), N, rec, ptr(stats), ptr(out64),
                                                      ptr(out32), ptr(outi), stream()), "det_map_accumulate")
    return stats, out64, out32, outi


# ------------------------------------------------------------------ Faster R-CNN heads (csrc/det_head_ops.hip)
def nms_segments(boxes, seg_off, thr, valid=None, max_seg=None):
    """Greedy NMS inside every segment without a host round trip.  boxes fp32 [n, 4] xyxy sorted by descending score
    within each segment, seg_off int32 [S + 1] on the device, valid uint8 [n] or None.  max_seg: an upper bound of the
    segment sizes known on the host (at most 4096); None reads the offsets back once to find it.  Returns keep_rank
    int32 [n] (position among the kept boxes of the segment, -1 for a dropped box) and count int32 [S]."""
    if max_seg is None:
        so = seg_off.detach().cpu()
        max_seg = int((so[1:] - so[:-1]).max()) if so.numel() > 1 else 0
    if max_seg > _lib.NMS_MAX_PER_SEGMENT:
        raise ValueError(f"nms_segments: {max_seg} boxes in a segment, the cap is {_lib.NMS_MAX_PER_SEGMENT}")
    _dev(boxes, seg_off, valid)
    _f32(boxes)
    _same_device(boxes, seg_off, valid)
    n, S = boxes.shape[0], seg_off.numel() - 1
    if boxes.dim() != 2 or boxes.shape[1] != 4 or seg_off.dtype != torch.int32 or seg_off.dim() != 1 or S < 1:
        raise ValueError("nms_segments needs boxes float32 [n, 4] and seg_off int32 [S + 1], S >= 1")
    if valid is not None and (valid.dtype != torch.uint8 or tuple(valid.shape) != (n,)):
        raise ValueError(f"valid must be uint8 [{n}]")
    keep_rank = torch.empty(n, dtype=torch.int32, device=boxes.device)
    count = torch.zeros(S, dtype=torch.int32, device=boxes.device)
    if n == 0 or max_seg <= 0:
        return keep_rank.fill_(-1), count
    L = _lib.load()
    nb = L.ssl4gie_nms_workspace_bytes(n, int(max_seg))
    if nb == 0:
        raise ValueError(f"nms_segments: invalid number of boxes {n}")
    ws = torch.empty(nb, dtype=torch.uint8, device=boxes.device)
    _lib.check(L.ssl4gie_nms_segments(ptr(boxes), ptr(valid), ptr(seg_off), S, n, int(max_seg), float(thr),
                                      ptr(keep_rank), ptr(count), ptr(ws), stream()), "nms_segments")
    return keep_rank, count


def rpn_decode(heads, grids, k_off, base_anchors, topk_idx, F, min_size, score_thresh):
    """The top-k candidates of every (image, level) decoded, clipped and flagged in one launch.  heads: the fp32 head
    outputs [B * g * g, ld] of the levels (columns [0, A) logits, then A x 4 deltas), grids their sides, k_off the
    candidate ranges of the levels (Python ints, k_off[0] == 0), base_anchors fp32 [L, A, 4] (host), topk_idx int64
    [B, k_off[-1]].  Returns boxes fp32 [B, Ktot, 4], scores fp32 [B, Ktot], valid uint8 [B, Ktot]."""
    _dev(topk_idx, *heads)
    _f32(*heads)
    _same_device(topk_idx, *heads)
    Ln = len(heads)
    base = torch.as_tensor(base_anchors, dtype=torch.float32).cpu().contiguous()
    A = base.shape[1]
    ld = heads[0].shape[1]
    B, ktot = topk_idx.shape
    if topk_idx.dtype != torch.int64 or len(grids) != Ln or len(k_off) != Ln + 1 or tuple(base.shape) != (Ln, A, 4) or \
            ktot != k_off[-1]:
        raise ValueError("rpn_decode: inconsistent level description")
    for h, g in zip(heads, grids):
        if h.dim() != 2 or tuple(h.shape) != (B * g * g, ld):
            raise ValueError(f"rpn_decode: a head output must be [{B * g * g}, {ld}], got {tuple(h.shape)}")
    dev = topk_idx.device
    boxes = torch.empty(B, ktot, 4, dtype=torch.float32, device=dev)
    scores = torch.empty(B, ktot, dtype=torch.float32, device=dev)
    valid = torch.empty(B, ktot, dtype=torch.uint8, device=dev)
    if B * ktot:
        hp = (_lib.vp * Ln)(*[h.data_ptr() for h in heads])
        gp = (_lib.i32 * Ln)(*[int(g) for g in grids])
        kp = (_lib.i32 * (Ln + 1))(*[int(k) for k in k_off])
        bp = (_lib.f32 * (Ln * A * 4))(*base.view(-1).tolist())
        _lib.check(_lib.load().ssl4gie_rpn_decode(hp, gp, kp, bp, Ln, A, ld, ptr(topk_idx), B, int(F), float(min_size),
                                                  float(score_thresh), ptr(boxes), ptr(scores), ptr(valid), stream()),
                   "rpn_decode")
    return boxes, scores, valid


def roi_decode(proposals, logits, deltas, weights, W, H, min_size, score_thresh):
    """Per-class boxes of the detection stage: proposals fp32 [K, 4], logits fp32 [K, C] and deltas fp32 [K, 4 C] (row
    views of one product are fine: unit stride inside a row).  Returns boxes fp32 [K, C - 1, 4], scores fp32 [K, C - 1]
    (row softmax without the background column) and valid uint8 [K, C - 1]."""
    for t in (proposals, logits, deltas):
        if not t.is_cuda:
            raise RuntimeError("ssl4gie_amd ops need tensors on the HIP device (no CPU fallback)")
    _f32(proposals, logits, deltas)
    _same_device(proposals, logits, deltas)
    K, Cn = logits.shape
    if not proposals.is_contiguous() or tuple(proposals.shape) != (K, 4) or tuple(deltas.shape) != (K, 4 * Cn) or \
            Cn < 2 or logits.stride(1) != 1 or deltas.stride(1) != 1:
        raise ValueError("roi_decode needs proposals [K, 4], logits [K, C], deltas [K, 4 C] with unit-stride rows")
    dev = logits.device
    boxes = torch.empty(K, Cn - 1, 4, dtype=torch.float32, device=dev)
    scores = torch.empty(K, Cn - 1, dtype=torch.float32, device=dev)
    valid = torch.empty(K, Cn - 1, dtype=torch.uint8, device=dev)
    if K:
        wx, wy, ww, wh = (float(w) for w in weights)
        _lib.check(_lib.load().ssl4gie_roi_decode(ptr(proposals), ptr(logits), logits.stride(0), ptr(deltas),
                                                  deltas.stride(0), K, Cn, wx, wy, ww, wh, float(W), float(H),
                                                  float(min_size), float(score_thresh), ptr(boxes), ptr(scores),
                                                  ptr(valid), stream()), "roi_decode")
    return boxes, scores, valid


def _roi_maps(maps, what):
    """the four NCHW views of channels-last fp32 storage as (pointers, (H, W) pairs, B, C)"""
    if len(maps) != 4:
        raise ValueError(f"{what} needs the four pyramid maps")
    B, Cn = maps[0].shape[:2]
    for m in maps:
        if not m.is_cuda:
            raise RuntimeError("ssl4gie_amd ops need tensors on the HIP device (no CPU fallback)")
        if m.dtype != torch.float32 or m.dim() != 4 or m.shape[0] != B or m.shape[1] != Cn:
            raise ValueError(f"{what}: a map must be float32 [B, C, H, W]")
        if not m.permute(0, 2, 3, 1).is_contiguous():
            raise RuntimeError(f"{what} needs channels-last maps (NCHW views of NHWC storage)")
    if Cn % 64 or (Cn > 256 and Cn % 256):
        raise ValueError(f"{what}: C = {Cn} must be a multiple of 64 (of 256 above 256)")
    hp = (_lib.vp * 4)(*[m.data_ptr() for m in maps])
    hw = (_lib.i32 * 8)(*[int(s) for m in maps for s in m.shape[2:]])
    return hp, hw, B, Cn


def roi_align_fwd(maps, scales, rois, roi_batch, out_dtype, want_levels=False):
    """MultiScaleRoIAlign(7, 2) over the four maps: [K, C * 49] in (c, ph, pw) order in out_dtype (and the level of every
    RoI, int32 [K], when asked).  rois fp32 [K, 4], roi_batch int32 [K]."""
    hp, hw, B, Cn = _roi_maps(maps, "roi_align_fwd")
    _dev(rois, roi_batch)
    _f32(rois)
    K = rois.shape[0]
    if tuple(rois.shape) != (K, 4) or roi_batch.dtype != torch.int32 or tuple(roi_batch.shape) != (K,):
        raise ValueError("roi_align_fwd needs rois float32 [K, 4] and roi_batch int32 [K]")
    out = torch.empty(K, Cn * 49, dtype=out_dtype, device=rois.device)
    levels = torch.empty(K, dtype=torch.int32, device=rois.device) if want_levels else None
    if K:
        sc = (_lib.f32 * 4)(*[float(s) for s in scales])
        _lib.check(_lib.load().ssl4gie_roi_align_fwd(hp, hw, sc, B, Cn, ptr(rois), ptr(roi_batch), K, ptr(out),
                                                     code(out_dtype), ptr(levels), stream()), "roi_align_fwd")
    return (out, levels) if want_levels else out


def roi_align_bwd(dmaps, scales, rois, roi_batch, dy):
    """dmaps (zeroed fp32 channels-last maps) += the gradient of roi_align_fwd's output (float atomics: the sums are not
    bitwise reproducible)"""
    hp, hw, B, Cn = _roi_maps(dmaps, "roi_align_bwd")
    _dev(rois, roi_batch, dy)
    _f32(rois)
    K = rois.shape[0]
    if tuple(rois.shape) != (K, 4) or roi_batch.dtype != torch.int32 or tuple(roi_batch.shape) != (K,) or \
            tuple(dy.shape) != (K, Cn * 49):
        raise ValueError("roi_align_bwd needs rois float32 [K, 4], roi_batch int32 [K] and dy [K, C * 49]")
    if K:
        sc = (_lib.f32 * 4)(*[float(s) for s in scales])
        _lib.check(_lib.load().ssl4gie_roi_align_bwd(hp, hw, sc, B, Cn, ptr(rois), ptr(roi_batch), K, ptr(dy),
                                                     code(dy.dtype), stream()), "roi_align_bwd")
    return dmaps


# ------------------------------------------------------------------ Mixup / CutMix (fine-tuning recipe)
def mixup(x, lam, box, use_cutmix):
    """timm.data.Mixup's image step IN PLACE on x fp32 [B, C, H, W]: sample i against sample B - 1 - i by the
    per-sample tables lam fp32 [B], box int32 [B, 4] = (y0, y1, x0, x1), use_cutmix uint8 [B] (data.mixup_tables)"""
    _dev(x, lam, box, use_cutmix)
    _f32(x, lam)
    B, Cn, H, W = x.shape
    if lam.shape != (B,) or tuple(box.shape) != (B, 4) or box.dtype != torch.int32 or use_cutmix.shape != (B,) \
            or use_cutmix.dtype != torch.uint8:
        raise ValueError("mixup needs lam fp32 [B], box int32 [B, 4], use_cutmix uint8 [B]")
    _lib.check(_lib.load().ssl4gie_mixup(ptr(x), ptr(lam), ptr(box), ptr(use_cutmix), B, Cn, H, W, stream()), "mixup")
    return x


def mixup_target(target, lam, num_classes, smoothing=0.0):
    """timm's mixup_target: int64 labels [B] + lam fp32 [B] -> fp32 soft targets [B, num_classes]"""
    _dev(target, lam)
    _f32(lam)
    if target.dtype != torch.int64 or target.dim() != 1 or lam.shape != target.shape:
        raise ValueError("mixup_target needs int64 labels [B] and lam fp32 [B]")
    B = target.shape[0]
    off = smoothing / num_classes
    on = 1.0 - smoothing + off
    out = torch.empty(B, num_classes, dtype=torch.float32, device=target.device)
    _lib.check(_lib.load().ssl4gie_mixup_target(ptr(target), ptr(lam), ptr(out), B, num_classes, on, off, stream()),
               "mixup_target")
    return out
