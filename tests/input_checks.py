"""fp64 numpy restatement of the resampling rule of ssl4gie_view_sample_u8 (include/ssl4gie_hip.h), and the fixed
cases the CPU and GPU tests share.  Not a test module: tests/test_input_checks_cpu.py pins it against torch's CPU
F.interpolate(antialias=True); tests/test_gpu_input_pipeline.py holds the kernel to it.

Rule, per axis (box length L -> S outputs): scale = L / S, fs = max(scale, 1), support = R fs (R = 2 bicubic,
1 bilinear); output o: c = (o + 0.5) scale, taps k in [max(0, int(c - support + 0.5)), min(L, int(c + support +
0.5))), weight f((k - c + 0.5) / fs) / sum.  Crop first, two separable passes, flip, clamp to [0, 255],
(v / 255 - mean) / std."""
import functools

import numpy as np

H_IMG, W_IMG = 96, 81   # 243-byte rows: no 4-byte alignment
BOXES = ((0, 0, 96, 80), (5, 7, 17, 23), (10, 3, 64, 64), (0, 0, 7, 9), (31, 11, 65, 40), (3, 2, 90, 75),
         (40, 40, 1, 1), (0, 0, 32, 32))   # (top, left, height, width)
SIZES = (32, 24)
FILTERS = ("bicubic", "bilinear")


def noise_image(seed=0, h=H_IMG, w=W_IMG):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def _filter(x, name):
    x = np.abs(x)
    if name == "bicubic":
        a = -0.5
        return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0,
                        np.where(x < 2.0, a * (((x - 5.0) * x + 8.0) * x - 4.0), 0.0))
    assert name == "bilinear", name
    return np.where(x < 1.0, 1.0 - x, 0.0)


@functools.lru_cache(maxsize=None)
def axis_weights(L, S, name):
    """[S, L] float64: row o holds the normalised weights of output o over the L source positions"""
    R = 2.0 if name == "bicubic" else 1.0
    scale = L / S
    fs = max(scale, 1.0)
    support = R * fs
    W = np.zeros((S, L), dtype=np.float64)
    for o in range(S):
        c = (o + 0.5) * scale
        lo = max(0, int(c - support + 0.5))
        hi = min(L, int(c + support + 0.5))
        k = np.arange(lo, hi, dtype=np.float64)
        w = _filter((k - c + 0.5) / fs, name)
        W[o, lo:hi] = w / w.sum()
    W.setflags(write=False)
    return W


def tap_counts(L, S, name):
    return (axis_weights(L, S, name) != 0).sum(axis=1)


def resample(img_u8, box, S, name, flip=False):
    """[3, S, S] float64 in 0..255 units: crop, two passes, flip — before the clamp"""
    top, left, h, w = box
    crop = img_u8[top:top + h, left:left + w, :].astype(np.float64)
    out = np.einsum("oy,yxc->oxc", axis_weights(h, S, name), crop)
    out = np.einsum("px,oxc->cop", axis_weights(w, S, name), out)
    return out[:, :, ::-1] if flip else out


def view_ref(img_u8, box, S, name, flip=False, mean=(0.0, 0.0, 0.0), std=(1.0 / 255.0,) * 3):
    """what ssl4gie_view_sample_u8 computes for one sample, in float64; the defaults give 0..255 units"""
    v = np.clip(resample(img_u8, box, S, name, flip), 0.0, 255.0)
    m = np.asarray(mean, dtype=np.float64).reshape(3, 1, 1)
    s = np.asarray(std, dtype=np.float64).reshape(3, 1, 1)
    return (v / 255.0 - m) / s


def torch_cpu_view(img_u8, box, S, name, flip=False):
    """torch's own CPU path in fp32: F.interpolate(crop.float(), (S, S), mode, antialias=True).clamp(0, 255)"""
    import torch
    import torch.nn.functional as F
    top, left, h, w = box
    crop = torch.from_numpy(np.ascontiguousarray(img_u8[top:top + h, left:left + w, :])).permute(2, 0, 1)[None].float()
    out = F.interpolate(crop, size=(S, S), mode=name, antialias=True, align_corners=False).clamp(0, 255)[0]
    return (out.flip(-1) if flip else out).numpy()


def cases():
    return [(box, S, name, flip) for name in FILTERS for S in SIZES for box in BOXES for flip in (False, True)]


@functools.lru_cache(maxsize=None)
def torch_cpu_error():
    """{filter: max |torch CPU fp32 - restatement| over the fixed cases, 0..255 units} (computed once)"""
    img = noise_image(0)
    err = {name: 0.0 for name in FILTERS}
    for box, S, name, flip in cases():
        d = np.abs(torch_cpu_view(img, box, S, name, flip).astype(np.float64) - view_ref(img, box, S, name, flip))
        err[name] = max(err[name], float(d.max()))
    return err
