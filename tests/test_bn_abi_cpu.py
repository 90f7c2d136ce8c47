"""CPU: the argument validation of the five BatchNorm entry points (ABI 12).

Every (source or mask kind, dtype, relu, set of pointers present) combination over a tiny shape is classified by the
table below, which restates the REQUIRE lines of the sixteen entry points of ABI 11 that the five replaced — it is
written out here, not derived from the library.  A combination none of the sixteen could express, or that its
function rejected, must come back as SSL4GIE_EARG; validation runs before anything touches the device, so these
calls need no GPU.  Combinations the table accepts are NOT called (they would launch).  Two deliberate
differences from ABI 11, both on pointers the old functions accepted and ignored: the running statistics under
ssl4gie_bn_fwd(training = 0) and the ReLU output under relu = 0 — ABI 12 has no ignored pointers, so they are
outside the table."""
import itertools

import numpy as np

from ssl4gie_amd import _lib
from ssl4gie_amd._lib import BF16, F32

EARG = 1000
ROWS, C = 4, 8
X, PARTIALS, STATS, COEF = range(4)          # SSL4GIE_BN_FROM_*
NONE, Y, XM, BITS = range(4)                 # SSL4GIE_BN_MASK_*
ANY = (F32, BF16)


def form(sel, need, may="", dtypes=ANY, relu=(0, 1)):
    return dict(sel=sel, need=set(need.split()), may=set(may.split()), dtypes=dtypes, relu=relu)


# argument order of the C prototypes; names in PTRS[f] are pointers, the rest scalars
ARGS = {
    "ssl4gie_bn_fwd": "source x partial parts gamma beta res y relu_bits coef mean rstd running_mean running_var "
                      "momentum eps relu workspace dtype rows C stream",
    "ssl4gie_bn_stats": "x partial parts mean var workspace dtype rows C stream",
    "ssl4gie_bn_bwd": "dy mask_kind mask x gamma beta mean rstd dx dres dgamma dbeta accumulate workspace dtype rows C "
                      "stream",
    "ssl4gie_bn_bwd_reduce": "dy mask_kind mask x gamma beta mean rstd dres sums workspace dtype rows C stream",
    "ssl4gie_bn_bwd_apply": "dy mask_kind mask x gamma beta mean rstd sums inv_count dx workspace dtype rows C stream",
}
SCALARS = {"source", "mask_kind", "parts", "momentum", "eps", "relu", "dtype", "rows", "C", "stream", "accumulate",
           "inv_count"}
PTRS = {f: [a for a in s.split() if a not in SCALARS] for f, s in ARGS.items()}
SELECTOR = {"ssl4gie_bn_fwd": "source", "ssl4gie_bn_stats": None, "ssl4gie_bn_bwd": "mask_kind",
            "ssl4gie_bn_bwd_reduce": "mask_kind", "ssl4gie_bn_bwd_apply": "mask_kind"}

_OPT = "gamma beta res running_mean running_var"
_BWD = "dy x mean rstd workspace"
# the sixteen entry points of ABI 11 as (selector, required pointers, optional pointers, dtypes, relu)
FORMS = {
    "ssl4gie_bn_fwd": {
        "bn_fwd(training=1)": form(X, "x y mean rstd workspace", _OPT),
        "bn_fwd(training=0)": form(STATS, "x y mean rstd workspace", "gamma beta res"),
        "bn_fwd_partials": form(PARTIALS, "x partial y mean rstd workspace", _OPT),
        "bn_fwd_partials_bits": form(PARTIALS, "x partial y relu_bits mean rstd workspace", _OPT, (BF16,), (1,)),
        "bn_coef_partials": form(PARTIALS, "partial mean rstd coef workspace", "gamma beta running_mean running_var"),
        "bn_coef_stats": form(STATS, "mean rstd coef", "gamma beta"),
        "bn_apply_bits": form(COEF, "x coef y relu_bits", "res", (BF16,), (1,)),
    },
    "ssl4gie_bn_stats": {
        "bn_stats": form(None, "x mean var workspace"),
        "bn_stats_partials": form(None, "partial mean var workspace"),
    },
    "ssl4gie_bn_bwd": {
        "bn_bwd(relu=0)": form(NONE, _BWD + " dx", "gamma dres dgamma dbeta"),
        "bn_bwd(relu=1)": form(Y, _BWD + " dx mask", "gamma dres dgamma dbeta"),
        "bn_bwd_xmask": form(XM, _BWD + " dx", "gamma beta dgamma dbeta"),
        "bn_bwd_bits": form(BITS, _BWD + " dx mask dres", "gamma dgamma dbeta", (BF16,)),
    },
    "ssl4gie_bn_bwd_reduce": {
        "bn_bwd_reduce(relu=0)": form(NONE, _BWD + " sums", "dres"),
        "bn_bwd_reduce(relu=1)": form(Y, _BWD + " sums mask", "dres"),
        "bn_bwd_reduce_xmask": form(XM, _BWD + " sums", "gamma beta"),
        "bn_bwd_reduce_bits": form(BITS, _BWD + " sums mask dres", "", (BF16,)),
    },
    "ssl4gie_bn_bwd_apply": {
        "bn_bwd_apply(relu=0)": form(NONE, _BWD + " sums dx", "gamma"),
        "bn_bwd_apply(relu=1)": form(Y, _BWD + " sums dx mask", "gamma"),
        "bn_bwd_apply_xmask": form(XM, _BWD + " sums dx", "gamma beta"),
    },
}
# scalars the old function did not take (so any value is "expressible") or did not check
NO_DTYPE = {"bn_coef_partials", "bn_coef_stats", "bn_stats_partials"}
ONLY_C_POSITIVE = {"bn_coef_stats"}


def _accepts(f, sel, dtype, relu, present):
    return any(fm["sel"] == sel and fm["need"] <= present <= fm["need"] | fm["may"]
               and (dtype in fm["dtypes"] or name in NO_DTYPE) and relu in fm["relu"]
               for name, fm in FORMS[f].items())


class _Caller:
    def __init__(self):
        self.lib = _lib.load()
        nbytes = max(self.lib.ssl4gie_bn_workspace_bytes(ROWS, C), 4 * ROWS * C)
        self.bufs = {}
        for f in ARGS:
            for p in PTRS[f]:
                self.bufs.setdefault(p, np.zeros(nbytes, dtype=np.uint8))   # a real host buffer per pointer
        self.defaults = dict(parts=2, momentum=0.1, eps=1e-5, relu=0, dtype=F32, rows=ROWS, C=C, stream=None,
                             accumulate=0, inv_count=0.25, source=X, mask_kind=NONE)

    def __call__(self, f, present, **scalars):
        vals = dict(self.defaults, **scalars)
        argv = [(self.bufs[a].ctypes.data if a in present else None) if a not in SCALARS else vals[a]
                for a in ARGS[f].split()]
        return getattr(self.lib, f)(*argv)


def test_every_combination_outside_the_old_sixteen_is_an_argument_error():
    call = _Caller()
    rejected = accepted = 0
    for f, ptrs in PTRS.items():
        sels = range(4) if SELECTOR[f] else (None,)
        relus = (0, 1) if f == "ssl4gie_bn_fwd" else (0,)
        subsets = [frozenset(itertools.compress(ptrs, bits)) for bits in itertools.product((0, 1), repeat=len(ptrs))]
        for sel, dtype, relu in itertools.product(sels, ANY, relus):
            kw = {SELECTOR[f]: sel} if SELECTOR[f] else {}
            for present in subsets:
                if _accepts(f, sel, dtype, relu, present):
                    accepted += 1
                    continue
                rc = call(f, present, dtype=dtype, relu=relu, **kw)
                assert rc == EARG, (f, sel, dtype, relu, sorted(present), rc)
                rejected += 1
    # the forms themselves: 2^optional pointers x dtypes x relu values each (a table typo shows up here)
    want = sum(2 ** len(fm["may"]) * (2 if name in NO_DTYPE else len(fm["dtypes"])) *
               (len(fm["relu"]) if f == "ssl4gie_bn_fwd" else 1)
               for f, forms in FORMS.items() for name, fm in forms.items())
    assert accepted == want and rejected > 100 * accepted, (accepted, want, rejected)


def test_every_form_rejects_sizes_dtypes_and_selectors_it_does_not_serve():
    """each of the old sixteen, with all and with none of its optional pointers: C % 8 == 0, rows > 0, parts > 0, the
    dtype codes and the selector range stay as they were (bn_coef_stats checks only C > 0, as it did)"""
    call = _Caller()
    for f, forms in FORMS.items():
        for name, fm in forms.items():
            base = {"dtype": fm["dtypes"][-1], "relu": fm["relu"][-1]}
            if SELECTOR[f]:
                base[SELECTOR[f]] = fm["sel"]
            bad = [{"C": 0}, {"C": -8}]
            if name not in ONLY_C_POSITIVE:
                bad += [{"C": 12}, {"C": 4}, {"rows": 0}, {"rows": -4}]
            if name not in NO_DTYPE:
                bad += [{"dtype": 2}, {"dtype": -1}]
            if "partial" in fm["need"]:
                bad += [{"parts": 0}, {"parts": -1}]
            if SELECTOR[f]:
                bad += [{SELECTOR[f]: 4}, {SELECTOR[f]: -1}]
            for present in (fm["need"], fm["need"] | fm["may"]):
                for b in bad:
                    rc = call(f, present, **dict(base, **b))
                    assert rc == EARG, (name, sorted(present), b, rc)


def test_workspace_bytes_cover_every_region():
    """[coef 3C][partials parts x 2C][sums 2C][pivot C] and the 64 x 2C fold of caller-supplied partials, for the
    partition counts of csrc/resnet_ops.hip's bn_parts (at least 64 rows of partials are always there)"""
    L = _lib.load()
    for rows, c in ((4, 8), (1 << 20, 64), (200704, 256), (1 << 26, 2048)):
        parts = min(1024, max(1, ((rows * c) >> 16) // ((c + 511) // 512)))
        floats = (3 + 2 * max(parts, 64) + 2 + 1) * c
        assert L.ssl4gie_bn_workspace_bytes(rows, c) >= 4 * floats
        assert L.ssl4gie_bn_workspace_bytes(rows, c) == 4 * (floats + 2 * 64 * c)   # unchanged from ABI 11
