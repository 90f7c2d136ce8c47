"""The loss kernels of loss_ops.hip — ssi_loss, dice_loss, infonce_loss, cross_entropy, soft_cross_entropy (given
targets and the label form) and bt_loss — against a plain fp64 reference, per element (tests/loss_checks.py: the
references, the bounds, how their constants were derived and the case list; tests/test_loss_checks_cpu.py: proof that
the checks bite).  bt_loss_grad is held bit for bit by tests/test_gpu_loss_heads.py.

Every kernel is called through the C ABI with its outputs and its workspace in the middle of a buffer that carries 256
sentinel elements on either side (`Guard`) and is itself filled with the sentinel.  Every case is run twice (same
bits, value and gradient) and, where the header allows a null gradient pointer, once more without it (same loss bits).

The branches the case list reaches (loss_checks.gpu_specs says how, shape by shape):
    infonce  spc = 2 (several sub-tiles per key chunk) with one row tile (8 x 4200) and with 16 (500 x 2200);
             a query of norm 0 (the g / eps branch); C = 1, N = 1; C = 1024
    bt_loss  D = 1025 (scalar path) and 1028 (ld4 path): the second trip of the row loop
    ssi      B = 300 > 256 (the finalize kernels' second trip), HW = 9216 > 8192 (the second grid-stride trip),
             3 x 5 and 7 x 9 (coarse grids with a single row or column), odd H and W, H = W = 1, an image with no, one
             and two equal valid pixels (det == 0)
    dice     B = 300, n = 8197 > 8192, n = 1
    ce       B = 2049 > 2048 rows per sweep, C = 63 / 64 / 65, C = 1, -inf logits, rows of weight 0

Run time on an MI355X: 46 tests in 2.5 s; the slowest after the first (which loads the library) takes 0.03 s."""
import math

import pytest
import torch

import loss_checks as lk

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64, I64, U8 = torch.float32, torch.float64, torch.int64, torch.uint8
EARG = 1000
SENTINEL, SENTINEL_BYTE, BAND = lk.SENTINEL, 0xAB, 256
WORST = {}      # worst error / (2^-24 mag) per check over the module (printed by the last test)
EXEMPT = {}     # case -> (exempt pixels, elements)
BIT_EQUAL = {}  # check -> (bit-equal elements, elements)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssl4gie_amd import _lib
    _lib.load()


def done(rep):
    for n, v in rep.worst.items():
        WORST[n] = max(WORST.get(n, 0.0), v)
    EXEMPT.update(rep.exempt)
    for n, (a, b) in rep.bit_equal.items():
        a0, b0 = BIT_EQUAL.get(n, (0, 0))
        BIT_EQUAL[n] = (a0 + a, b0 + b)
    rep.assert_ok()


class Guard:
    """outputs with BAND sentinel elements before and after, themselves filled with the sentinel"""

    def __init__(self):
        self.items = []

    def out(self, shape, dtype=F32):
        n = math.prod(shape)
        fill = SENTINEL_BYTE if dtype == U8 else SENTINEL
        buf = torch.full((n + 2 * BAND,), fill, dtype=dtype, device=DEV)
        self.items.append((buf, n, fill))
        return buf[BAND:BAND + n].view(shape)

    def check(self, tag):
        torch.cuda.synchronize()
        for buf, n, fill in self.items:
            assert bool((buf[:BAND] == fill).all()), "%s: written before the output" % tag
            assert bool((buf[BAND + n:] == fill).all()), "%s: written past the output" % tag

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((buf == fill).all()) for buf, n, fill in self.items)


def lib():
    from ssl4gie_amd import _lib
    return _lib.load()


def ptr(t):
    return 0 if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def on(c, *names):
    return [None if c[n] is None else c[n].to(DEV).contiguous() for n in names]


def bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------ the entry points; each returns (rc, outputs)
def call_ssi(G, p, t, B, H, W, alpha, scales, nulls=()):
    L = lib()
    loss, d = G.out((1,)), G.out((p.shape[0],) + tuple(p.shape[1:]))
    ws = G.out((max(L.ssl4gie_ssi_loss_workspace_bytes(*p.shape), 16),), U8)
    a = {"pred": ptr(p), "target": ptr(t), "loss": ptr(loss), "dpred": ptr(d), "ws": ptr(ws)}
    a.update({n: 0 for n in nulls})
    rc = L.ssl4gie_ssi_loss(a["pred"], a["target"], a["loss"], a["dpred"], B, H, W, float(alpha), int(scales), a["ws"], stream())
    return rc, {"loss": loss.view(()), "dpred": d}


def call_dice(G, l, t, B, n, smooth, nulls=()):
    L = lib()
    loss, d = G.out((1,)), G.out(tuple(l.shape))
    ws = G.out((max(L.ssl4gie_dice_loss_workspace_bytes(l.shape[0]), 16),), U8)
    a = {"logits": ptr(l), "target": ptr(t), "loss": ptr(loss), "dlogits": ptr(d), "ws": ptr(ws)}
    a.update({k: 0 for k in nulls})
    rc = L.ssl4gie_dice_loss(a["logits"], a["target"], a["loss"], a["dlogits"], B, n, float(smooth), a["ws"], stream())
    return rc, {"loss": loss.view(()), "dlogits": d}


def call_nce(G, q, k, N, M, C, T, off, nulls=()):
    L = lib()
    loss, d = G.out((1,)), G.out(tuple(q.shape))
    ws = G.out((max(L.ssl4gie_infonce_workspace_bytes(q.shape[0], k.shape[0], q.shape[1]), 16),), U8)
    a = {"q": ptr(q), "k": ptr(k), "loss": ptr(loss), "dq": ptr(d), "ws": ptr(ws)}
    a.update({n: 0 for n in nulls})
    rc = L.ssl4gie_infonce_loss(a["q"], a["k"], a["loss"], a["dq"], N, M, C, float(T), int(off), a["ws"], stream())
    return rc, {"loss": loss.view(()), "dq": d}


def call_ce(G, x, t, w, B, C, nulls=()):
    L = lib()
    loss, d = G.out((1,)), G.out(tuple(x.shape))
    ws = G.out((max(L.ssl4gie_cross_entropy_workspace_bytes(*x.shape), 16),), U8)
    a = {"logits": ptr(x), "target": ptr(t), "weight": ptr(w), "loss": ptr(loss), "dlogits": ptr(d), "ws": ptr(ws)}
    a.update({n: 0 for n in nulls})
    rc = L.ssl4gie_cross_entropy(a["logits"], a["target"], a["weight"], a["loss"], a["dlogits"], B, C, a["ws"], stream())
    return rc, {"loss": loss.view(()), "dlogits": d}


def call_softce(G, x, t, y, conf, off, B, C, nulls=()):
    L = lib()
    loss, d = G.out((1,)), G.out(tuple(x.shape))
    ws = G.out((max(L.ssl4gie_soft_cross_entropy_workspace_bytes(*x.shape), 16),), U8)
    a = {"logits": ptr(x), "soft": ptr(t), "label": ptr(y), "loss": ptr(loss), "dlogits": ptr(d), "ws": ptr(ws)}
    a.update({n: 0 for n in nulls})
    rc = L.ssl4gie_soft_cross_entropy(a["logits"], a["soft"], a["label"], float(conf), float(off), a["loss"], a["dlogits"],
                                      B, C, a["ws"], stream())
    return rc, {"loss": loss.view(()), "dlogits": d}


def call_bt(G, c, D, lambd, nulls=()):
    L = lib()
    loss = G.out((1,))
    ws = G.out((max(L.ssl4gie_bt_loss_workspace_bytes(c.shape[0]), 16),), U8)
    a = {"c": ptr(c), "loss": ptr(loss), "ws": ptr(ws)}
    a.update({n: 0 for n in nulls})
    rc = L.ssl4gie_bt_loss(a["c"], a["loss"], D, float(lambd), a["ws"], stream())
    return rc, {"loss": loss.view(())}


def softce_scalars(c):
    """(conf, off) as ssl4gie_amd.losses._SoftCeFn hands them over"""
    return (1.0 - lk.SMOOTHING, lk.SMOOTHING / c["shape"][1]) if c["form"] == "label" else (0.0, 0.0)


def entry(c, G, nulls=()):
    kind = c["kind"]
    if kind == "ssi":
        p, t = on(c, "pred", "target")
        return call_ssi(G, p, t, *c["shape"], c["alpha"], c["scales"], nulls)
    if kind == "dice":
        l, t = on(c, "logits", "target")
        return call_dice(G, l, t, *c["shape"], lk.DICE_SMOOTH, nulls)
    if kind == "nce":
        q, k = on(c, "q", "k")
        return call_nce(G, q, k, *c["shape"], c["T"], c["off"], nulls)
    if kind == "ce":
        x, t, w = on(c, "x", "t", "w")
        return call_ce(G, x, t, w, *c["shape"], nulls)
    if kind == "softce":
        x, t, y = on(c, "x", "t", "y")
        return call_softce(G, x, t, y, *softce_scalars(c), *c["shape"], nulls)
    c_, = on(c, "c")
    return call_bt(G, c_, c["shape"][0], lk.LAMBD, nulls)


GRAD = {"ssi": "dpred", "dice": "dlogits", "nce": "dq", "ce": "dlogits", "softce": "dlogits"}
NULLABLE = ("nce", "ce", "softce")      # the header allows dq / dlogits = NULL
SPECS = {kind: lk.gpu_specs(kind) for kind in lk.KINDS}


def run_case(kind, c, tag):
    G = Guard()
    rc, o = entry(c, G)
    assert rc == 0, (tag, rc)
    G.check(tag)
    G2 = Guard()
    rc2, o2 = entry(c, G2)                  # run to run: the same bits
    assert rc2 == 0
    G2.check(tag)
    for n in o:
        assert bits(o[n], o2[n]), "%s: %s differs between two calls" % (tag, n)
    if kind in NULLABLE:                    # forward only: the same loss bits, the gradient buffer untouched
        G3 = Guard()
        rc3, o3 = entry(c, G3, nulls=(GRAD[kind],))
        assert rc3 == 0
        G3.check(tag)
        assert bits(o3["loss"], o["loss"]), "%s: the forward-only loss differs" % tag
        assert bool((o3[GRAD[kind]] == SENTINEL).all()), "%s: the forward-only call wrote the gradient" % tag
    return lk.run_check(c, {k: v.cpu() for k, v in o.items()}, tag=tag)


def run_group(kind, group):
    rep = lk.Report()
    for grp, a in SPECS[kind]:
        if grp == group:
            rep.merge(run_case(kind, lk.make(kind, a), "%s %s %s" % (kind, group, a)))
    done(rep)


@pytest.mark.parametrize("group", lk.groups(SPECS["ssi"]))
def test_ssi_loss(group):
    """scales 1..4 and alpha 0, 0.5, 1 on the small shapes; `narrow` (the determinant cancels) at alpha = 0;
    `degenerate` (det == 0 with no, one and two valid pixels); `dyadic` (every intermediate exact, sign(0));
    `perfect_fit`; HW > 8192; B > 256"""
    run_group("ssi", group)


@pytest.mark.parametrize("group", lk.groups(SPECS["dice"]))
def test_dice_loss(group):
    run_group("dice", group)


@pytest.mark.parametrize("group", lk.groups(SPECS["nce"]))
def test_infonce_loss(group):
    run_group("nce", group)


def test_infonce_cases_reach_several_subtiles_per_chunk():
    """nce_plan restated: the two cases named for it have spc = 2, with one row tile and with 16; no older case has"""
    plans = {(s[0], s[1]): lk.nce_plan(s[0], s[1]) for s in lk.NCE_SHAPES}
    for nm in lk.NCE_SPC2:
        assert plans[nm][2] == 2, (nm, plans[nm])
    assert plans[(8, 4200)][0] == 1 and plans[(500, 2200)][0] == 16
    assert lk.nce_plan(256, 2048)[2] == 1 and lk.nce_plan(512, 4096)[2] == 2
    for (N, M), p in plans.items():
        assert p[3] <= lk.NCE_MAXCHUNK and (p[3] - 1) * p[2] < p[1] <= p[3] * p[2]


@pytest.mark.parametrize("group", lk.groups(SPECS["ce"]))
def test_cross_entropy(group):
    run_group("ce", group)


@pytest.mark.parametrize("group", lk.groups(SPECS["softce"]))
def test_soft_cross_entropy(group):
    run_group("softce", group)


@pytest.mark.parametrize("group", lk.groups(SPECS["bt"]))
def test_bt_loss(group):
    run_group("bt", group)


# ------------------------------------------------------------------ refusals
def _refused(what, fn):
    G = Guard()
    rc, _ = fn(G)
    assert rc == EARG, (what, rc)
    assert G.untouched(), "%s: a refused call wrote something" % what


def test_refusals_write_nothing():
    """every REQUIRE of the six entry points and of bt_loss_grad: rc = 1000, outputs and workspace keep their fill;
    B = 65536 by argument only (the check comes before any launch, no buffer of that size exists)"""
    c = lk.ssi_case("uniform", 2, 7, 9, 0.5, 4)
    p, t = on(c, "pred", "target")
    for n in ("pred", "target", "loss", "dpred", "ws"):
        _refused("ssi null " + n, lambda G: call_ssi(G, p, t, 2, 7, 9, 0.5, 4, nulls=(n,)))
    for what, a in (("B = 0", (0, 7, 9, 0.5, 4)), ("H = 0", (2, 0, 9, 0.5, 4)), ("W = 0", (2, 7, 0, 0.5, 4)),
                    ("B < 0", (-1, 7, 9, 0.5, 4)), ("scales = 0", (2, 7, 9, 0.5, 0)), ("scales = 5", (2, 7, 9, 0.5, 5)),
                    ("B = 65536", (65536, 1, 1, 0.5, 4))):
        _refused("ssi " + what, lambda G: call_ssi(G, p, t, *a))

    c = lk.dice_case("gauss", 3, 1000)
    l, t = on(c, "logits", "target")
    for n in ("logits", "target", "loss", "dlogits", "ws"):
        _refused("dice null " + n, lambda G: call_dice(G, l, t, 3, 1000, 1e-8, nulls=(n,)))
    for what, a in (("B = 0", (0, 1000)), ("n = 0", (3, 0)), ("n < 0", (3, -5)), ("B = 65536", (65536, 1))):
        _refused("dice " + what, lambda G: call_dice(G, l, t, *a, 1e-8))

    c = lk.nce_case("plain", 8, 24, 16, 4, 1.0)
    q, k = on(c, "q", "k")
    for n in ("q", "k", "loss", "ws"):
        _refused("nce null " + n, lambda G: call_nce(G, q, k, 8, 24, 16, 1.0, 4, nulls=(n,)))
    for what, a in (("N = 0", (0, 24, 16, 1.0, 0)), ("M = 0", (8, 0, 16, 1.0, 0)), ("C = 0", (8, 24, 0, 1.0, 0)),
                    ("C = 1025", (8, 24, 1025, 1.0, 0)), ("T = 0", (8, 24, 16, 0.0, 0)), ("T < 0", (8, 24, 16, -1.0, 0)),
                    ("off < 0", (8, 24, 16, 1.0, -1)), ("off + N > M", (8, 24, 16, 1.0, 17))):
        _refused("nce " + what, lambda G: call_nce(G, q, k, *a))

    c = lk.ce_case("plain", "weighted", 7, 63)
    x, t, w = on(c, "x", "t", "w")
    for n in ("logits", "target", "loss", "ws"):
        _refused("ce null " + n, lambda G: call_ce(G, x, t, w, 7, 63, nulls=(n,)))
    for what, a in (("B = 0", (0, 63)), ("C = 0", (7, 0)), ("B < 0", (-7, 63))):
        _refused("ce " + what, lambda G: call_ce(G, x, t, w, *a))

    c = lk.softce_case("plain", "soft", 7, 63)
    x, ts = on(c, "x", "t")
    y = torch.zeros(7, dtype=I64, device=DEV)
    for n in ("logits", "loss", "ws"):
        _refused("softce null " + n, lambda G: call_softce(G, x, ts, None, 0.0, 0.0, 7, 63, nulls=(n,)))
    _refused("softce both targets", lambda G: call_softce(G, x, ts, y, 0.9, 0.1 / 63, 7, 63))
    _refused("softce no target", lambda G: call_softce(G, x, None, None, 0.9, 0.1 / 63, 7, 63))
    for what, a in (("B = 0", (0, 63)), ("C = 0", (7, 0))):
        _refused("softce " + what, lambda G: call_softce(G, x, ts, None, 0.0, 0.0, *a))

    cc, = on(lk.bt_case("corr", 129), "c")
    for n in ("c", "loss", "ws"):
        _refused("bt null " + n, lambda G: call_bt(G, cc, 129, lk.LAMBD, nulls=(n,)))
    _refused("bt D = 0", lambda G: call_bt(G, cc, 0, lk.LAMBD))

    from ssl4gie_amd.ops import code
    L = lib()
    s = torch.ones((), device=DEV)

    def grad(G, D=129, dtype=code(F32), nulls=()):
        w, wt = G.out((129, 129)), G.out((129, 129))
        a = {"c": ptr(cc), "scale": ptr(s), "w": ptr(w), "wt": ptr(wt)}
        a.update({n: 0 for n in nulls})
        return L.ssl4gie_bt_loss_grad(a["c"], a["scale"], a["w"], a["wt"], dtype, D, float(lk.LAMBD), stream()), None

    for n in ("c", "scale", "w", "wt"):
        _refused("bt_grad null " + n, lambda G: grad(G, nulls=(n,)))
    _refused("bt_grad D = 0", lambda G: grad(G, D=0))
    _refused("bt_grad dtype", lambda G: grad(G, dtype=77))
    _refused("bt_grad more than 65535 tiles", lambda G: grad(G, D=65535 * 64 + 1))


# ------------------------------------------------------------------ wrappers
def _with_upstream(fn, x, factor):
    xd = x.to(DEV).requires_grad_(True)
    loss = fn(xd)
    (loss * factor).backward()
    return loss.detach(), xd.grad


def _wrapper_agrees(tag, c, fn, x):
    """loss and gradient of the wrapper equal the entry point's bits; an upstream gradient of 3 gives the entry
    point's gradient times 3, rounded once"""
    G = Guard()
    rc, o = entry(c, G)
    assert rc == 0
    l1, g1 = _with_upstream(fn, x, 1.0)
    l3, g3 = _with_upstream(fn, x, 3.0)
    want = o[GRAD[c["kind"]]].view(g1.shape)
    assert bits(l1, o["loss"]) and bits(l3, o["loss"]), tag
    assert bits(g1, want), tag
    assert bits(g3, want * 3.0), tag


def test_wrappers_agree_with_the_c_entry_points():
    from ssl4gie_amd import losses, ops
    c = lk.ssi_case("depth", 4, 17, 19, 0.5, 3)
    t = c["target"].to(DEV)
    _wrapper_agrees("ssi", c, lambda p: losses.ScaleAndShiftInvariantLoss(alpha=0.5, scales=3)(p, t[:, None]), c["pred"][:, None])
    c = lk.dice_case("gauss", 3, 1000)
    t2 = c["target"].to(DEV)
    _wrapper_agrees("dice", c, lambda l: losses.SoftDiceLoss(smooth=lk.DICE_SMOOTH)(l, t2), c["logits"])
    c = lk.nce_case("alike", 33, 99, 30, 66, 1.0)
    k = c["k"].to(DEV)
    _wrapper_agrees("nce", c, lambda q: losses.info_nce(q, k, c["T"], c["off"]), c["q"])
    for weights in lk.CE_WEIGHTS:
        c = lk.ce_case("plain", weights, 7, 65)
        fn = losses.CrossEntropyLoss(c["w"]).to(DEV)
        y = c["t"].to(DEV)
        _wrapper_agrees("ce " + weights, c, lambda x: fn(x, y), c["x"])
    c = lk.softce_case("mixup", "soft", 7, 65)
    ts = c["t"].to(DEV)
    _wrapper_agrees("softce soft", c, lambda x: losses.SoftTargetCrossEntropy()(x, ts), c["x"])
    c = lk.softce_case("plain", "label", 7, 65)
    y2 = c["y"].to(DEV)
    _wrapper_agrees("softce label", c, lambda x: losses.LabelSmoothingCrossEntropy(lk.SMOOTHING)(x, y2), c["x"])
    for D in (129, 1028):
        c = lk.bt_case("corr", D)
        rc, o = entry(c, Guard())
        assert rc == 0 and bits(ops.bt_loss(c["c"].to(DEV), lk.LAMBD), o["loss"])


def test_zz_worst_ratios():
    """the kernels' worst error / (2^-24 mag) per check over this module, for loss_checks' table; the exempt share
    per family and the bit-equal count of `dyadic`; every check of loss_checks was exercised at least once"""
    print("\n" + lk.table(WORST))
    share = {}
    for tag, (a, b) in EXEMPT.items():
        f = tag.split("'")[1]
        share[f] = max(share.get(f, 0.0), a / b)
    print("worst exempt share per family:", {f: "%.3f %%" % (100 * v) for f, v in sorted(share.items())})
    print("bit-equal elements:", BIT_EQUAL)
    missing = (set(lk.BOUNDED) | set(lk.EXACT)) - set(WORST)
    assert not missing, "never exercised: %s" % sorted(missing)
