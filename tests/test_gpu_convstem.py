"""GPU tests of the MoCo-v3 conv-stem ViTs (reference Models/moco_v3/vits.py:72-143): the 3-channel 3x3
stride-2 stem kernels through the C ABI, then the ConvStem engine path against tests/golden/g19_convstem.npz
(made by tests/golden/make_golden_convstem.py from the reference's own classes).

Kernel tests use small integers, so every product and partial sum is exact in bf16 / fp32 and the comparison
with torch's fp64 convolution on the CPU is BIT-EXACT: a wrong window offset, MFMA lane mapping, edge mask or
reduction is an integer error."""
import os
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import keyed_weights, load_golden, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
F32 = torch.float32
EARG = 1000  # SSL4GIE_EARG


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssl4gie_amd import _lib
    _lib.load()


def ints(shape, seed, lo=-2, hi=3):
    g = torch.Generator("cpu").manual_seed(seed)
    return torch.randint(lo, hi, shape, generator=g).double()


# production (B = 64, 224 x 224, both widths) and edge shapes: partial tiles in both directions, odd sizes
KERNEL_SHAPES = [(64, 224, 224, 48), (64, 224, 224, 96),
                 (3, 40, 56, 16), (3, 40, 56, 32), (3, 37, 51, 16), (3, 37, 51, 32)]
KERNEL_CASES = [s + (BF,) for s in KERNEL_SHAPES] + [s + (F32,) for s in KERNEL_SHAPES[2:]] + \
               [(2, 2, 2, 16, BF), (2, 3, 131, 128, BF), (1, 300, 5, 80, BF), (2, 33, 259, 48, F32)]


@pytest.mark.parametrize("B,H,W,C0,dt", KERNEL_CASES)
def test_stem3x3_fwd_exact(B, H, W, C0, dt):
    from ssl4gie_amd import ops
    x = ints((B, 3, H, W), 1)
    w = ints((C0, 3, 3, 3), 2)
    ref = F.conv2d(x, w, None, stride=2, padding=1).permute(0, 2, 3, 1).contiguous()   # fp64, |.| <= 108
    y, stats = ops.stem3x3_fwd(x.float().to(DEV), w.float().to(DEV), dt, colstats=True)
    torch.cuda.synchronize()
    assert y.dtype == dt and y.shape == ref.shape
    assert torch.equal(y.double().cpu(), ref)
    y2 = ops.stem3x3_fwd(x.float().to(DEV), w.float().to(DEV), dt)   # without statistics: the same map
    assert torch.equal(y2, y)
    # per-tile sums are exact in fp32 (256 pixels x 108^2 < 2^24); the tiles are added in fp64 here
    assert stats.shape[1:] == (2, C0)
    s = stats.double().cpu().sum(0)
    flat = ref.view(-1, C0)
    assert torch.equal(s[0], flat.sum(0))
    assert torch.equal(s[1], (flat * flat).sum(0))


@pytest.mark.parametrize("B,H,W,C0,dt", KERNEL_CASES)
def test_stem3x3_wgrad_exact(B, H, W, C0, dt):
    from ssl4gie_amd import ops
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x = ints((B, 3, H, W), 3)
    dy = ints((B, Ho, Wo, C0), 4)
    # fp64 weight gradient of conv2d (|.| <= 4 B Ho Wo < 2^24 at every shape here)
    ref = torch.nn.grad.conv2d_weight(x, (C0, 3, 3, 3), dy.permute(0, 3, 1, 2).contiguous(), stride=2, padding=1)
    xd, dyd = x.float().to(DEV), dy.to(DEV, dt)
    dw = ops.stem3x3_wgrad(dyd, xd)
    torch.cuda.synchronize()
    assert dw.shape == (C0, 3, 3, 3) and dw.dtype == F32
    assert torch.equal(dw.double().cpu(), ref)
    dw2 = ops.stem3x3_wgrad(dyd, xd)                       # deterministic: no atomics
    assert torch.equal(dw2, dw)
    base = ints((C0, 3, 3, 3), 5, -50, 50)
    acc = base.float().to(DEV)
    ops.stem3x3_wgrad(dyd, xd, out=acc, accumulate=True)
    assert torch.equal(acc.double().cpu(), base + ref)


def test_stem3x3_rejects_what_it_does_not_take():
    from ssl4gie_amd import _lib, ops
    L = _lib.load()
    x = torch.zeros(2, 3, 32, 32, device=DEV)
    y = torch.zeros(2, 16, 16, 160, dtype=BF, device=DEV)
    w = torch.zeros(160, 3, 3, 3, device=DEV)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    st = ops.stream()
    for C0 in (20, 8, 0, 144):
        assert L.ssl4gie_stem3x3_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), 0, _lib.BF16, 2, 32, 32, C0, st) \
            == EARG
        assert L.ssl4gie_stem3x3_wgrad_workspace_bytes(_lib.BF16, 2, 32, 32, C0) == 0
        assert L.ssl4gie_stem3x3_wgrad(y.data_ptr(), x.data_ptr(), w.data_ptr(), ws.data_ptr(), ws.numel(), _lib.BF16,
                                       2, 32, 32, C0, 0, st) == EARG
    assert L.ssl4gie_stem3x3_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), 0, _lib.BF16, 2, 1, 32, 16, st) == EARG
    assert L.ssl4gie_stem3x3_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), 0, 7, 2, 32, 32, 16, st) == EARG
    assert L.ssl4gie_stem3x3_fwd(0, w.data_ptr(), y.data_ptr(), 0, _lib.BF16, 2, 32, 32, 16, st) == EARG
    # too small a workspace is an argument error, not an overrun
    assert L.ssl4gie_stem3x3_wgrad(y.data_ptr(), x.data_ptr(), w.data_ptr(), ws.data_ptr(), 16, _lib.BF16,
                                   2, 32, 32, 16, 0, st) == EARG
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.stem3x3_fwd(x, torch.zeros(20, 3, 3, 3, device=DEV), BF)


# ---------------------------------------------------------------------------------------------------------------
# the ConvStem engine path against the reference's own classes (tests/golden/g19_convstem.npz)
VIT_KW = dict(embed_dim=256, depth=2, num_heads=4, num_classes=64)


def _sample(t, n):
    """make_golden.py's strided sample"""
    f = t.detach().reshape(-1)
    step = max(1, f.numel() // n)
    return f[::step][:n]


def _stored(t, g):
    """a tensor as the fixture stores it: whole up to `small` elements, a strided sample of `ns` above"""
    return t.detach().reshape(-1) if t.numel() <= int(g["small"]) else _sample(t, int(g["ns"]))


def _small_vit(prec):
    from ssl4gie_amd.Models.moco_v3 import vits
    g = load_golden("g19_convstem.npz")
    m = vits.VisionTransformerMoCo(embed_layer=vits.ConvStem, **VIT_KW)
    keyed_weights(m, 91, g["vit/keys"], g["vit/digest"], keep=("pos_embed",))
    return m.to(DEV).set_precision(prec), g


def _vit_inputs():
    gen = torch.Generator("cpu").manual_seed(92)
    return torch.randn(4, 3, 224, 224, generator=gen), torch.randn(4, VIT_KW["num_classes"], generator=gen)


@pytest.mark.parametrize("D,seed", [(384, 93), (768, 94)])
def test_g19_stem_alone_fp32_matches_reference(D, seed):
    """fixture (a): the reference's ConvStem(embed_dim) alone at the production widths, training mode, on the fp32
    engine: tokens <= 1e-3, every parameter gradient <= 5e-3 (conftest.rel_err), running means <= 1e-3,
    running variances <= 3e-3, num_batches_tracked == 1 (the bars of test_g16 / the ResNet-head tests)"""
    from ssl4gie_amd.Models.moco_v3 import vits
    from ssl4gie_amd.resnet_engine import flush_batch_counts
    g = load_golden("g19_convstem.npz")
    m = vits.VisionTransformerMoCo(embed_dim=D, depth=1, num_heads=12, num_classes=8, embed_layer=vits.ConvStem)
    keyed_weights(m.patch_embed, seed, g[f"stem{D}/keys"], g[f"stem{D}/digest"])
    with torch.no_grad():   # [cls | tokens] + pos with a zero table: rows 1.. are the stem's tokens
        m.pos_embed.zero_()
        m.cls_token.zero_()
    m.to(DEV).set_precision("fp32").train()
    gen = torch.Generator("cpu").manual_seed(seed + 100)
    x = torch.randn(4, 3, 224, 224, generator=gen)
    w = torch.randn(4, 196, D, generator=gen)
    m._prepare()
    tok = m._conv_stem_tokens(x.to(DEV))[:, 1:]
    (tok * w.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert tok.shape == (4, 196, D)
    e = rel_err(_sample(tok, 8 * int(g["ns"])), g[f"stem{D}/tokens"])
    print(f"stem{D} fp32: tokens {e:.2e}")
    assert e < 1e-3
    assert abs(float(tok.detach().double().norm()) - float(g[f"stem{D}/tokens_norm"])) < 1e-3 * float(g[f"stem{D}/tokens_norm"])
    params = dict(m.patch_embed.named_parameters())
    names = g[f"stem{D}/names"].tolist()
    assert sorted(params) == names and len(names) == 14
    for k in names:
        assert params[k].grad is not None, k
        e = rel_err(_stored(params[k].grad, g), g[f"stem{D}/g/{k}"])
        print(f"stem{D} fp32: grad {k} {e:.2e}")
        assert e < 5e-3, (k, e)
    flush_batch_counts(m)
    for k, b in m.patch_embed.named_buffers():
        ref = g[f"stem{D}/buf/{k}"]
        if k.endswith("num_batches_tracked"):
            assert int(b) == int(ref) == 1, k
        else:
            assert rel_err(b, ref) < (1e-3 if k.endswith("running_mean") else 3e-3), k


def test_g19_whole_model_fp32_matches_reference():
    """fixture (b) on the fp32 engine: logits <= 1e-3, every gradient tensor <= 5e-3 against the reference's fp32 run"""
    m, g = _small_vit("fp32")
    x, w = _vit_inputs()
    m.train()
    logits = m(x.to(DEV))
    (logits * w.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    e = rel_err(logits, g["vit/logits_fp32"])
    print(f"vit fp32: logits {e:.2e}")
    assert e < 1e-3
    params = dict(m.named_parameters())
    names = g["vit/names"].tolist()
    assert sorted(k for k, p in params.items() if p.requires_grad) == names
    worst = 0.0
    for k in names:
        assert params[k].grad is not None, k
        e = rel_err(_stored(params[k].grad, g), g[f"vit/fp32/g/{k}"])
        worst = max(worst, e)
        assert e < 5e-3, (k, e)
    print(f"vit fp32: worst gradient {worst:.2e}")


def test_g19_whole_model_bf16_within_the_references_own_autocast_error():
    """fixture (b) on the bf16 engine, the G17 rule (tests/test_gpu_models_golden.py:_bf16_gate) unchanged: per-tensor
    relative L2 of the engine's gradient samples against the reference's fp64 samples; median, 90th percentile and the
    worst tensor of >= 1024 elements within 1.5 x the same statistic of the reference's own bf16-autocast errors, the
    smallest tensors within 3 x the reference's worst.  Every gradient tensor of the model enters.
    Reference (torch.autocast("cpu", bfloat16) vs fp64): logits 5.2e-3; gradients median 6.8e-3, p90 0.111, worst
    0.155 (patch_embed.proj.1.weight): the BatchNorm backward of the stem cancels heavily.
    Engine (bf16, MI355X, measured): logits 4.4e-3; gradients median 6.2e-3, p90 0.112, worst 0.152 (the same tensor)."""
    m, g = _small_vit("bf16")
    x, w = _vit_inputs()
    m.train()
    logits = m(x.to(DEV))
    (logits.float() * w.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    l64 = torch.from_numpy(g["vit/logits_fp64"]).double()
    le = float((logits.detach().double().cpu() - l64).norm() / l64.norm())
    names = g["vit/names"].tolist()
    ref_err = np.asarray(g["vit/autocast_err"], dtype=np.float64)
    params = dict(m.named_parameters())
    errs, big = [], []
    for k in names:
        assert params[k].grad is not None, k
        a = torch.from_numpy(g[f"vit/sample/{k}"]).double()
        b = _sample(params[k].grad, int(g["ns"])).double().cpu()
        errs.append(float((a - b).norm() / (a.norm() + 1e-300)))
        big.append(params[k].numel() >= 1024)
    errs, big = np.array(errs), np.array(big)
    order = np.argsort(-errs)[:4]
    print(f"vit bf16: logits {le:.3e} (reference autocast {float(g['vit/logits_autocast_err']):.3e}); gradients median "
          f"{np.median(errs):.3e} p90 {np.quantile(errs, 0.9):.3e} worst {errs.max():.3e} (reference "
          f"{np.median(ref_err):.3e} / {np.quantile(ref_err, 0.9):.3e} / {ref_err.max():.3e}); worst tensors " +
          ", ".join(f"{names[i]} {errs[i]:.3e} (ref {ref_err[i]:.3e})" for i in order))
    assert np.isfinite(le) and np.isfinite(errs).all()
    assert np.median(errs) <= 1.5 * np.median(ref_err), (np.median(errs), np.median(ref_err))
    assert np.quantile(errs, 0.9) <= 1.5 * np.quantile(ref_err, 0.9), (np.quantile(errs, 0.9), np.quantile(ref_err, 0.9))
    wb = int(np.argmax(np.where(big, errs, 0)))
    assert errs[wb] <= 1.5 * ref_err[big].max(), (names[wb], errs[wb], ref_err[big].max())
    assert errs.max() <= 3.0 * ref_err.max(), (names[int(errs.argmax())], errs.max(), ref_err.max())


def test_g19_eval_mode_and_statistics_under_no_grad():
    """fixture (c): two training-mode forwards under torch.no_grad() (what MoCo's momentum encoder does) move the
    running statistics and the batch count, then model.eval() normalises with them: output <= 1e-3 (fp32 engine)"""
    from ssl4gie_amd.resnet_engine import flush_batch_counts
    m, g = _small_vit("fp32")
    gen = torch.Generator("cpu").manual_seed(93)
    xt = [torch.randn(4, 3, 224, 224, generator=gen) for _ in range(2)]
    xe = torch.randn(4, 3, 224, 224, generator=gen)
    bn = m.patch_embed.proj[10]
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    m.train()
    with torch.no_grad():
        m(xt[0].to(DEV))
        torch.cuda.synchronize()
        assert not torch.equal(bn.running_mean, rm0) and not torch.equal(bn.running_var, rv0)
        flush_batch_counts(m)
        assert int(bn.num_batches_tracked) == 1 and int(m.patch_embed.proj[1].num_batches_tracked) == 1
        m(xt[1].to(DEV))
    flush_batch_counts(m)
    assert int(m.patch_embed.proj[1].num_batches_tracked) == int(g["eval/num_batches_tracked"]) == 2
    assert rel_err(bn.running_var, g["eval/running_var/proj.10"]) < 3e-3
    m.eval()
    rv1 = bn.running_var.clone()
    with torch.no_grad():
        y = m(xe.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(bn.running_var, rv1), "eval mode must not touch the running statistics"
    e = rel_err(y, g["eval/out"])
    print(f"vit eval fp32: {e:.2e}")
    assert e < 1e-3


def _conv_moco():
    from ssl4gie_amd.Models.moco_v3 import vits
    from ssl4gie_amd.Models.moco_v3.moco import builder
    return builder.MoCo_ViT(partial(vits.VisionTransformerMoCo, embed_dim=256, depth=2, num_heads=4,
                                    embed_layer=vits.ConvStem, stop_grad_conv1=True), 64, 256, 0.2)


def test_moco_step_on_a_conv_stem_backbone(monkeypatch):
    """MoCo_ViT over a vit_conv-style backbone: finite loss, a gradient on every base-encoder parameter (stem
    included; the fixed position table excepted), none on the momentum encoder, the EMA exact over the stem's
    parameters too, and the side-stream momentum branch the same arithmetic bit for bit"""
    torch.manual_seed(0)
    m = _conv_moco().to(DEV).set_precision("bf16")
    m._prepare()
    with torch.no_grad():
        for p in m.base_encoder.parameters():
            p.add_(torch.randn_like(p) * 0.01)
    before_b = [p.detach().clone() for p in m.base_encoder.parameters()]
    before_m = [p.detach().clone() for p in m.momentum_encoder.parameters()]
    m._update_momentum_encoder(0.99)
    assert len(before_b) == len(before_m) and any(p.dim() == 4 and p.shape[1:] == (3, 3, 3) for p in before_b)
    for pb, pm0, pm in zip(before_b, before_m, m.momentum_encoder.parameters()):
        assert torch.allclose(pm, pm0 * 0.99 + pb * (1.0 - 0.99), rtol=1e-6, atol=1e-8)
    for pb0, pb in zip(before_b, m.base_encoder.parameters()):
        assert torch.equal(pb0, pb)

    g = torch.Generator().manual_seed(6)
    x1 = torch.randn(8, 3, 224, 224, generator=g).to(DEV)
    x2 = torch.randn(8, 3, 224, 224, generator=g).to(DEV)

    def run(overlap):
        monkeypatch.setenv("SSL4GIE_MOCO_OVERLAP", "1" if overlap else "0")
        torch.manual_seed(0)
        mm = _conv_moco().to(DEV).set_precision("bf16")
        opt = torch.optim.AdamW([p for p in mm.parameters() if p.requires_grad], lr=1e-3)
        out = []
        for step in range(3):
            opt.zero_grad(set_to_none=True)
            loss = mm(x1, x2, 0.99)
            loss.backward()
            if step == 0:
                for name, p in mm.named_parameters():
                    if name.startswith("momentum_encoder.") or name.endswith("pos_embed"):
                        assert p.grad is None, name
                    else:
                        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
            opt.step()
            torch.cuda.synchronize()
            out.append(loss.detach().cpu().clone())
        grads = [p.grad.detach().cpu().clone() for p in mm.parameters() if p.grad is not None]
        mom = [p.detach().cpu().clone() for p in mm.momentum_encoder.parameters()]
        stats = [b.detach().cpu().clone() for n, b in mm.named_buffers() if "running" in n]
        return out, grads, mom, stats

    a, b = run(False), run(True)
    assert all(bool(torch.isfinite(x)) for x in a[0])
    for x, y in zip(a[0], b[0]):
        assert torch.equal(x, y), (float(x), float(y))
    for part in (1, 2, 3):
        assert len(a[part]) == len(b[part]) and len(a[part]) > 10
        for x, y in zip(a[part], b[part]):
            assert torch.equal(x, y)


def test_checkpoint_round_trip_of_a_conv_stem_model():
    """state_dict() -> checkpoints.load_matching into a fresh model: all 26 stem tensors (BatchNorm buffers
    included) are reported loaded and the two models compute the same thing"""
    from ssl4gie_amd import checkpoints
    from ssl4gie_amd.Models.moco_v3 import vits
    m, _ = _small_vit("fp32")
    x, _ = _vit_inputs()
    m.train()
    with torch.no_grad():
        m(x.to(DEV))            # the running statistics leave their initial values
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    torch.manual_seed(1)
    m2 = vits.VisionTransformerMoCo(embed_layer=vits.ConvStem, **VIT_KW)
    loaded, missing, unexpected = checkpoints.load_matching(m2, sd)
    stem = [k for k in loaded if k.startswith("patch_embed.proj.")]
    assert len(stem) == 26 and not missing and not unexpected
    assert int(m2.patch_embed.proj[4].num_batches_tracked) == 1
    m2.to(DEV).set_precision("fp32")
    for mode in ("eval", "train"):
        getattr(m, mode)()
        getattr(m2, mode)()
        with torch.no_grad():
            assert torch.equal(m(x.to(DEV)), m2(x.to(DEV))), mode


def _syncbn_worker(rank, world, port, q):
    """half of fixture (b)'s batch on each of two processes sharing the device, SyncBatchNorm children"""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), SSL4GIE_COMM_CUS="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    out = {}
    try:
        from ssl4gie_amd.Models.moco_v3 import vits
        m = vits.VisionTransformerMoCo(embed_layer=vits.ConvStem, **VIT_KW)
        keyed_weights(m, 91, keep=("pos_embed",))
        m = torch.nn.SyncBatchNorm.convert_sync_batchnorm(m)
        assert isinstance(m.patch_embed.proj[1], torch.nn.SyncBatchNorm)
        m.to(DEV).set_precision("fp32").train()
        x, w = _vit_inputs()
        sl = slice(2 * rank, 2 * rank + 2)
        logits = m(x[sl].to(DEV))
        ((logits * w[sl].to(DEV)).sum() / 2).backward()     # mean over the rank's images: the ranks' average is the
        torch.cuda.synchronize()                            # whole batch's mean
        out["logits"] = logits.detach().cpu()
        out["grads"] = {k: p.grad.detach().cpu() for k, p in m.named_parameters()
                        if k.startswith("patch_embed.") and p.grad is not None}
        out["running_var"] = m.patch_embed.proj[1].running_var.detach().cpu()
    except Exception:  # noqa: BLE001
        import traceback
        out["error"] = traceback.format_exc()
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_syncbatchnorm_conv_stem_two_processes_one_device():
    """convert_sync_batchnorm (main_moco.py:196) on a conv-stem model: two ranks with half a batch each exchange the
    stem's statistics — logits and (rank-averaged) stem gradients equal the one-process run on the whole batch at the
    fp32 bars (1e-3 / 5e-3)"""
    import socket
    import torch.multiprocessing as mp
    m, _ = _small_vit("fp32")
    x, w = _vit_inputs()
    m.train()
    logits = m(x.to(DEV))
    ((logits * w.to(DEV)).sum() / 4).backward()
    torch.cuda.synchronize()
    one = {k: p.grad.detach().cpu() for k, p in m.named_parameters() if k.startswith("patch_embed.")}
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_syncbn_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=240) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    for r in (0, 1):
        assert "error" not in res[r], res[r]["error"]
    both = torch.cat([res[0]["logits"], res[1]["logits"]])
    assert rel_err(both, logits.detach().cpu()) < 1e-3
    assert len(one) == 14 and sorted(res[0]["grads"]) == sorted(one)
    for k in sorted(one):
        avg = (res[0]["grads"][k] + res[1]["grads"][k]) / 2
        e = rel_err(avg, one[k])
        assert e < 5e-3, (k, e)
    for r in (0, 1):   # the running statistics are those of the WHOLE batch on both ranks
        assert rel_err(res[r]["running_var"], m.patch_embed.proj[1].running_var.detach().cpu()) < 3e-3
