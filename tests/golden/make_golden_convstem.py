"""Generator of tests/golden/g19_convstem.npz: the MoCo-v3 conv-stem ViTs (reference Models/moco_v3/vits.py:72-143)
run through the reference's OWN classes on the CPU (on the timm restatement, as every other model fixture).

    python tests/golden/make_golden_convstem.py [--ref /path/to/reference]

Contents (numeric arrays and key lists only; weights are oracle.synth.keyed_tensor(key, shape, seed)):
  stem{384,768}/...  ConvStem(embed_dim) alone, training mode, B = 4 at 224 x 224, loss = sum(tokens * w): a strided
                     sample of the tokens, every parameter gradient (strided sample above 4096 elements), running
                     statistics and num_batches_tracked after the step
  vit/...            VisionTransformerMoCo(embed_dim=256, depth=2, num_heads=4, embed_layer=ConvStem, num_classes=64),
                     B = 4, loss = sum(logits * w): logits and gradient samples in fp32 and in fp64, and the
                     reference's own per-tensor error under torch.autocast("cpu", bfloat16) against its fp64 (the G17
                     recipe of make_golden.py)
  eval/...           the same model: two training-mode forwards, then model.eval() on a third batch (the G18 recipe)
  zoo/...            sorted state_dict keys, shapes, parameter counts and frozen parameters of vit_conv_small /
                     vit_conv_base (num_classes=256), with and without stop_grad_conv1
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from make_golden import _sample, import_reference_models, load_keyed  # noqa: E402

NS = 1024          # elements per strided sample
SMALL = 4096       # tensors up to this size are stored whole
SEED_W, SEED_X = 91, 92
VIT_KW = dict(embed_dim=256, depth=2, num_heads=4, num_classes=64)


def _pack(out, prefix, grads):
    names = sorted(grads)
    out[prefix + "names"] = np.array(names)
    for k in names:
        g = grads[k].detach()
        out[f"{prefix}g/{k}"] = (g.reshape(-1) if g.numel() <= SMALL else _sample(g, NS)).float().numpy().copy()


def stem_alone(vits, out):
    for D, seed in ((384, 93), (768, 94)):
        m = vits.ConvStem(embed_dim=D)
        shapes, digest = load_keyed(m, seed=seed)
        out[f"stem{D}/keys"] = np.array(sorted(shapes))
        out[f"stem{D}/digest"] = np.array(digest)
        m.train()
        gen = torch.Generator("cpu").manual_seed(seed + 100)
        x = torch.randn(4, 3, 224, 224, generator=gen)
        w = torch.randn(4, 196, D, generator=gen)
        tok = m(x)
        (tok * w).sum().backward()
        out[f"stem{D}/tokens"] = _sample(tok, 8 * NS).numpy().copy()
        out[f"stem{D}/tokens_norm"] = np.array(float(tok.double().norm()))
        _pack(out, f"stem{D}/", {k: p.grad for k, p in m.named_parameters()})
        for k, b in m.named_buffers():
            out[f"stem{D}/buf/{k}"] = b.detach().numpy().copy()
        print(f"g19 stem{D}: |tokens| {float(tok.double().norm()):.5f}", flush=True)


def whole_model(vits, out):
    gen = torch.Generator("cpu").manual_seed(SEED_X)
    x = torch.randn(4, 3, 224, 224, generator=gen)
    w = torch.randn(4, VIT_KW["num_classes"], generator=gen)
    res = {}
    for mode in ("fp32", "fp64", "bf16"):
        m = vits.VisionTransformerMoCo(embed_layer=vits.ConvStem, **VIT_KW)
        shapes, digest = load_keyed(m, seed=SEED_W, keep=("pos_embed",))
        m.train()
        if mode == "fp64":
            m.double()
            logits = m(x.double())
            loss = (logits * w.double()).sum()
        elif mode == "bf16":
            with torch.autocast("cpu", dtype=torch.bfloat16):
                logits = m(x)
            loss = (logits.float() * w).sum()
        else:
            logits = m(x)
            loss = (logits * w).sum()
        loss.backward()
        res[mode] = (logits.detach().double(), {k: p.grad.detach().double() for k, p in m.named_parameters()
                                                if p.grad is not None})
    out["vit/keys"] = np.array(sorted(shapes))
    out["vit/digest"] = np.array(digest)
    l64, g64 = res["fp64"]
    l32, g32 = res["fp32"]
    l16, g16 = res["bf16"]
    names = sorted(g64)
    assert names == sorted(g32) == sorted(g16)
    out["vit/logits_fp32"] = l32.float().numpy()
    out["vit/logits_fp64"] = l64.numpy()
    out["vit/logits_autocast_err"] = np.array(float((l16 - l64).norm() / l64.norm()))
    out["vit/names"] = np.array(names)
    _pack(out, "vit/fp32/", {k: g32[k] for k in names})
    errs, e32 = [], []
    for k in names:
        a, b, c = _sample(g64[k], NS), _sample(g16[k], NS), _sample(g32[k], NS)
        assert bool(torch.isfinite(b).all()), f"the reference's autocast gradient of {k} is not finite"
        out[f"vit/sample/{k}"] = a.float().numpy().copy()
        errs.append(float((a - b).norm() / (a.norm() + 1e-300)))
        e32.append(float((a - c).norm() / (a.norm() + 1e-300)))
    out["vit/autocast_err"] = np.array(errs, dtype=np.float64)
    e = np.array(errs)
    print(f"g19 vit: fp32 vs fp64: logits {float((l32 - l64).norm() / l64.norm()):.2e}, worst gradient {max(e32):.2e}; "
          f"autocast vs fp64: logits {float(out['vit/logits_autocast_err']):.3e}, gradients median {np.median(e):.3e} "
          f"p90 {np.quantile(e, 0.9):.3e} worst {e.max():.3e} ({names[int(e.argmax())]})", flush=True)


def eval_mode(vits, out):
    gen = torch.Generator("cpu").manual_seed(SEED_X + 1)
    xt = [torch.randn(4, 3, 224, 224, generator=gen) for _ in range(2)]
    xe = torch.randn(4, 3, 224, 224, generator=gen)
    m = vits.VisionTransformerMoCo(embed_layer=vits.ConvStem, **VIT_KW)
    load_keyed(m, seed=SEED_W, keep=("pos_embed",))
    m.train()
    with torch.no_grad():
        for x in xt:
            m(x)
    m.eval()
    with torch.no_grad():
        y = m(xe)
    out["eval/out"] = y.numpy()
    out["eval/running_var/proj.10"] = m.patch_embed.proj[10].running_var.numpy().copy()
    out["eval/num_batches_tracked"] = np.array(int(m.patch_embed.proj[1].num_batches_tracked))
    print(f"g19 eval: |out| {float(y.double().norm()):.5f}", flush=True)


def zoo(vits, out):
    for name in ("vit_conv_small", "vit_conv_base"):
        for stop in (False, True):
            m = getattr(vits, name)(num_classes=256, stop_grad_conv1=stop)
            sd = m.state_dict()
            keys = sorted(sd)
            tag = f"zoo/{name}/{'stop' if stop else 'plain'}"
            out[f"{tag}/frozen"] = np.array(sorted(k for k, p in m.named_parameters() if not p.requires_grad))
            if not stop:
                out[f"zoo/{name}/keys"] = np.array(keys)
                out[f"zoo/{name}/shapes"] = np.array([",".join(str(d) for d in sd[k].shape) for k in keys])
                out[f"zoo/{name}/params"] = np.array(sum(p.numel() for p in m.parameters()))
                out[f"zoo/{name}/depth"] = np.array(len(m.blocks))
                print(f"g19 zoo: {name}: {len(keys)} tensors, {int(out[f'zoo/{name}/params'])} parameters", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=None, help="root of the reference checkout (default: make_golden.py's)")
    a = ap.parse_args()
    if a.ref:
        mg.REF = os.path.abspath(a.ref)
    import_reference_models()
    import Models.moco_v3.vits as vits
    torch.manual_seed(0)
    out = {"ns": np.array(NS), "small": np.array(SMALL)}
    stem_alone(vits, out)
    whole_model(vits, out)
    eval_mode(vits, out)
    zoo(vits, out)
    path = os.path.join(HERE, "g19_convstem.npz")
    np.savez_compressed(path, **out)
    print(f"g19 ok: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
