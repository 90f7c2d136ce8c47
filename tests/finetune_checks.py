"""fp64 restatements of the MAE fine-tuning recipe, shared by test_finetune_recipe_cpu.py and
test_gpu_finetune_recipe.py.  timm is not installed (as everywhere in this project), so this boundary is unpinned:
the rules are restated here from timm's published source (`timm.models.vision_transformer`, `timm.models.layers.drop`,
`timm.data.mixup`, `timm.loss.cross_entropy`) and from the MAE tree's `models_vit.py` / `util/lr_decay.py`, written
out statement by statement in plain torch so that they can be read against those sources.  Nothing is read from any
other tree; every function takes and returns CPU tensors and computes in the dtype of its inputs (the tests pass
fp64)."""
import math

import torch
import torch.nn.functional as F


# ---------------------------------------------------------------------------------------------- block and model
def block(sd, pre, x, heads, eps, s_attn=None, s_mlp=None):
    """timm Block with DropPath on both branches: x + drop_path(attn(norm1(x))), then x + drop_path(mlp(norm2(x))).
    `s_*` [B] is drop_path's per-sample random tensor already divided by keep_prob (0 or 1 / keep_prob)."""
    B, N, D = x.shape
    hd = D // heads
    h = F.layer_norm(x, (D,), sd[pre + "norm1.weight"], sd[pre + "norm1.bias"], eps)
    qkv = F.linear(h, sd[pre + "attn.qkv.weight"], sd[pre + "attn.qkv.bias"])
    qkv = qkv.reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    att = ((q * hd ** -0.5) @ k.transpose(-2, -1)).softmax(dim=-1)
    a = (att @ v).transpose(1, 2).reshape(B, N, D)
    a = F.linear(a, sd[pre + "attn.proj.weight"], sd[pre + "attn.proj.bias"])
    if s_attn is not None:
        a = a * s_attn.to(a.dtype).view(B, 1, 1)
    x = x + a
    h = F.layer_norm(x, (D,), sd[pre + "norm2.weight"], sd[pre + "norm2.bias"], eps)
    h = F.linear(F.gelu(F.linear(h, sd[pre + "mlp.fc1.weight"], sd[pre + "mlp.fc1.bias"])),
                 sd[pre + "mlp.fc2.weight"], sd[pre + "mlp.fc2.bias"])
    if s_mlp is not None:
        h = h * s_mlp.to(h.dtype).view(B, 1, 1)
    return x + h


def vit_logits(sd, imgs, depth, heads, patch, global_pool, eps=1e-6, drop_scales=None):
    """models_vit.VisionTransformer.forward: patch embedding (a stride-p convolution), cls concat, pos_embed add, the
    blocks, then mean over the patch tokens + fc_norm, or norm + the cls row; head."""
    B = imgs.shape[0]
    x = F.conv2d(imgs, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=patch)
    x = x.flatten(2).transpose(1, 2)
    x = torch.cat((sd["cls_token"].expand(B, -1, -1), x), dim=1) + sd["pos_embed"]
    for i in range(depth):
        sa = sm = None
        if drop_scales is not None:
            sa, sm = drop_scales[i, 0], drop_scales[i, 1]
        x = block(sd, f"blocks.{i}.", x, heads, eps, sa, sm)
    D = x.shape[-1]
    if global_pool:
        x = F.layer_norm(x[:, 1:, :].mean(dim=1), (D,), sd["fc_norm.weight"], sd["fc_norm.bias"], eps)
    else:
        x = F.layer_norm(x, (D,), sd["norm.weight"], sd["norm.bias"], eps)[:, 0]
    return F.linear(x, sd["head.weight"], sd["head.bias"])


# ---------------------------------------------------------------------------------------------- Mixup
def mixup_images(x, lam, box, use_cutmix):
    """timm Mixup._mix_elem, sample by sample from a copy of the unmixed batch: sample i against B - 1 - i, a box copy
    when use_cutmix[i], the blend x_i lam + x_j (1 - lam) otherwise (computed in x's dtype, the (1 - lam) in lam's)"""
    B = x.shape[0]
    orig = x.clone()
    out = x.clone()
    for i in range(B):
        j = B - 1 - i
        if int(use_cutmix[i]):
            y0, y1, x0, x1 = (int(v) for v in box[i])
            out[i][:, y0:y1, x0:x1] = orig[j][:, y0:y1, x0:x1]
        else:
            li = lam[i].to(x.dtype)
            out[i] = orig[i] * li + orig[j] * (1 - lam[i]).to(x.dtype)
    return out


def mixup_targets(target, lam, num_classes, smoothing, dtype=torch.float64):
    """timm mixup_target: one_hot(y) lam + one_hot(y.flip(0)) (1 - lam) with off = eps / C, on = 1 - eps + off"""
    off = smoothing / num_classes
    on = 1.0 - smoothing + off
    t = target.long().view(-1, 1)
    y1 = torch.full((t.shape[0], num_classes), off, dtype=dtype).scatter_(1, t, on)
    y2 = torch.full((t.shape[0], num_classes), off, dtype=dtype).scatter_(1, t.flip(0), on)
    l2 = lam.to(dtype).view(-1, 1)
    return y1 * l2 + y2 * (1.0 - l2)


# ---------------------------------------------------------------------------------------------- losses
def soft_target_ce(x, t):
    """timm SoftTargetCrossEntropy"""
    return torch.sum(-t * F.log_softmax(x, dim=-1), dim=-1).mean()


def label_smoothing_ce(x, y, smoothing):
    """timm LabelSmoothingCrossEntropy"""
    logp = F.log_softmax(x, dim=-1)
    nll = -logp.gather(dim=-1, index=y.unsqueeze(1)).squeeze(1)
    smooth = -logp.mean(dim=-1)
    return ((1.0 - smoothing) * nll + smoothing * smooth).mean()


def loss_and_grad(fn, x, *args, dtype=torch.float64):
    x = x.detach().clone().to(dtype).requires_grad_(True)
    args = [a.to(dtype) if torch.is_tensor(a) and a.is_floating_point() else a for a in args]
    loss = fn(x, *args)
    loss.backward()
    return loss.detach(), x.grad


# ---------------------------------------------------------------------------------------------- optimiser and groups
def adamw_first_step(p, g, lr, weight_decay, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.AdamW's first update from zero moments, in fp64"""
    p, g = p.double(), g.double()
    p = p * (1.0 - lr * weight_decay)
    m = (1.0 - betas[0]) * g
    v = (1.0 - betas[1]) * g * g
    mhat = m / (1.0 - betas[0])
    vhat = v / (1.0 - betas[1])
    return p - lr * mhat / (vhat.sqrt() + eps)


def layer_of(name, depth):
    """util/lr_decay.get_layer_id_for_vit with num_layers = depth + 1"""
    if name in ("cls_token", "pos_embed") or name.startswith("patch_embed"):
        return 0
    if name.startswith("blocks"):
        return int(name.split(".")[1]) + 1
    return depth + 1


def linspace_rates(rate, depth):
    return [rate * i / (depth - 1) if depth > 1 else 0.0 for i in range(depth)]


def five_sigma(keep, n):
    return 5.0 * math.sqrt(keep * (1.0 - keep) / n)
