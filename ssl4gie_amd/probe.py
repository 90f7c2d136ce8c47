"""Linear probing on the engine: what the reference's two probe drivers do to a model around their training loop.

    Models/mae/main_linprobe.py     ViT (models_vit) + BatchNorm head, LARS, util/crop.py's RandomResizedCrop
    Models/moco_v3/main_lincls.py   ViT ('head') or ResNet50 ('fc'), torch.optim.SGD, torchvision's RandomResizedCrop

    model = models_vit.vit_base_patch16(num_classes=1000, global_pool=False)      # main_linprobe.py:186-189
    model.load_state_dict(checkpoint_model, strict=False)
    mae_linear_probe(model).cuda()                                                 # :218-227
    optimizer = LARS(model.head.parameters(), lr=lr, weight_decay=0.0)             # :252 (Models/mae/util/lars.py)
    loader = DeviceLoader(bank, 512, sampler=sampler, transform=data.MAELinprobeTransform(224))
    scores = metrics.TopKAccuracy((1, 5))                                          # engine_finetune.py:119-124
    for samples, targets in loader:
        loss = criterion(model(samples), targets); loss.backward(); optimizer.step(); optimizer.zero_grad()

    model = resnet50(num_classes=1000)                                             # main_lincls.py:160-161
    moco_linear_probe(model, "fc")                                                 # :164-169
    load_moco_pretrained(model, checkpoint["state_dict"], "fc")                    # :178-189
    optimizer = ArenaSGD(model, [p for p in model.parameters() if p.requires_grad], init_lr, momentum=0.9)  # :236-238
    model.eval()                                                                   # :348 (BN stays frozen)
    ...
    sanity_check(model.state_dict(), checkpoint["state_dict"], "fc")              # :434-455

The frozen trunk's forward is the bulk of a probe step and runs as it always did (forward only: no parameter needs a
gradient, so the block stack keeps one activation area and no backward graph).  What is new on the device sits
around it: scoring (metrics.TopKAccuracy), the head's optimizer step over its own segments (optim.ArenaSGD, LARS) and
the crop rule (data.tf_rrc_boxes).  `main_lincls.py`'s command line and ImageFolder stay out.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn


def mae_linear_probe(model):
    """main_linprobe.py:218-227: truncated-normal head weight (std 0.01), `head` <- Sequential(BatchNorm1d(in_features,
    affine=False, eps=1e-6), head), everything but the head frozen.  Returns the model."""
    head = model.head
    if not isinstance(head, nn.Linear):
        raise TypeError(f"mae_linear_probe needs a model whose head is an nn.Linear, got {type(head).__name__}")
    nn.init.trunc_normal_(head.weight, std=0.01)
    model.head = nn.Sequential(nn.BatchNorm1d(head.in_features, affine=False, eps=1e-6), head).to(head.weight.device)
    for _, p in model.named_parameters():
        p.requires_grad = False
    for _, p in model.head.named_parameters():
        p.requires_grad = True
    return model


def moco_linear_probe(model, linear_keyword):
    """main_lincls.py:164-169: freeze all layers but the last linear one (`linear_keyword`: 'head' for a ViT, 'fc' for a
    ResNet), whose weight is drawn from N(0, 0.01) and whose bias is zeroed.  Returns the model."""
    for name, param in model.named_parameters():
        if name not in ["%s.weight" % linear_keyword, "%s.bias" % linear_keyword]:
            param.requires_grad = False
    lin = getattr(model, linear_keyword)
    lin.weight.data.normal_(mean=0.0, std=0.01)
    lin.bias.data.zero_()
    return model


def load_moco_pretrained(model, state_dict, linear_keyword):
    """main_lincls.py:178-189 on a MoCo checkpoint's `state_dict`: keep `module.base_encoder.*` up to before the
    embedding layer, strip the prefix, load non-strictly and assert that exactly the linear layer is missing.  The
    caller's dict is not modified (the reference edits it in place).  Returns load_state_dict's result."""
    renamed = {}
    for k, v in state_dict.items():
        if k.startswith("module.base_encoder") and not k.startswith("module.base_encoder.%s" % linear_keyword):
            renamed[k[len("module.base_encoder."):]] = v
    msg = model.load_state_dict(renamed, strict=False)
    assert set(msg.missing_keys) == {"%s.weight" % linear_keyword, "%s.bias" % linear_keyword}, msg.missing_keys
    return msg


def sanity_check(state_dict, pretrained_state_dict, linear_keyword):
    """main_lincls.py:434-455: linear-classifier training must not change anything but the linear layer (e.g. update
    BatchNorm statistics).  Both arguments are dicts — `pretrained_state_dict` the MoCo checkpoint's `state_dict` with
    its `module.base_encoder.` prefix; a path goes through `checkpoints.load_file(path)["state_dict"]` first.  Raises
    AssertionError naming the first changed entry."""
    for k in list(state_dict.keys()):
        if "%s.weight" % linear_keyword in k or "%s.bias" % linear_keyword in k:  # only ignore linear layer
            continue
        k_pre = "module.base_encoder." + k[len("module."):] if k.startswith("module.") else "module.base_encoder." + k
        assert k_pre in pretrained_state_dict, "{} is missing from the pre-trained weights.".format(k_pre)
        assert bool((state_dict[k].cpu() == pretrained_state_dict[k_pre].cpu()).all()), \
            "{} is changed in linear classifier training.".format(k)


def adjust_learning_rate(optimizer, init_lr, epoch, epochs):
    """main_lincls.py:499-503: half-cycle cosine decay per epoch; returns the rate"""
    cur_lr = init_lr * 0.5 * (1. + math.cos(math.pi * epoch / epochs))
    for param_group in optimizer.param_groups:
        param_group["lr"] = cur_lr
    return cur_lr
