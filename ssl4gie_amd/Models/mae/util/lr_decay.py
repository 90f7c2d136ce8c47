"""Layer-wise learning-rate decay for the MAE fine-tuning recipe (reference: Models/mae/util/lr_decay.py:15-76,
called at main_finetune.py:283; the rule is BEiT's).  Every trainable parameter lands in one group named by its
layer and by whether it is decayed: layer 0 holds `cls_token`, `pos_embed` and the patch embedding, block i is layer
i + 1, and everything behind the blocks (`norm` / `fc_norm`, `head`) is layer depth + 1.  Layer l trains at
`layer_decay ** (depth + 1 - l)` of the base rate, carried as `lr_scale` (lr_sched.adjust_learning_rate applies it);
one-dimensional parameters and the names in `no_weight_decay_list` get `weight_decay` 0.  The groups go straight to
`optim.ArenaAdamW`."""


def get_layer_id_for_vit(name, num_layers):
    """layer of a parameter by its name; `num_layers` = depth + 1 is the layer of whatever follows the blocks"""
    if name in ("cls_token", "pos_embed") or name.startswith("patch_embed"):
        return 0
    if name.startswith("blocks"):
        return int(name.split(".")[1]) + 1
    return num_layers


def param_groups_lrd(model, weight_decay=0.05, no_weight_decay_list=[], layer_decay=.75):
    """-> list of {"lr_scale", "weight_decay", "params"} in order of first appearance in `model.named_parameters()`"""
    num_layers = len(model.blocks) + 1
    skip = set(no_weight_decay_list)
    groups = {}
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        decayed = not (p.ndim == 1 or name in skip)
        layer = get_layer_id_for_vit(name, num_layers)
        key = (layer, decayed)
        if key not in groups:
            groups[key] = {"lr_scale": layer_decay ** (num_layers - layer),
                           "weight_decay": weight_decay if decayed else 0.,
                           "params": []}
        groups[key]["params"].append(p)
    return list(groups.values())
