"""LARS of the MAE linear probe (reference: Models/mae/util/lars.py:14-47, built at main_linprobe.py:252 over
`model_without_ddp.head.parameters()`): no rate scaling or weight decay for parameters of one dimension.

The signature is the reference's — it is handed parameters, not a model.  The arena those parameters live in is found
from them (engine.arena_of) at `step()`, because a model builds its arena at its first forward on the device.  The
update is `optim.ArenaLARS`'s (the three launches of ssl4gie_lars_arena) run over the hull of the head's segments
only: the momentum buffer and the workspace are hull-sized (3 MB for a ViT-B head of 0.77 M elements, where an
arena-sized buffer is 344 MB).  `param_groups[i]["lr"]` stays writable by `lr_sched.adjust_learning_rate`."""
from ....optim import RangedLARS


class LARS(RangedLARS):
    """`LARS(params, lr=0, weight_decay=0, momentum=0.9, trust_coefficient=0.001)`"""

    def __init__(self, params, lr=0, weight_decay=0, momentum=0.9, trust_coefficient=0.001):
        super().__init__(None, params, lr=lr, weight_decay=weight_decay, momentum=momentum,
                         trust_coefficient=trust_coefficient)
