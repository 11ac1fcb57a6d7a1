"""Cases for the DINOv2 optimizer schedules and parameter groups, shared by the golden generator (real reference) and the
host test of the product (octic_vits_amd/schedules.py)."""
from functools import partial

# CosineScheduler(**kw), read at every index up to 5 past total_iters
COSINE = {
    "warmup": dict(base_value=1e-3, final_value=1e-6, total_iters=40, warmup_iters=8, start_warmup_value=0),
    "freeze": dict(base_value=0.04, final_value=0.2, total_iters=30, warmup_iters=5, start_warmup_value=0.01, freeze_iters=4),
    "final": dict(base_value=0.992, final_value=1.0, total_iters=25),
    "all_warmup": dict(base_value=0.07, final_value=0.07, total_iters=12, warmup_iters=12, start_warmup_value=0.04),
}

# build_schedulers(optim, teacher, epoch_length): the keys of ssl_default_config.yaml's optim / teacher sections
BUILD = {
    "a": dict(optim=dict(lr=2e-3, min_lr=1e-6, epochs=6, warmup_epochs=2, weight_decay=0.04, weight_decay_end=0.2,
                         freeze_last_layer_epochs=1),
              teacher=dict(momentum_teacher=0.992, final_momentum_teacher=1.0, teacher_temp=0.07, warmup_teacher_temp=0.04,
                           warmup_teacher_temp_epochs=3),
              epoch_length=5),
    "b": dict(optim=dict(lr=5e-4, min_lr=1e-5, epochs=4, warmup_epochs=0, weight_decay=0.05, weight_decay_end=0.05,
                         freeze_last_layer_epochs=2),
              teacher=dict(momentum_teacher=0.996, final_momentum_teacher=1.0, teacher_temp=0.06, warmup_teacher_temp=0.04,
                           warmup_teacher_temp_epochs=1),
              epoch_length=7),
}
BUILD_NAMES = ("lr", "wd", "momentum", "teacher_temp", "last_layer_lr")
PAST_END = 5

# the reference recipe's groups (ssl_default_config.yaml:104-105)
LAYERWISE_DECAY, PATCH_EMBED_LR_MULT = 0.9, 0.2
SPEC = dict(img_size=32, patch_size=4, embed_dim=64, depth=4, num_heads=2)
HEAD = dict(out_dim=32, hidden_dim=48, bottleneck_dim=16, nlayers=3)


def schedule_values(s):
    return [float(s[i]) for i in range(s.total_iters + PAST_END)]


def student(backbone_cls, block_d8, block, head_cls):
    """A small hybrid DINOv2 student: backbone (4 blocks: 2 octic, 2 standard), dino_head, ibot_head."""
    import torch.nn as nn
    bb = backbone_cls(**SPEC, octic_block_layers=partial(block_d8, init_values=1e-5),
                      standard_block_layers=partial(block, init_values=1e-5))
    return nn.ModuleDict({"backbone": bb, "dino_head": head_cls(in_dim=SPEC["embed_dim"], **HEAD),
                          "ibot_head": head_cls(in_dim=SPEC["embed_dim"], **HEAD)})
