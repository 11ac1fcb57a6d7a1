"""Optimizer schedules and parameter groups of the DINOv2 recipe, on the host (numpy; no device work).

* ``CosineScheduler`` / ``build_schedulers``: dinov2/utils/utils.py:67-87 and dinov2/train/train.py:71-116 - per-iteration
  lr, weight decay, teacher momentum, teacher temperature and the last layer's lr (0 for ``freeze_last_layer_epochs``).
* ``params_groups_with_decay`` / ``fuse_params_groups``: dinov2/utils/param_groups.py:13-103 - every trainable tensor of a
  sub-model gets an ``lr_multiplier`` (layer-wise decay over the blocks, x ``patch_embed_lr_mult`` for the patch embedding),
  a ``wd_multiplier`` (0 for biases, norms and layer scales) and ``is_last_layer`` (the DINO head's weight-normed last layer);
  tensors with equal triples share one group.
* ``apply_optim_scheduler``: dinov2/train/train.py:119-125, the rule that turns one iteration's values into the groups'
  ``lr`` / ``weight_decay``.

The engine's optimizers read those two keys from their ``param_groups`` at every step (``train.FusedLamb`` uploads them to
the device when they change, so a captured step follows them too)."""
import numpy as np


class CosineScheduler:
    """``freeze_iters`` zeros, a linear warm-up from ``start_warmup_value`` to ``base_value`` over ``warmup_iters``, then a
    half cosine from ``base_value`` to ``final_value`` over the remaining iterations; ``final_value`` past ``total_iters``."""

    def __init__(self, base_value, final_value, total_iters, warmup_iters=0, start_warmup_value=0, freeze_iters=0):
        self.final_value = final_value
        self.total_iters = total_iters
        freeze = np.zeros((freeze_iters))
        warmup = np.linspace(start_warmup_value, base_value, warmup_iters)
        iters = np.arange(total_iters - warmup_iters - freeze_iters)
        cosine = final_value + 0.5 * (base_value - final_value) * (1 + np.cos(np.pi * iters / len(iters)))
        self.schedule = np.concatenate((freeze, warmup, cosine))
        if len(self.schedule) != self.total_iters:
            raise ValueError("CosineScheduler: freeze_iters + warmup_iters exceed total_iters")

    def __getitem__(self, it):
        return self.final_value if it >= self.total_iters else self.schedule[it]


def build_schedulers(optim, teacher, epoch_length):
    """The five schedules of one DINOv2 run from the ``optim`` / ``teacher`` sections of its config (mappings with the keys
    of ssl_default_config.yaml) and ``train.OFFICIAL_EPOCH_LENGTH``: (lr, wd, momentum, teacher_temp, last_layer_lr).
    ``optim["lr"]`` is the lr after the config's batch-size scaling rule."""
    total = optim["epochs"] * epoch_length
    lr = dict(base_value=optim["lr"], final_value=optim["min_lr"], total_iters=total,
              warmup_iters=optim["warmup_epochs"] * epoch_length, start_warmup_value=0)
    temp_iters = teacher["warmup_teacher_temp_epochs"] * epoch_length
    lr_s = CosineScheduler(**lr)
    wd_s = CosineScheduler(optim["weight_decay"], optim["weight_decay_end"], total)
    mom_s = CosineScheduler(teacher["momentum_teacher"], teacher["final_momentum_teacher"], total)
    temp_s = CosineScheduler(teacher["teacher_temp"], teacher["teacher_temp"], temp_iters, warmup_iters=temp_iters,
                             start_warmup_value=teacher["warmup_teacher_temp"])
    last_s = CosineScheduler(**lr)
    last_s.schedule[:optim["freeze_last_layer_epochs"] * epoch_length] = 0
    return lr_s, wd_s, mom_s, temp_s, last_s


def _layer_id(name, num_layers, force_is_backbone, chunked_blocks):
    """0 for the embeddings, i + 1 for a tensor of block i, num_layers + 1 for everything else."""
    if not (name.startswith("backbone") or force_is_backbone):
        return num_layers + 1
    embeds = ("pos_embed", "patch_embed", "mask_token", "cls_token", "register_tokens")
    if any("." + e in name for e in embeds) or (force_is_backbone and any(e in name for e in embeds)):
        return 0
    if ".blocks." in name and ".residual." not in name:
        return int(name[name.find(".blocks."):].split(".")[2]) + 1
    if chunked_blocks and "blocks." in name and "residual." not in name:
        return int(name[name.find("blocks."):].split(".")[2]) + 1
    if "blocks." in name and "residual." not in name:
        return int(name[name.find("blocks."):].split(".")[1]) + 1
    return num_layers + 1


def params_groups_with_decay(model, lr_decay_rate=1.0, patch_embed_lr_mult=1.0):
    """One dict per trainable tensor of ``model`` (one student sub-model: backbone, dino_head, ibot_head), in
    ``named_parameters`` order: params (the tensor), name, lr_multiplier, wd_multiplier, is_last_layer."""
    chunked = False
    if hasattr(model, "n_blocks"):
        n_blocks, chunked = model.n_blocks, model.chunked_blocks
    elif hasattr(model, "blocks"):
        n_blocks = len(model.blocks)
    elif hasattr(model, "backbone"):
        n_blocks = len(model.backbone.blocks)
    else:
        n_blocks = 0
    out = []
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        lid = _layer_id(name, n_blocks, n_blocks > 0, chunked)
        d = {"params": p, "name": name, "lr_multiplier": lr_decay_rate ** (n_blocks + 1 - lid), "wd_multiplier": 1.0,
             "is_last_layer": "last_layer" in name}
        if name.endswith(".bias") or "norm" in name or "gamma" in name:
            d["wd_multiplier"] = 0.0
        if "patch_embed" in name:
            d["lr_multiplier"] = d["lr_multiplier"] * patch_embed_lr_mult
        out.append(d)
    return out


def fuse_params_groups(groups, keys=("lr_multiplier", "wd_multiplier", "is_last_layer")):
    """Tensors with equal ``keys`` in one group (groups in order of first appearance, tensors in the given order)."""
    fused = {}
    for d in groups:
        g = fused.setdefault(tuple(k + str(d[k]) for k in keys), {"params": []})
        for k in keys:
            g[k] = d[k]
        g["params"].append(d["params"])
    return list(fused.values())


def apply_optim_scheduler(param_groups, lr=None, wd=None, last_layer_lr=None):
    """One iteration's values into the groups: weight_decay = wd * wd_multiplier, lr = (last_layer_lr if is_last_layer else
    lr) * lr_multiplier (missing keys: multipliers 1, not the last layer).  A value that is None leaves the groups it
    would set as they are."""
    for g in param_groups:
        if wd is not None:
            g["weight_decay"] = wd * g.get("wd_multiplier", 1.0)
        base = last_layer_lr if g.get("is_last_layer", False) else lr
        if base is not None:
            g["lr"] = base * g.get("lr_multiplier", 1.0)
