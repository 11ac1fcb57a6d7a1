"""CPU: the DINOv2 schedules and parameter groups of octic_vits_amd/schedules.py against tests/golden/optim_*.npz, recorded
from the real reference (dinov2/utils/utils.py CosineScheduler, dinov2/train/train.py build_schedulers,
dinov2/utils/param_groups.py get_params_groups_with_decay; tests/golden/make_optim_golden.py), and the rule that turns one
iteration's values into the optimizer groups (SSLTrainer on its torch.optim.AdamW path)."""
import os
from functools import partial

import numpy as np
import pytest
import torch

import optim_case

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _fixture(name):
    return np.load(os.path.join(GOLDEN, name))


@pytest.mark.parametrize("case", sorted(optim_case.COSINE))
def test_cosine_scheduler_equals_the_reference(case):
    from octic_vits_amd.schedules import CosineScheduler
    want = _fixture("optim_schedules.npz")["cosine." + case]
    s = CosineScheduler(**optim_case.COSINE[case])
    got = np.array(optim_case.schedule_values(s))
    assert got.shape == want.shape and np.array_equal(got, want), case
    assert got[-1] == optim_case.COSINE[case]["final_value"]        # indices past the end


@pytest.mark.parametrize("case", sorted(optim_case.BUILD))
def test_build_schedulers_equals_the_reference(case):
    from octic_vits_amd.schedules import build_schedulers
    fx = _fixture("optim_schedules.npz")
    c = optim_case.BUILD[case]
    scheds = build_schedulers(c["optim"], c["teacher"], c["epoch_length"])
    for which, s in zip(optim_case.BUILD_NAMES, scheds):
        want = fx[f"build.{case}.{which}"]
        got = np.array(optim_case.schedule_values(s))
        assert got.shape == want.shape and np.array_equal(got, want), which
    frozen = c["optim"]["freeze_last_layer_epochs"] * c["epoch_length"]
    assert np.all(fx[f"build.{case}.last_layer_lr"][:frozen] == 0) and fx[f"build.{case}.last_layer_lr"][frozen] > 0


def _product_student():
    from octic_vits_amd import d8_layers, dinov2_models, ssl, vit
    torch.manual_seed(0)
    return optim_case.student(dinov2_models.OcticDinoVisionTransformer, d8_layers.NestedTensorBlockD8,
                              partial(vit.NestedTensorBlock, attn_class=vit.MemEffAttention), ssl.DINOHead)


def test_param_group_multipliers_equal_the_reference():
    """(lr_multiplier, wd_multiplier, is_last_layer) of every trainable tensor of a hybrid student - layer-wise decay over
    the blocks, x 0.2 for the patch embedding, no decay for biases / norms / gamma, the head's last layer flagged."""
    from octic_vits_amd.schedules import fuse_params_groups, params_groups_with_decay
    fx = _fixture("optim_groups.npz")
    want = {str(n): (float(a), float(b), bool(c)) for n, a, b, c in
            zip(fx["names"], fx["lr_multiplier"], fx["wd_multiplier"], fx["is_last_layer"])}
    student = _product_student()
    got = {}
    for k in student:
        per = params_groups_with_decay(student[k], lr_decay_rate=optim_case.LAYERWISE_DECAY,
                                       patch_embed_lr_mult=optim_case.PATCH_EMBED_LR_MULT)
        for d in per:
            got[k + "." + d["name"]] = (d["lr_multiplier"], d["wd_multiplier"], d["is_last_layer"])
        fused = fuse_params_groups(per)
        # fused groups: a partition of the tensors by their triple, one group per distinct triple
        assert sum(len(g["params"]) for g in fused) == len(per)
        keys = [(g["lr_multiplier"], g["wd_multiplier"], g["is_last_layer"]) for g in fused]
        assert len(set(keys)) == len(keys)
        for g in fused:
            ids = {id(p) for p in g["params"]}
            assert all((d["lr_multiplier"], d["wd_multiplier"], d["is_last_layer"]) == (g["lr_multiplier"], g["wd_multiplier"],
                                                                                          g["is_last_layer"])
                       for d in per if id(d["params"]) in ids)
    assert got == want
    assert len({v[0] for v in got.values()}) >= 5 and any(v[2] for v in got.values())


def test_apply_optim_scheduler_rule_and_none_keeps():
    from octic_vits_amd.schedules import apply_optim_scheduler
    groups = [{"lr": 1.0, "weight_decay": 1.0, "lr_multiplier": 0.5, "wd_multiplier": 1.0, "is_last_layer": False},
              {"lr": 1.0, "weight_decay": 1.0, "lr_multiplier": 1.0, "wd_multiplier": 0.0, "is_last_layer": True},
              {"lr": 1.0, "weight_decay": 1.0}]
    apply_optim_scheduler(groups, lr=4e-3, wd=0.04, last_layer_lr=0.0)
    assert [g["lr"] for g in groups] == [4e-3 * 0.5, 0.0, 4e-3]
    assert [g["weight_decay"] for g in groups] == [0.04, 0.0, 0.04]
    apply_optim_scheduler(groups, lr=None, wd=None, last_layer_lr=2e-3)          # only the last layer moves
    assert [g["lr"] for g in groups] == [4e-3 * 0.5, 2e-3, 4e-3]
    assert [g["weight_decay"] for g in groups] == [0.04, 0.0, 0.04]


def test_ssl_trainer_builds_reference_groups_on_the_torch_path():
    """SSLTrainer(optim_groups=...) on the torch.optim.AdamW path: one group per (sub-model, triple), lr = lr x
    lr_multiplier and weight_decay = wd x wd_multiplier from the start; the default stays the two decay groups."""
    from octic_vits_amd import ssl as S
    from octic_vits_amd.schedules import apply_optim_scheduler

    def make():
        from octic_vits_amd import d8_layers, dinov2_models, vit
        return dinov2_models.OcticDinoVisionTransformer(
            **optim_case.SPEC, octic_block_layers=partial(d8_layers.NestedTensorBlockD8, init_values=1e-5),
            standard_block_layers=partial(vit.NestedTensorBlock, attn_class=vit.MemEffAttention, init_values=1e-5))
    torch.manual_seed(0)
    arch = S.SSLMetaArch(make, optim_case.SPEC["embed_dim"], head_n_prototypes=32, head_hidden_dim=48, head_bottleneck_dim=16,
                         ibot_separate_head=True)
    plain = S.SSLTrainer(arch, lr=1e-3, weight_decay=0.04, fused_optimizer=False)
    assert len(plain.optimizer.param_groups) == 2
    assert [g["weight_decay"] for g in plain.optimizer.param_groups] == [0.04, 0.0]
    tr = S.SSLTrainer(arch, lr=1e-3, weight_decay=0.04, fused_optimizer=False,
                      optim_groups={"layerwise_decay": 0.9, "patch_embed_lr_mult": 0.2})
    pg = tr.optimizer.param_groups
    n_trainable = sum(1 for p in arch.student.parameters() if p.requires_grad)
    assert sum(len(g["params"]) for g in pg) == n_trainable and len(pg) > 6
    for g in pg:
        assert g["lr"] == 1e-3 * g["lr_multiplier"] and g["weight_decay"] == 0.04 * g["wd_multiplier"]
    patch = [g for g in pg if any(p is q for q in g["params"] for p in arch.student["backbone"].patch_embed.parameters())]
    assert patch and all(g["lr_multiplier"] == pytest.approx(0.2 * 0.9 ** 5) for g in patch)     # layer 0 of 4 blocks
    apply_optim_scheduler(pg, lr=2e-3, wd=0.1, last_layer_lr=0.0)
    assert all(g["lr"] == 0.0 for g in pg if g["is_last_layer"]) and any(g["is_last_layer"] for g in pg)
    assert all(g["lr"] == 2e-3 * g["lr_multiplier"] for g in pg if not g["is_last_layer"])
