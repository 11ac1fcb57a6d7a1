"""The standard DeiT-III / DINOv2 baselines (octic_vits_amd/vit_models.py, dinov2_vit.py) without a GPU: registry names,
state_dict layouts against the reference's (tests/golden/baseline_facts.npz, made by make_baseline_golden.py), weight
decay exclusions, refusals."""
import os

import numpy as np
import pytest
import torch

import baseline_cases as BC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LS = ["deit_tiny_patch16_LS", "deit_small_patch16_LS", "deit_medium_patch16_LS", "deit_base_patch16_LS",
      "deit_large_patch16_LS", "deit_huge_patch14_LS"]


def test_all_eight_baselines_are_registered():
    from octic_vits_amd import deit_models as D
    for name in LS + ["vit_large", "vit_huge"]:
        assert name in D._LOCAL_REGISTRY, name


@pytest.mark.parametrize("name", list(BC.FACT_MODELS))
def test_state_dict_layout_equals_the_reference(name):
    from octic_vits_amd.deit_models import create_model
    facts = np.load(os.path.join(GOLDEN, "baseline_facts.npz"))
    with torch.device("meta"):
        m = create_model(name, **BC.FACT_MODELS[name])
    got = BC.state_dict_facts(m)
    for k, v in got.items():
        assert v == int(facts[f"{name}.{k}"][0]), f"{name}.{k}: {v} vs reference {int(facts[f'{name}.{k}'][0])}"


def test_deit_baseline_hyper_parameters_and_init():
    from octic_vits_amd.deit_models import create_model
    m = create_model("deit_huge_patch14_LS", num_classes=10)
    assert m.patch_embed.proj.kernel_size == (14, 14) and m.embed_dim == 1280 and len(m.blocks) == 32
    assert m.blocks[0].attn.num_heads == 16 and m.blocks[0].mlp.fc1.out_features == 5120
    assert m.blocks[0].norm1.eps == 1e-6 and m.norm.eps == 1e-6
    assert torch.all(m.blocks[3].gamma_1 == 1e-4)
    assert m.cls_token.shape == (1, 1, 1280) and m.pos_embed.shape == (1, 256, 1280)
    assert 0.015 < float(m.pos_embed.std()) < 0.025 and 0.015 < float(m.blocks[0].attn.qkv.weight.std()) < 0.025
    assert m.octic_equi_break_layer == 0
    assert all(hasattr(b, "_next_norm") for b in m.blocks[:-1])     # next-norm fusion linked across the stack


def test_no_weight_decay_names():
    from octic_vits_amd.deit_models import create_model
    m = create_model("deit_tiny_patch16_LS")
    assert m.no_weight_decay() == {"pos_embed", "cls_token", "_orig_mod.pos_embed", "_orig_mod.cls_token"}
    from octic_vits_amd.train import param_groups_weight_decay
    no_decay, decay = param_groups_weight_decay(m, 0.05, m.no_weight_decay())
    assert any(p is m.pos_embed for p in no_decay["params"]) and any(p is m.cls_token for p in no_decay["params"])
    assert all(p.ndim == 2 or p.ndim == 4 for p in decay["params"])


@pytest.mark.parametrize("name", LS + ["vit_large", "vit_huge"])
def test_pretrained_weights_are_refused(name):
    """The factories themselves refuse pretrained=True (create_model refuses it before the lookup for every name)."""
    from octic_vits_amd import dinov2_vit, vit_models
    factory = getattr(vit_models if name.startswith("deit") else dinov2_vit, name)
    with pytest.raises(RuntimeError, match="pretrained"):
        factory(pretrained=True)


def test_deit_baseline_refuses_a_non_native_resolution():
    from octic_vits_amd.deit_models import create_model
    m = create_model("deit_tiny_patch16_LS", img_size=64, num_classes=5).eval()
    with torch.no_grad():
        assert m(torch.randn(1, 3, 64, 64)).shape == (1, 5)
        with pytest.raises(ValueError, match="native resolution"):
            m(torch.randn(1, 3, 96, 96))


def test_dino_baseline_refuses_what_it_does_not_restate():
    from octic_vits_amd.dinov2_vit import DinoVisionTransformer
    with pytest.raises(NotImplementedError):
        DinoVisionTransformer(embed_dim=64, depth=2, num_heads=2, ffn_layer="swiglufused")
    with pytest.raises(NotImplementedError):
        DinoVisionTransformer(embed_dim=64, depth=2, num_heads=2, block_chunks=4)


def test_dino_position_resize_matrix_equals_interpolate():
    """The bicubic position resize as one matrix equals F.interpolate with the reference's scale factor (offset 0.1)."""
    import math
    from octic_vits_amd.dinov2_vit import DinoVisionTransformer
    m = DinoVisionTransformer(img_size=224, patch_size=16, embed_dim=64, depth=1, num_heads=2)
    pos = m.pos_embed.detach()
    M, D = 14, 64
    want = torch.nn.functional.interpolate(pos[0, 1:].reshape(1, M, M, D).permute(0, 3, 1, 2), mode="bicubic",
                                           scale_factor=(6.1 / M, 6.1 / M)).permute(0, 2, 3, 1).reshape(-1, D)
    got = m._pos_rows(96, 96)
    assert got.shape == (1 + 36, D)
    assert torch.allclose(got[0], pos[0, 0]) and torch.allclose(got[1:], want, atol=1e-6, rtol=1e-5)
    assert math.isclose(float((got[1:] - want).abs().max()), 0.0, abs_tol=1e-6)


@pytest.mark.parametrize("name", list(BC.DEIT_CASES) + list(BC.DINO_CASES))
def test_cpu_forward_matches_the_reference_goldens(name):
    """On the CPU the models run stock PyTorch ops (convolution, the blocks' eager path): the goldens hold to f32 rounding."""
    from functools import partial
    import torch.nn as nn
    from octic_vits_amd.dinov2_vit import DinoVisionTransformer
    from octic_vits_amd.vit_models import vit_models
    want = np.load(os.path.join(GOLDEN, name + ".npz"))
    if name in BC.DEIT_CASES:
        got = BC.run_deit_case(lambda **kw: vit_models(mlp_ratio=4, qkv_bias=True,
                                                       norm_layer=partial(nn.LayerNorm, eps=1e-6), **kw), name)
    else:
        got = BC.run_dino_case(lambda **kw: DinoVisionTransformer(**kw), name)
    assert set(got) == set(want.files)
    for k in want.files:
        scale = max(1.0, float(np.abs(want[k]).max()) if want[k].size else 1.0)
        assert np.allclose(got[k], want[k], rtol=1e-4, atol=1e-4 * scale), k
