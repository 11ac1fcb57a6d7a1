"""Generate the golden vectors of the standard DeiT-III / DINOv2 baselines by RUNNING THE REAL REFERENCE on CPU.

    python tests/golden/make_baseline_golden.py      # writes tests/golden/baseline_*.npz

Runs only where the reference is importable (``_ref_import.load_reference``).  The files hold the reference's outputs and
state_dict facts - no reference source.  The timm stand-in's ``PatchEmbed`` raises when built, and ``deit/vit.py`` binds
``Patch_layer=PatchEmbed`` at import, so the DeiT models get the Conv2d patch layer below (timm's arithmetic: one strided
Conv2d, flattened to tokens)."""
import importlib
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import baseline_cases as BC  # noqa: E402
from _ref_import import load_reference  # noqa: E402


class ConvPatchEmbed(nn.Module):
    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768):
        super().__init__()
        self.img_size, self.patch_size = (img_size, img_size), (patch_size, patch_size)
        self.num_patches = (img_size // patch_size) ** 2
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size)

    def forward(self, x):
        return self.proj(x).flatten(2).transpose(1, 2)


def main():
    torch.set_num_threads(8)
    ref = load_reference()
    dv = ref.deit_vit
    vt = importlib.import_module("dinov2.models.vision_transformer")
    total = 0

    def save(name, arrays):
        nonlocal total
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **arrays)
        total += os.path.getsize(path)
        print(f"{name:28s} {len(arrays):4d} arrays  {os.path.getsize(path) / 1024:8.1f} KiB")

    from functools import partial
    for name, spec in BC.DEIT_CASES.items():
        make = lambda **kw: dv.vit_models(mlp_ratio=4, qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6),
                                          block_layers=dv.Layer_scale_init_Block, Patch_layer=ConvPatchEmbed, **kw)
        save(name, BC.run_deit_case(make, name))
    for name in BC.DINO_CASES:
        make = lambda **kw: vt.DinoVisionTransformer(block_fn=partial(vt.Block, attn_class=vt.MemEffAttention),
                                                     block_chunks=0, **kw)
        save(name, BC.run_dino_case(make, name))
    facts = {}
    for mname, kw in BC.FACT_MODELS.items():
        if mname.startswith("deit"):
            m = getattr(dv, mname)(Patch_layer=ConvPatchEmbed, **kw)
        else:
            m = getattr(vt, mname)(**kw)
        facts[mname] = BC.state_dict_facts(m)
        print(mname, facts[mname])
    save("baseline_facts", BC.facts_arrays(facts))
    print(f"total {total / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
