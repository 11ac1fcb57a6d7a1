"""Generate tests/golden/dense_tail_census.json: which kernels one forward + backward of the standard half launches, and how
often, for every routing of the residual tail (functional.DenseProjResidFn / DenseMlpFn) - {configuration: {timer name:
launches}} as ops.KERNEL_TIMER counts them.  The numbers of a run do not enter, only the routing.  Needs the GPU:

    python tests/golden/make_dense_tail_census.py

tests/test_dense_gpu.py imports census() from here, so the test and the fixture count the same passes.
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

PATH = os.path.join(HERE, "dense_tail_census.json")
DIM, HEADS, SHAPE = 256, 4, (3, 50, 256)       # 150 rows: ragged row tiles; 256 columns: the LayerNorm-tail kernel's least width

# module flags of octic_vits_amd.functional per configuration (everything else at its default)
CONFIGS = {
    "defaults": {},
    "no_next_norm": {"NEXT_NORM_FUSED": False},
    "no_ln_tail": {"LN_TAIL_FUSED": False},
    "resid_fused": {"NEXT_NORM_FUSED": False, "DENSE_RESID_FUSED": True},
    "mixed_routing": {"DENSE_HIP": {"qkv", "fc1"}},
    "library": {"DENSE_HIP": set()},
    "rows_to": {},          # the ragged pass of a DINOv2 backbone with batch-subset stochastic depth through row maps
}


def _two_blocks():
    from octic_vits_amd import vit
    torch.manual_seed(0)
    blocks = torch.nn.ModuleList([vit.Layer_scale_init_Block(dim=DIM, num_heads=HEADS, qkv_bias=True, init_values=0.5,
                                                             drop_path=0.0) for _ in range(2)]).cuda().train()
    vit.link_blocks(blocks)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(*SHAPE, generator=g).cuda().requires_grad_(True)
    cot = torch.randn(*SHAPE, generator=g).cuda()

    def run():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            h = x
            for blk in blocks:
                h = blk(h)
        h.backward(cot)
    return run


def _ragged_backbone():
    from octic_vits_amd import d8_layers, dinov2_models, vit
    torch.manual_seed(0)
    strip = lambda kw: {k: v for k, v in kw.items() if k != "init_values"}
    net = dinov2_models.OcticDinoVisionTransformer(
        img_size=32, patch_size=4, embed_dim=DIM, depth=4, num_heads=HEADS, drop_path_rate=0.4,
        octic_block_layers=lambda **kw: d8_layers.NestedTensorBlockD8(init_values=0.3, **strip(kw)),
        standard_block_layers=lambda **kw: vit.NestedTensorBlock(attn_class=vit.MemEffAttention, init_values=0.3,
                                                                 **strip(kw))).cuda().train()
    net.patch_embed.strict_img_size = False
    g = torch.Generator(device="cuda").manual_seed(1)
    xg = torch.randn(4, 3, 32, 32, generator=g, device="cuda")
    xl = torch.randn(8, 3, 16, 16, generator=g, device="cuda")

    def run():
        assert vit.ROW_MAPS
        torch.manual_seed(7)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            og, ol = net([xg, xl], masks=[None, None], is_training=True)
        (og["x_norm_patchtokens"].float().square().mean() + ol["x_norm_clstoken"].float().square().mean()).backward()
    return run


def census(name):
    """{timer name: launches} of one forward + backward under configuration `name`; the flags are put back."""
    from octic_vits_amd import functional as OF, ops
    run = _ragged_backbone() if name == "rows_to" else _two_blocks()
    flags = CONFIGS[name]
    saved = {k: getattr(OF, k) for k in flags}
    try:
        for k, v in flags.items():
            setattr(OF, k, set(v) if isinstance(v, set) else v)
        ops.KERNEL_TIMER.enable()
        run()
        summary = ops.KERNEL_TIMER.summary()
    finally:
        ops.KERNEL_TIMER.disable()
        for k, v in saved.items():
            setattr(OF, k, v)
    return {k: v["launches"] for k, v in sorted(summary.items())}


if __name__ == "__main__":
    res = {name: census(name) for name in CONFIGS}
    with open(sys.argv[1] if len(sys.argv) > 1 else PATH, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, c in res.items():
        print(f"{name:14s} {len(c):3d} kernels  {sum(c.values()):4d} launches")
