"""Generate tests/golden/depth_linear.npz by RUNNING THE REAL REFERENCE on CPU: its DinoVisionTransformer, its BNHead built as
_make_dinov2_linear_depth_head builds it, its DepthEncoderDecoder and CenterPadding, wired as _make_dinov2_linear_depther does.

    python tests/golden/make_depth_golden.py

Runs only where the reference is importable (``_ref_import.load_reference``).  The file holds arrays and names - the head's
weights and the reference's outputs for the calls of depth_cases.run - and no reference source."""
import importlib
import os
import sys
from functools import partial

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import cases  # noqa: E402
import depth_cases as DC  # noqa: E402
from _ref_import import load_reference  # noqa: E402


def main():
    torch.set_num_threads(8)
    load_reference()
    vt = importlib.import_module("dinov2.models.vision_transformer")
    depthers = importlib.import_module("dinov2.hub.depthers")
    depth = importlib.import_module("dinov2.hub.depth")
    utils = importlib.import_module("dinov2.hub.utils")
    arrays = {}
    for layers in (4, 1):
        backbone = vt.DinoVisionTransformer(block_fn=partial(vt.Block, attn_class=vt.MemEffAttention), block_chunks=0, **DC.SPEC)
        cases.fill_parameters(backbone, salt=DC.SALT)
        head = depthers._make_dinov2_linear_depth_head(embed_dim=DC.SPEC["embed_dim"], layers=layers, min_depth=0.001,
                                                       max_depth=10.0)
        w, b = DC.head_weights(layers)
        with torch.no_grad():
            head.conv_depth.weight.copy_(w)
            head.conv_depth.bias.copy_(b)
        model = depth.DepthEncoderDecoder(backbone=backbone, decode_head=head).eval()
        model.backbone.forward = partial(backbone.get_intermediate_layers, n=DC.OUT_INDEX[layers], reshape=True,
                                         return_class_token=True, norm=False)
        model.backbone.register_forward_pre_hook(lambda _, x: utils.CenterPadding(DC.SPEC["patch_size"])(x[0]))
        arrays[f"L{layers}.conv_depth.weight"] = w.numpy().astype(np.float16)
        arrays[f"L{layers}.conv_depth.bias"] = b.numpy().astype(np.float16)
        arrays.update(DC.run(model, layers))
    pad = utils.CenterPadding(14)
    for size in (1, 13, 14, 15):
        arrays[f"pad.{size}"] = pad(torch.arange(1.0, 1 + 2 * size * (size + 1)).reshape(1, 2, size, size + 1)).numpy()
    path = os.path.join(HERE, "depth_linear.npz")
    np.savez_compressed(path, **arrays)
    for k, v in arrays.items():
        print(f"{k:28s} {str(v.shape):20s} {v.dtype}  [{float(v.min()):.4f}, {float(v.max()):.4f}]")
    print(f"{path}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
