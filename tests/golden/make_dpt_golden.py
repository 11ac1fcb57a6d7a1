"""Generate tests/golden/dpt_head.npz by RUNNING THE REAL REFERENCE on CPU: its DinoVisionTransformer, its DPTHead built as
_make_dinov2_dpt_depth_head builds it, its DepthEncoderDecoder and CenterPadding, wired as _make_dinov2_dpt_depther does.

    python tests/golden/make_dpt_golden.py

Runs only where the reference is importable (``_ref_import.load_reference``).  The file holds arrays and names - the head's
state-dict keys and shapes and the reference's outputs for the calls of dpt_cases.run - and no reference source; no weights
either: they are name-keyed (cases.fill_parameters)."""
import importlib
import os
import sys
from functools import partial

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import cases  # noqa: E402
import dpt_cases as PC  # noqa: E402
from _ref_import import load_reference  # noqa: E402


def main():
    torch.set_num_threads(8)
    load_reference()
    vt = importlib.import_module("dinov2.models.vision_transformer")
    depthers = importlib.import_module("dinov2.hub.depthers")
    depth = importlib.import_module("dinov2.hub.depth")
    utils = importlib.import_module("dinov2.hub.utils")
    backbone = vt.DinoVisionTransformer(block_fn=partial(vt.Block, attn_class=vt.MemEffAttention), block_chunks=0, **PC.SPEC)
    cases.fill_parameters(backbone, salt=PC.SALT)
    head = depthers._make_dinov2_dpt_depth_head(embed_dim=PC.SPEC["embed_dim"], min_depth=PC.MIN_DEPTH, max_depth=PC.MAX_DEPTH)
    PC.fill_head(head)
    model = depth.DepthEncoderDecoder(backbone=backbone, decode_head=head).eval()
    model.backbone.forward = partial(backbone.get_intermediate_layers, n=PC.OUT_INDEX, reshape=True, return_class_token=True,
                                     norm=False)
    model.backbone.register_forward_pre_hook(lambda _, x: utils.CenterPadding(PC.SPEC["patch_size"])(x[0]))
    sd = head.state_dict()
    arrays = {"keys": np.array(list(sd)), "shapes": np.array([" ".join(str(s) for s in v.shape) for v in sd.values()])}
    arrays.update(PC.run(model))
    for k, v in arrays.items():         # a golden whose pixels sit on the min_depth clamp hides everything
        if v.dtype == np.float32:
            assert not bool((v <= np.float32(PC.MIN_DEPTH)).any()), f"{k}: an output pixel sits on the min_depth clamp"
    path = os.path.join(HERE, "dpt_head.npz")
    np.savez_compressed(path, **arrays)
    for k, v in arrays.items():
        rng = f"[{float(v.min()):.4f}, {float(v.max()):.4f}]" if v.dtype == np.float32 else f"{len(v)} names"
        print(f"{k:12s} {str(v.shape):20s} {v.dtype}  {rng}")
    print(f"{path}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
