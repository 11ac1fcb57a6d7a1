"""Generate the golden vectors of the SwiGLU-FFN DINOv2 ViT by RUNNING THE REAL REFERENCE on CPU.

    python tests/golden/make_swiglu_golden.py      # writes tests/golden/swiglu_vit.npz

Runs only where the reference is importable (``_ref_import.load_reference``).  The file holds the input image and the
reference's outputs, state_dict keys and shapes of both cases of swiglu_cases.py - no reference source, no weights (they are
filled by name)."""
import importlib
import os
import sys
from functools import partial

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import swiglu_cases as SC  # noqa: E402
from _ref_import import load_reference  # noqa: E402


def main():
    torch.set_num_threads(8)
    load_reference()
    vt = importlib.import_module("dinov2.models.vision_transformer")
    make = lambda **kw: vt.DinoVisionTransformer(block_fn=partial(vt.Block, attn_class=vt.MemEffAttention), block_chunks=0,
                                                 **kw)
    arrays = {}
    for name in SC.CASES:
        m = SC.build(make, name)
        ffn = m.blocks[0].mlp
        print(name, type(ffn).__name__, "w12", tuple(ffn.w12.weight.shape), "w3", tuple(ffn.w3.weight.shape))
        arrays.update(SC.run_model(m, name))
        arrays[f"{name}.state_keys"] = SC.state_keys(m)
    np.savez_compressed(SC.GOLDEN, **arrays)
    print(f"{os.path.basename(SC.GOLDEN)}: {len(arrays)} arrays, {os.path.getsize(SC.GOLDEN) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
