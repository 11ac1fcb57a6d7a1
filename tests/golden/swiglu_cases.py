"""Parity cases of the DINOv2 ViT with the SwiGLU FFN (``ffn_layer="swiglufused"``: dinov2/layers/swiglu_ffn.py, the FFN of
ViT-g/14) at two small widths: embed_dim 128 -> hidden 344 (a width csrc/dense_gemm.hip refuses: library GEMMs around the
HIP gate) and embed_dim 192 -> hidden 512 (all four GEMMs hand-written).

``build`` and ``run_model`` drive the real reference (golden generation: make_swiglu_golden.py) and the product (tests/test_swiglu_host.py,
tests/test_swiglu_gpu.py) through the same calls.  Weights come from ``cases.fill_parameters`` (name-keyed), the image from
``cases.randn`` (tag-keyed); tests/golden/swiglu_vit.npz holds the image, the outputs and the reference's state_dict keys and
shapes of both cases."""
import os

import numpy as np
import torch

import cases

SPEC = dict(img_size=28, patch_size=14, depth=2, ffn_layer="swiglufused", init_values=1.0)
CASES = {
    "swiglu_vit_128": dict(embed_dim=128, num_heads=2),
    "swiglu_vit_192": dict(embed_dim=192, num_heads=3),
}
OUTPUTS = ("x_norm_clstoken", "x_norm_patchtokens", "x_prenorm")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "swiglu_vit.npz")


def image(name):
    return cases.randn(name + ".img", 2, 3, SPEC["img_size"], SPEC["img_size"])


def build(make, name):
    """make(**kw) -> a DinoVisionTransformer with name-keyed parameters (CPU, eval)."""
    m = make(**dict(SPEC, **CASES[name]))
    cases.fill_parameters(m, salt=name + ".")
    return m.eval()


def state_keys(m):
    """The sorted 'key:shape' list of a model's state_dict (what load_state_dict(strict=True) compares)."""
    return np.array(sorted(f"{k}:{tuple(v.shape)}" for k, v in m.state_dict().items()))


def run_model(m, name, device="cpu", autocast=False):
    """forward_features of the case's image -> {"<name>.<output>": ndarray} (+ the image itself)."""
    x = image(name)
    with torch.no_grad(), torch.autocast(device, dtype=torch.bfloat16, enabled=autocast):
        out = m.to(device)(x.to(device), is_training=True)
    res = {f"{name}.{k}": out[k].float().cpu().numpy() for k in OUTPUTS}
    res[f"{name}.img"] = x.numpy()
    return res


def check_golden(got, tol=1e-3):
    """The rule of tests/test_baselines_gpu.py::_check_golden on the entries of `got`: max error within tol of scale."""
    want = np.load(GOLDEN)
    assert set(got) <= set(want.files) and got
    for k in got:
        scale = max(1.0, float(np.abs(want[k]).max()))
        err = float(np.abs(got[k] - want[k]).max())
        assert err <= tol * scale, f"{k} max err {err:.3e} scale {scale:.3g}"
