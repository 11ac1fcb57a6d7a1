"""Parity cases for the standard DeiT-III / DINOv2 baselines (octic_vits_amd/vit_models.py, octic_vits_amd/dinov2_vit.py).

``run_deit_case`` / ``run_dino_case`` drive the real reference (golden generation: make_baseline_golden.py) and the product
(tests/test_baselines_gpu.py) through the same calls; ``build_*`` takes the model class / factory so either side can be
plugged in.  Weights come from ``cases.fill_parameters`` (name-keyed), inputs from ``cases.randn`` (tag-keyed)."""
import numpy as np
import torch

import cases

# small-dimension models with the full-size layouts: p = 16 and p = 14 DeiT (K = 768 / 588 im2col columns),
# a 224 DINOv2 model with 4 register tokens and masks, and a 96 x 96 crop through interpolate_pos_encoding
DEIT_CASES = {
    "baseline_deit_p16": dict(img_size=64, patch_size=16, embed_dim=64, depth=2, num_heads=2, num_classes=10),
    "baseline_deit_p14": dict(img_size=56, patch_size=14, embed_dim=64, depth=2, num_heads=2, num_classes=10),
}
DINO_SPEC = dict(img_size=224, patch_size=16, embed_dim=64, depth=2, num_heads=2, init_values=1e-5)
DINO_CASES = {
    "baseline_dino": dict(num_register_tokens=0),
    "baseline_dino_reg4": dict(num_register_tokens=4),
}
# full-size models whose state_dict layout is pinned: (registry name, reference factory keywords)
FACT_MODELS = {
    "deit_large_patch16_LS": dict(),
    "deit_huge_patch14_LS": dict(),
    "vit_large": dict(init_values=1e-5, block_chunks=0),
    "vit_huge": dict(init_values=1e-5, block_chunks=0),
}


def state_dict_facts(m):
    """params, tensors, CRC of the sorted key list, CRC of the sorted 'key:shape' list."""
    import zlib
    sd = m.state_dict()
    keys = sorted(sd.keys())
    shapes = "\n".join(f"{k}:{tuple(sd[k].shape)}" for k in keys)
    return {"params": sum(p.numel() for p in m.parameters()), "tensors": len(list(m.parameters())),
            "keys_crc": zlib.crc32("\n".join(keys).encode()), "shapes_crc": zlib.crc32(shapes.encode())}


def run_deit_case(make, name, device="cpu"):
    """make(**spec) -> a vit_models; eval forward (logits) and the features of two images."""
    spec = DEIT_CASES[name]
    m = make(**spec)
    cases.fill_parameters(m, salt=name + ".")
    m = m.to(device).eval()
    s = spec["img_size"]
    x = cases.randn(name + ".img", 2, 3, s, s).to(device)
    with torch.no_grad():
        return {"logits": m(x).float().cpu().numpy(), "features": m.forward_features(x).float().cpu().numpy()}


def run_dino_case(make, name, device="cpu"):
    """make(**kw) -> a DinoVisionTransformer; forward_features at 224 (with masks) and on a 96 x 96 crop, the head output
    and the last block through get_intermediate_layers."""
    kw = dict(DINO_SPEC, **DINO_CASES[name])
    m = make(**kw)
    cases.fill_parameters(m, salt=name + ".")
    m = m.to(device).eval()
    G = DINO_SPEC["img_size"] // DINO_SPEC["patch_size"]
    x = cases.randn(name + ".img", 2, 3, 224, 224).to(device)
    xl = cases.randn(name + ".img96", 2, 3, 96, 96).to(device)
    masks = (cases.randn(name + ".mask", 2, G * G) > 0.6).to(device)
    res = {}
    with torch.no_grad():
        for tag, args in (("g", (x, masks)), ("g_nomask", (x, None)), ("l96", (xl, None))):
            out = m.forward_features(*args)
            for k in ("x_norm_clstoken", "x_norm_regtokens", "x_norm_patchtokens", "x_prenorm"):
                t = out[k] if k.endswith(("clstoken", "regtokens")) else out[k][:, ::5]   # (every fifth token: small files)
                res[f"{tag}.{k}"] = t.float().cpu().numpy()
        res["forward"] = m(x).float().cpu().numpy()
        inter = m.get_intermediate_layers(x, n=1, return_class_token=True)
        res["inter.patch"] = inter[0][0][:, ::5].float().cpu().numpy()
        res["inter.cls"] = inter[0][1].float().cpu().numpy()
    return res


def facts_arrays(facts_by_model):
    out = {}
    for name, f in facts_by_model.items():
        for k, v in f.items():
            out[f"{name}.{k}"] = np.array([v], dtype=np.int64)
    return out
