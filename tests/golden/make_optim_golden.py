"""Generate tests/golden/optim_schedules.npz and tests/golden/optim_groups.npz by RUNNING THE REAL REFERENCE on CPU:
dinov2/utils/utils.py (CosineScheduler), dinov2/train/train.py (build_schedulers), dinov2/utils/param_groups.py
(get_params_groups_with_decay) on a small hybrid DINOv2 student (octic_vits/dinov2_models.py backbone, dinov2/layers
DINOHead heads).  Nothing of the reference is copied: the files hold numbers and parameter names.

    python tests/golden/make_optim_golden.py
"""
import ast
import importlib
import os
import sys
from functools import partial

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import optim_case  # noqa: E402
from _ref_import import REFERENCE_ROOT, load_reference  # noqa: E402


class _Cfg(dict):
    """Attribute and item access, as the reference's OmegaConf config offers both."""
    __getattr__ = dict.__getitem__


def reference_build_schedulers():
    """build_schedulers, compiled from its file on its own: the module around it imports the training-only packages
    (fvcore, wandb, the data pipeline)."""
    from dinov2.utils.utils import CosineScheduler
    path = os.path.join(REFERENCE_ROOT, "dinov2", "train", "train.py")
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "build_schedulers")
    ns = {"CosineScheduler": CosineScheduler, "print": lambda *a, **k: None}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), path, "exec"), ns)
    return ns["build_schedulers"]


def schedules():
    load_reference()
    from dinov2.utils.utils import CosineScheduler
    build = reference_build_schedulers()
    res = {}
    for name, kw in optim_case.COSINE.items():
        res["cosine." + name] = np.array(optim_case.schedule_values(CosineScheduler(**kw)), dtype=np.float64)
    for name, case in optim_case.BUILD.items():
        cfg = _Cfg(train=_Cfg(OFFICIAL_EPOCH_LENGTH=case["epoch_length"]), optim=_Cfg(case["optim"]),
                   teacher=_Cfg(case["teacher"]))
        for which, s in zip(optim_case.BUILD_NAMES, build(cfg)):
            res[f"build.{name}.{which}"] = np.array(optim_case.schedule_values(s), dtype=np.float64)
    return res


def groups():
    load_reference()
    dm = importlib.import_module("octic_vits.dinov2_models")
    head = importlib.import_module("dinov2.layers.dino_head").DINOHead
    pg = importlib.import_module("dinov2.utils.param_groups")
    student = optim_case.student(dm.OcticDinoVisionTransformer, dm.BlockD8, partial(dm.Block, attn_class=dm.MemEffAttention),
                                 head)
    names, lr_m, wd_m, last = [], [], [], []
    for k in student:
        for d in pg.get_params_groups_with_decay(student[k], lr_decay_rate=optim_case.LAYERWISE_DECAY,
                                                 patch_embed_lr_mult=optim_case.PATCH_EMBED_LR_MULT):
            names.append(k + "." + d["name"])
            lr_m.append(d["lr_multiplier"])
            wd_m.append(d["wd_multiplier"])
            last.append(d["is_last_layer"])
    return {"names": np.array(names), "lr_multiplier": np.array(lr_m, dtype=np.float64),
            "wd_multiplier": np.array(wd_m, dtype=np.float64), "is_last_layer": np.array(last, dtype=bool)}


if __name__ == "__main__":
    import logging
    logging.disable(logging.INFO)                # get_params_groups_with_decay logs one line per tensor
    for fname, res in (("optim_schedules.npz", schedules()), ("optim_groups.npz", groups())):
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **res)
        print(f"{fname:24s} {len(res):3d} arrays  {os.path.getsize(path) / 1024:6.1f} KiB")
