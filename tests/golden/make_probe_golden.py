"""Generate tests/golden/probe_grid.npz, probe_inputs.npz and probe_trajectory.npz by RUNNING THE REAL REFERENCE on CPU:
dinov2/eval/linear.py (scale_lr, setup_linear_classifiers, create_linear_input, LinearClassifier) with torch.optim.SGD and
torch.optim.lr_scheduler.CosineAnnealingLR as linear.py:519-521 builds them.  linear.py is imported by file path; the packages
it imports at module level that are absent here or not needed (fvcore, constants, dinov2.data, dinov2.distributed with a
settable world size, dinov2.eval.metrics / setup / utils, dinov2.logging) are in-memory stand-ins, and Module.cuda() is a
no-op while setup_linear_classifiers runs.  Nothing of the reference is copied: the files hold numbers and names.

    python tests/golden/make_probe_golden.py
"""
import argparse
import enum
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _ref_import import REFERENCE_ROOT  # noqa: E402
WORLD = [1]


def _module(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def load_linear():
    def absent(*a, **k):
        raise RuntimeError("stand-in: not available in the golden maker")

    class MetricType(enum.Enum):
        MEAN_ACCURACY = "mean_accuracy"

    _module("fvcore")
    _module("fvcore.common")
    _module("fvcore.common.checkpoint", Checkpointer=absent, PeriodicCheckpointer=absent)
    _module("constants", IMAGENET_PATH="")
    for pkg in ("dinov2", "dinov2.eval"):
        _module(pkg).__path__ = []
    _module("dinov2.data", SamplerType=None, make_data_loader=absent, make_dataset=absent)
    _module("dinov2.data.transforms", make_classification_eval_transform=absent, make_classification_train_transform=absent)
    sys.modules["dinov2"].distributed = _module(
        "dinov2.distributed", get_global_size=lambda: WORLD[0], is_enabled=lambda: False, is_main_process=lambda: True)
    _module("dinov2.eval.metrics", MetricType=MetricType, build_metric=absent)
    _module("dinov2.eval.setup", get_args_parser=lambda parents=None, add_help=True: argparse.ArgumentParser(add_help=False),
            setup_and_build_model=absent)
    _module("dinov2.eval.utils", ModelWithIntermediateLayers=absent, evaluate=absent)
    _module("dinov2.logging", MetricLogger=absent)
    spec = importlib.util.spec_from_file_location("reference_linear", os.path.join(REFERENCE_ROOT, "dinov2", "eval", "linear.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def token_list(g, B, T, D, n, dtype, prefix):
    """n (patch tokens, class token) pairs sliced from [B, T, D] tensors, as get_intermediate_layers returns them."""
    xs = [torch.randn(B, T, D, generator=g).to(dtype) for _ in range(n)]
    return xs, [(x[:, prefix:], x[:, 0]) for x in xs]


def setup(lin, sample, n_list, rates, batch, classes, world):
    WORLD[0] = world
    keep = torch.nn.Module.cuda
    torch.nn.Module.cuda = lambda self, *a, **k: self
    try:
        return lin.setup_linear_classifiers(sample, n_list, rates, batch, classes)
    finally:
        torch.nn.Module.cuda = keep


def main():
    lin = load_linear()
    torch.manual_seed(20251016)              # LinearClassifier initialises from the global generator
    rates = lin.get_args_parser().get_default("learning_rates")
    g = torch.Generator().manual_seed(20251016)

    # ---- names, widths, scaled rates: the collision case (batch 128, world 1) and the clean one (world 8)
    grid = {"default_learning_rates": np.asarray(rates, dtype=np.float64)}
    _, sample = token_list(g, 2, 5, 64, 4, torch.float32, 1)
    for world in (1, 8):
        clfs, groups = setup(lin, sample, [1, 4], np.asarray(rates), 128, 10, world)
        d = clfs.classifiers_dict
        by_param = {id(p): float(gr["lr"]) for gr in groups for p in (list(gr["params"]))}
        grid[f"w{world}_names"] = np.asarray(list(d.keys()))
        grid[f"w{world}_widths"] = np.asarray([m.out_dim for m in d.values()], dtype=np.int64)
        grid[f"w{world}_lrs"] = np.asarray([by_param[id(m.linear.weight)] for m in d.values()], dtype=np.float64)
        grid[f"w{world}_n_groups"] = np.asarray(len(groups))
        grid[f"w{world}_state_keys"] = np.asarray(list(clfs.state_dict().keys()))
        grid[f"w{world}_scaled"] = np.asarray([lin.scale_lr(r, 128) for r in rates], dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, "probe_grid.npz"), **grid)

    # ---- create_linear_input: 4 layouts x {f32, bf16} x {0, 2 register tokens}
    inputs = {}
    for dt_name, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        for reg in (0, 2):
            xs, pairs = token_list(g, 3, 1 + reg + 6, 64, 4, dt, 1 + reg)
            key = f"{dt_name}_reg{reg}"
            inputs[f"{key}_tokens"] = torch.stack(xs).float().numpy()       # bf16 values are exact in f32
            for n in (1, 4):
                for avg in (False, True):
                    inputs[f"{key}_n{n}_avg{int(avg)}"] = lin.create_linear_input(pairs, n, avg).numpy()
    np.savez_compressed(os.path.join(HERE, "probe_inputs.npz"), **inputs)

    # ---- five iterations in float64: B = 16, D = 64, T = 1 + 4, 10 classes, 2 rates x 4 layouts
    B, D, T, C, iters, base = 16, 64, 5, 10, 5, [0.8, 1.6]
    traj = {"base_rates": np.asarray(base), "batch": np.asarray(B), "classes": np.asarray(C), "iters": np.asarray(iters)}
    xs, pairs = token_list(g, B, T, D, 4, torch.float32, 1)
    labels = torch.randint(0, C, (B,), generator=g)
    clfs, groups = setup(lin, pairs, [1, 4], np.asarray(base), B, C, 1)
    names = list(clfs.classifiers_dict.keys())
    assert len(names) == 8 and len(groups) == 8
    traj["tokens"] = torch.stack(xs).numpy()
    traj["labels"] = labels.numpy()
    traj["names"] = np.asarray(names)
    for name, m in clfs.classifiers_dict.items():
        traj[f"w0_{name}"] = m.linear.weight.detach().numpy().copy()         # f32 initial weights (the bias starts at 0)
    clfs = clfs.double()
    groups = [{"params": list(m.parameters()), "lr": float(gr["lr"])} for m, gr in zip(clfs.classifiers_dict.values(), groups)]
    opt = torch.optim.SGD(groups, momentum=0.9, weight_decay=0)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, iters, eta_min=0)
    feats = {name: lin.create_linear_input(pairs, m.use_n_blocks, m.use_avgpool).double() for name, m in clfs.classifiers_dict.items()}
    losses, lrs = [], []
    for _ in range(iters):
        lrs.append([gr["lr"] for gr in opt.param_groups])
        out = {name: m.linear(feats[name]) for name, m in clfs.classifiers_dict.items()}
        ls = {name: torch.nn.CrossEntropyLoss()(v, labels) for name, v in out.items()}
        loss = sum(ls.values())
        opt.zero_grad()
        loss.backward()
        opt.step()
        sched.step()
        losses.append([ls[name].item() for name in names])
    traj["losses"] = np.asarray(losses)
    traj["lrs"] = np.asarray(lrs)
    for name, m in clfs.classifiers_dict.items():
        traj[f"w_{name}"] = m.linear.weight.detach().numpy()
        traj[f"b_{name}"] = m.linear.bias.detach().numpy()
        traj[f"mw_{name}"] = opt.state[m.linear.weight]["momentum_buffer"].numpy()
        traj[f"mb_{name}"] = opt.state[m.linear.bias]["momentum_buffer"].numpy()
    np.savez_compressed(os.path.join(HERE, "probe_trajectory.npz"), **traj)
    for f in ("probe_grid.npz", "probe_inputs.npz", "probe_trajectory.npz"):
        print(f, os.path.getsize(os.path.join(HERE, f)), "bytes")
    print("world 1:", len(grid["w1_names"]), "classifiers /", int(grid["w1_n_groups"]), "groups; world 8:", len(grid["w8_names"]))


if __name__ == "__main__":
    main()
