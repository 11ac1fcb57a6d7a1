"""CPU-only: the host side of the linear probe (octic_vits_amd/probe.py) against goldens recorded from the real reference
(tests/golden/make_probe_golden.py: dinov2/eval/linear.py run on CPU), and the C ABI's argument checks.  No kernel runs."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

from octic_vits_amd import _lib, probe
from octic_vits_amd.build import build

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _g(name):
    return np.load(os.path.join(GOLDEN, name))


@pytest.mark.parametrize("world", [1, 8])
def test_grid_names_widths_rates_equal_the_reference(world):
    g = _g("probe_grid.npz")
    assert tuple(g["default_learning_rates"]) == probe.DEFAULT_LEARNING_RATES
    heads, n_groups = probe.classifier_grid(64, (1, 4), probe.DEFAULT_LEARNING_RATES, 128, world)
    assert list(heads) == list(g[f"w{world}_names"])
    assert [h["out_dim"] for h in heads.values()] == list(g[f"w{world}_widths"])
    assert [h["lr"] for h in heads.values()] == list(g[f"w{world}_lrs"])          # equal: the same float64 expression
    assert n_groups == int(g[f"w{world}_n_groups"]) == 52
    assert [probe.scale_lr(r, 128, world) for r in probe.DEFAULT_LEARNING_RATES] == list(g[f"w{world}_scaled"])


def test_name_collision_at_batch_128_on_one_gpu():
    """5e-6 and 1e-5 print alike: 48 classifiers for 52 groups, the survivor carries the LATER rate in the earlier position."""
    g = _g("probe_grid.npz")
    heads, n_groups = probe.classifier_grid(64, (1, 4), probe.DEFAULT_LEARNING_RATES, 128, 1)
    assert len(heads) == len(g["w1_names"]) == 48 and n_groups == 52
    first = next(iter(heads.values()))
    assert first["lr"] == probe.scale_lr(2e-5, 128) == 1e-5
    heads8, _ = probe.classifier_grid(64, (1, 4), probe.DEFAULT_LEARNING_RATES, 128, 8)
    assert len(heads8) == len(g["w8_names"]) == 52


@pytest.mark.parametrize("world", [1, 8])
def test_state_dict_keys_equal_the_reference(world):
    g = _g("probe_grid.npz")
    p = probe.LinearProbe(None, embed_dim=64, num_classes=10, batch_size=128, world_size=world)
    sd = p.state_dict()
    assert list(sd) == list(g[f"w{world}_state_keys"])
    for name, h in p.heads.items():
        assert tuple(sd[f"classifiers_dict.{name}.linear.weight"].shape) == (10, h["out_dim"])
        assert tuple(sd[f"classifiers_dict.{name}.linear.bias"].shape) == (10,)
        assert sd[f"classifiers_dict.{name}.linear.bias"].abs().max() == 0
    w = torch.cat([v.flatten() for k, v in sd.items() if k.endswith("weight")])
    assert abs(w.std().item() - 0.01) < 1e-3 and abs(w.mean().item()) < 1e-3     # normal_(0, 0.01)
    # round trip, and a DDP-wrapped checkpoint ("module." prefix)
    q = probe.LinearProbe(None, embed_dim=64, num_classes=10, batch_size=128, world_size=world)
    q.load_state_dict({"module." + k: v for k, v in sd.items()})
    assert torch.equal(q.flat, p.flat)
    with pytest.raises(KeyError):
        q.load_state_dict({k: v for k, v in list(sd.items())[:-1]})


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("reg", [0, 2])
def test_create_linear_input_equals_the_reference(dt, reg):
    g = _g("probe_inputs.npz")
    toks = torch.from_numpy(g[f"{dt}_reg{reg}_tokens"]).to(torch.float32 if dt == "f32" else torch.bfloat16)
    pairs = [(x[:, 1 + reg:], x[:, 0]) for x in toks]
    D = toks.shape[-1]
    full = probe.create_linear_input(pairs, 4, True)
    for n, avg, sl in ((1, False, slice(3 * D, 4 * D)), (1, True, slice(3 * D, 5 * D)), (4, False, slice(0, 4 * D)),
                       (4, True, slice(0, 5 * D))):
        out = probe.create_linear_input(pairs, n, avg)
        assert out.dtype == torch.float32
        assert torch.equal(out, torch.from_numpy(g[f"{dt}_reg{reg}_n{n}_avg{int(avg)}"]))
        assert torch.equal(out, full[:, sl])                  # every layout is a column range of one feature row


def test_probe_sgd_follows_torchs_cosine_schedule_exactly():
    p = probe.LinearProbe(None, embed_dim=64, num_classes=10, batch_size=128)
    opt = probe.ProbeSGD(p, momentum=0.9)
    assert len(opt.param_groups) == len(p) == 48
    stock = torch.optim.SGD([{"params": [torch.zeros(1, requires_grad=True)], "lr": h["lr"]} for h in p.heads.values()],
                            momentum=0.9, weight_decay=0)
    s0 = torch.optim.lr_scheduler.CosineAnnealingLR(opt, 20, eta_min=0)
    s1 = torch.optim.lr_scheduler.CosineAnnealingLR(stock, 20, eta_min=0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                       # scheduler.step() before optimizer.step(): no device here
        for _ in range(20):
            assert [g["lr"] for g in opt.param_groups] == [g["lr"] for g in stock.param_groups]
            s0.step()
            s1.step()
    assert [g["lr"] for g in opt.param_groups] == [g["lr"] for g in stock.param_groups]
    sd = opt.state_dict()
    assert [g["name"] for g in sd["param_groups"]] == p.names and sd["momentum_buffer"].abs().max() == 0
    opt2 = probe.ProbeSGD(probe.LinearProbe(None, embed_dim=64, num_classes=10, batch_size=128))
    opt2.load_state_dict(sd)
    assert [g["lr"] for g in opt2.param_groups] == [g["lr"] for g in opt.param_groups]


def test_probe_without_a_gpu_refuses_to_compute():
    p = probe.LinearProbe(None, embed_dim=64, num_classes=10, batch_size=16)
    opt = probe.ProbeSGD(p)
    with pytest.raises(RuntimeError, match="GPU only"):
        p.forward_features(torch.zeros(16, 320))
    with pytest.raises(RuntimeError, match="GPU only"):
        opt.step()
    with pytest.raises(NotImplementedError):
        p.evaluate([], metric_type="mean_per_class_accuracy")
    with pytest.raises(NotImplementedError):
        p.evaluate([], class_mapping=[0, 1])


def test_probe_symbols_exported_and_arguments_validated_without_gpu():
    path = build()
    L = _lib.lib()
    out = __import__("subprocess").run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    for s in ("octic_probe_features", "octic_probe_forward", "octic_probe_ce", "octic_probe_sgd"):
        assert s in _lib._PROTOS and s in _lib.header_symbols() and f" {s}\n" in out
    assert ctypes.sizeof(ctypes.c_void_p) * 4 + 16 == probe._HEAD_DTYPE.itemsize == 48
    a = ctypes.c_void_p(4096)
    # NULL pointers
    assert L.octic_probe_forward(None, 4, a, 320, 16, 10, a, None) == -4
    assert L.octic_probe_forward(a, 4, a, 320, 16, 10, None, None) == -4
    assert L.octic_probe_sgd(a, 4, 20, a, 320, a, 16, 10, None, 0.9, None) == -4
    assert L.octic_probe_ce(a, None, 4, 16, 10, None, a, a, None, None, None, None) == -4
    # sizes
    assert L.octic_probe_forward(a, 0, a, 320, 16, 10, a, None) == -1
    assert L.octic_probe_forward(a, 4, a, 320, 0, 10, a, None) == -1
    assert L.octic_probe_sgd(a, 4, 3, a, 320, a, 16, 10, a, 0.9, None) == -1          # fewer k-tiles than classifiers
    assert L.octic_probe_ce(a, a, 4, 16, 0, None, a, a, None, None, None, None) == -1
    # alignment: feature rows must stay 16-byte aligned
    assert L.octic_probe_forward(a, 4, ctypes.c_void_p(4100), 320, 16, 10, a, None) == -2
    assert L.octic_probe_forward(a, 4, a, 321, 16, 10, a, None) == -2
    cls = (ctypes.c_void_p * 1)(4096)
    ld = (ctypes.c_int64 * 1)(64 * 5)
    assert L.octic_probe_features(cls, ld, 1, a, 320, 64, _lib.F32, 2, 4, 96, a, 192, None) == -1     # D % 64
    assert L.octic_probe_features(cls, ld, 5, a, 320, 64, _lib.F32, 2, 4, 64, a, 384, None) == -1     # n > 4
    assert L.octic_probe_features(cls, ld, 1, a, 320, 64, 7, 2, 4, 64, a, 128, None) == -3
    assert L.octic_probe_features(cls, ld, 1, a, 320, 64, _lib.F32, 2, 4, 64, a, 64, None) == -1      # F narrower than (n+1) D
    assert L.octic_probe_features(cls, ld, 1, ctypes.c_void_p(4104), 320, 64, _lib.F32, 2, 4, 64, a, 128, None) == -2
