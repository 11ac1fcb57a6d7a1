"""Attentive-probe evaluation, host side (no GPU): the reference's modules and grid bookkeeping of
octic_vits_amd/classification.py, the fold identity of csrc/attnpool.hip in float64, and the argument checks of every new C
entry point (they return before any launch)."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from octic_vits_amd import _lib
from octic_vits_amd import classification as CL


def test_parameter_names_shapes_and_init():
    torch.manual_seed(0)
    a = CL.AttnPoolClassifier(256, 10)
    assert [(n, tuple(p.shape)) for n, p in a.named_parameters()] == [
        ("query_token", (256,)), ("kv.weight", (512, 256)), ("kv.bias", (512,)), ("linear.weight", (10, 256)), ("linear.bias", (10,))]
    assert a.num_heads == 4
    lin = CL.LinearClassifier(192, 7)
    assert [(n, tuple(p.shape)) for n, p in lin.named_parameters()] == [("linear.weight", (7, 192)), ("linear.bias", (7,))]
    for w in (a.kv.weight, a.linear.weight, lin.linear.weight, a.query_token):
        # trunc_normal_(std=0.02) cut at +-2 (100 sigma: never reached): mean 0, std 0.02
        assert w.abs().max() < 0.2 and abs(w.mean().item()) < 4 * 0.02 / w.numel() ** 0.5
        assert abs(w.std().item() - 0.02) < 0.02 * 4 / (2 * w.numel()) ** 0.5 + 1e-4
    assert a.kv.bias.abs().max() == 0 and a.linear.bias.abs().max() == 0 and lin.linear.bias.abs().max() == 0


def test_stock_forward_runs_on_cpu_and_matches_the_sdpa_formula():
    torch.manual_seed(1)
    m = CL.AttnPoolClassifier(128, 5).double()
    x = torch.randn(2, 5, 128, dtype=torch.float64)
    kv = m.kv(x).reshape(2, 5, 2, 2, 64)
    k, v = kv[:, :, 0], kv[:, :, 1]                                      # [B, N, H, 64]
    q = m.query_token.reshape(2, 64)
    p = torch.softmax(torch.einsum("hj,bnhj->bnh", q, k) / 8.0, dim=1)
    want = m.linear(torch.einsum("bnh,bnhj->bhj", p, v).reshape(2, 128))
    assert torch.allclose(m(x), want, rtol=1e-12, atol=1e-14)


def test_fold_identity_float64():
    torch.manual_seed(2)
    m = CL.AttnPoolClassifier(128, 5).double()
    with torch.no_grad():
        m.kv.bias.normal_()                                              # a nonzero key AND value bias
    x = torch.randn(2, 5, 128, dtype=torch.float64)
    stock = m(x)
    folded = m.linear(CL.fold_forward(m.query_token, m.kv.weight, m.kv.bias, x))
    assert (stock - folded).abs().max() <= 1e-12 * stock.abs().max()


def test_all_classifiers_key_order_pop_and_state_dict_round_trip():
    grid = CL.ClassifierGrid(None, representations=("cls", "patch"), learning_rates=(1e-3, 1e-2), weight_decays=(0.0, 0.1),
                             batch_size=8, num_classes=3, n_iters=10, warmup_iters=2, embed_dim=64)
    hp = list(itertools.product((1e-3, 1e-2), (0.0, 0.1)))
    assert grid.keys == [(s, h) for s in ("cls", "cls_avg_patch", "patch") for h in hp]
    assert [type(m).__name__ for m in grid.classifiers] == ["LinearClassifier"] * 8 + ["AttnPoolClassifier"] * 4
    assert grid.classifiers[4].linear.in_features == 128                 # cls_avg_patch is always there, 2 D wide
    sd = grid.state_dict()
    assert list(sd)[:2] == ["0.linear.weight", "0.linear.bias"]
    assert list(sd)[16:21] == ["8.query_token", "8.kv.weight", "8.kv.bias", "8.linear.weight", "8.linear.bias"]
    other = CL.ClassifierGrid(None, representations=("cls", "patch"), learning_rates=(1e-3, 1e-2), weight_decays=(0.0, 0.1),
                              batch_size=8, num_classes=3, n_iters=10, warmup_iters=2, embed_dim=64)
    assert not torch.equal(other.classifiers[8].kv.weight, grid.classifiers[8].kv.weight)
    flat_ptr = other.flat.data_ptr()
    other.load_state_dict({"module." + k: v for k, v in sd.items()})
    for (k, a), b in zip(sd.items(), other.state_dict().values()):
        assert torch.equal(a, b), k
    other.load_state_dict(sd)
    # the parameters still live in the flat buffer after loading
    p = other.classifiers[0].linear.weight
    assert p.data_ptr() == flat_ptr and torch.equal(other.flat[:p.numel()].view_as(p), p.data)
    popped = grid.classifiers.pop_key(("cls", hp[1]))
    assert isinstance(popped, CL.LinearClassifier) and len(grid.classifiers) == 11 and ("cls", hp[1]) not in grid.keys
    assert grid.keys[1] == ("cls", hp[2])


def test_schedule_matches_the_formula():
    n, w = 50, 7
    s = CL.lr_schedule(n, w)
    assert len(s) == n
    assert s[0] == 0.0 and s[w - 1] == 1.0 and s[w] == 1.0
    assert abs(s[n - 1]) < 1e-15
    for it in (0, w - 1):
        assert s[it] == it / (w - 1)
    for it in (w, w + 5, n - 1):
        assert abs(s[it] - (np.cos(np.pi * (it - w) / (n - w - 1)) + 1) / 2) < 1e-15


def test_lr_and_wd_of_every_parameter():
    grid = CL.ClassifierGrid(None, representations=("cls", "patch"), learning_rates=(1e-3, 1e-2), weight_decays=(5e-4, 0.1),
                             batch_size=128, num_classes=3, embed_dim=64)
    rows = grid.param_hyper()
    assert len(rows) == 8 * 2 + 4 * 5
    names = dict(grid.classifiers.named_parameters())
    for (name, base_lr, wd), key in zip(rows, [k for k in grid.keys for _ in range(2 if k[0] != "patch" else 5)]):
        assert name in names
        lr, want_wd = key[1]
        assert base_lr == lr * 128 / 256.0
        assert wd == (0.0 if "bias" in name else want_wd), name
    assert any(n.endswith("query_token") and wd == 0.1 for n, _, wd in rows)


def test_any_match_accuracy_hand_counted():
    # 2 heads, 4 classes, 5 samples; sample 3 has no valid target and is left out
    pred = torch.tensor([[0, 1, 2, 3, 0], [2, 2, 2, 2, 2]])
    preds = F.one_hot(pred, 4).float().permute(0, 2, 1)                  # [n_head, n_cls, bs]
    target = torch.tensor([[0, -1, -1], [2, 1, -1], [3, 0, 1], [-1, -1, -1], [1, -1, -1]])
    m = CL.AnyMatchAccuracy(top_k=1)
    m.update(preds, target[None].expand(2, -1, -1))
    # head 0: hits samples 0, 1 of the 4 counted; head 1: hits sample 1 only
    assert m.compute().tolist() == [0.5, 0.25]
    m.update(preds[:, :, :1], torch.tensor([[0]])[None].expand(2, -1, -1))
    assert m.compute().tolist() == [np.float32(3) / np.float32(5), np.float32(1) / np.float32(5)]      # a float32 mean
    m5 = CL.AnyMatchAccuracy(top_k=2)
    scores = torch.tensor([[[0.1], [0.5], [0.4], [0.0]]])                # top-2 = classes 1, 2
    m5.update(scores, torch.tensor([[[2, -1]]]))
    assert m5.compute().tolist() == [1.0]


def test_best_key_takes_the_first_maximum():
    keys = [("cls", (1, 0)), ("cls", (2, 0)), ("cls", (3, 0)), ("patch", (1, 0)), ("patch", (2, 0))]
    best = CL.best_keys(keys, [0.5, 0.7, 0.7, 0.2, 0.2])
    assert best == {"cls": ("cls", (2, 0)), "patch": ("patch", (1, 0))}


def test_refusals():
    with pytest.raises(AssertionError):
        CL.AttnPoolClassifier(96, 4)
    for rep in ("objects", "avg_objects", "concat_objects"):
        with pytest.raises(ValueError, match="register"):
            CL.ClassifierGrid(None, representations=("cls", rep), learning_rates=(1e-3,), weight_decays=(0.0,), num_classes=3,
                              embed_dim=64, num_register_tokens=0)
    ok = CL.ClassifierGrid(None, representations=("objects",), learning_rates=(1e-3,), weight_decays=(0.0,), num_classes=3,
                           embed_dim=64, num_register_tokens=4)
    assert [k[0] for k in ok.keys] == ["cls_avg_patch", "reg"]
    grid = CL.ClassifierGrid(None, representations=("patch",), learning_rates=(1e-3,), weight_decays=(0.0,), num_classes=3,
                             embed_dim=64)
    with pytest.raises(RuntimeError, match="GPU only"):
        grid.step(torch.zeros(2, 3, 28, 28), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="GPU only"):
        grid.step_features({"cls_avg_patch": torch.zeros(2, 128), "patch": torch.zeros(2, 4, 64)}, torch.zeros(2, dtype=torch.int64))


class _Regless(nn.Module):
    def forward_features(self, x):
        return {"x_norm_clstoken": torch.zeros(1, 64), "x_norm_regtokens": torch.zeros(1, 0, 64),
                "x_norm_patchtokens": torch.zeros(1, 4, 64)}


def test_features_dictionary_and_objects_refusal():
    out = CL.features(_Regless(), None, ("cls", "avg_patch", "patch"))
    assert list(out) == ["cls", "avg_patch", "cls_avg_patch", "patch"] and out["cls_avg_patch"].shape == (1, 128)
    assert out["patch"].dtype == torch.float32
    with pytest.raises(ValueError, match="register"):
        CL.features(_Regless(), None, ("cls", "objects"))


# ------------------------------------------------------------------------------------------------ C entry points, no device
P = 1 << 20            # a well-aligned fake address: every check runs before any launch, nothing is dereferenced


def _calls(L):
    """name -> (call with good arguments replaced per (position -> value)); the good call itself is never made."""
    return {
        "fold": (L.octic_attnpool_fold, [P, P, 2, 128, P, 4, None], {"shape": {3: 96}, "align": {4: P + 4}, "null": {0: None}}),
        "softmax": (L.octic_attnpool_softmax, [P, 8, 2, 5, 6, None], {"shape": {1: 4}, "align": {0: P + 8}, "null": {0: None}}),
        "pool": (L.octic_attnpool_pool, [P, 8, P, 128, 2, 5, 128, 6, P, None],
                 {"shape": {3: 64}, "align": {2: P + 4}, "null": {8: None}}),
        "value": (L.octic_attnpool_value, [P, P, P, 2, 3, 128, P, 384, None],
                  {"shape": {7: 256}, "align": {6: P + 4}, "null": {2: None}}),
        "dinput": (L.octic_attnpool_dinput, [P, P, 3, 2, 5, 128, 1.0, P, 384, None],
                   {"shape": {5: 100}, "align": {8: 386}, "null": {1: None}}),
        "dweight": (L.octic_attnpool_dweight, [P, P, 388, 0, 128, 3, 2, 5, 128, 1.0, P, None],
                    {"shape": {2: 300}, "align": {3: 2}, "null": {10: None}}),
        "colsum": (L.octic_attnpool_colsum, [P, 10, 5, 3, 2, 5, 1.0, P, None],
                   {"shape": {2: 4}, "align": {0: P + 4}, "null": {7: None}}),
        "dz": (L.octic_attnpool_dz, [P, 384, P, 2, 3, 128, P, None], {"shape": {4: 0}, "align": {6: P + 4}, "null": {2: None}}),
        "dwv": (L.octic_attnpool_dwv, [P, 384, P, 2, 3, 128, P, None], {"shape": {1: 128}, "align": {1: 386}, "null": {6: None}}),
        "dscores": (L.octic_attnpool_dscores, [P, 128, P, 2 * P, 8, 2, 5, 128, 6, P, None],
                    {"shape": {6: 0}, "align": {3: 2 * P + 4}, "null": {2: None}}),
        "unfold": (L.octic_attnpool_unfold, [P, P, P, 2, 128, P, P, P, None],
                   {"shape": {4: 32}, "align": {2: P + 4}, "null": {7: None}}),
    }


@pytest.mark.parametrize("name", ["fold", "softmax", "pool", "value", "dinput", "dweight", "colsum", "dz", "dwv", "dscores", "unfold"])
def test_entry_points_refuse_bad_arguments_without_a_device(name):
    fn, good, bad = _calls(_lib.lib())[name]
    for kind, code in (("shape", -1), ("align", -2), ("null", -4)):
        args = list(good)
        for pos, val in bad[kind].items():
            args[pos] = val
        assert fn(*args) == code, (name, kind)


def test_dscores_refuses_in_place_on_the_probabilities():
    L = _lib.lib()
    assert L.octic_attnpool_dscores(P, 128, P, P, 8, 2, 5, 128, 6, P, None) == -1
