"""The linear depth head (csrc/depth.hip, octic_vits_amd/depth.py) without a GPU: the ABI additions, the acceptance query at the
edges of its range, the launchers' refusals before any launch (fake pointers, as test_koleo_host), the module's state-dict
keys, CenterPadding, the stock composition on CPU against the reference's numbers (tests/golden/depth_linear.npz), the hub
factories' tables and refusals, and non-strict checkpoint loading.

Bound of the golden comparison: the head sums 2 D layers products per logit in float32, so two correct float32 evaluations
differ by up to (2 D layers) 2^-24 relative to the largest depth; the backbone in front (4 tiny blocks, the same composition
op for op) adds less than that.  The issue's CPU measurement of the two summation orders (1.2e-5 .. 1.5e-5 at depths near 40)
sits inside it."""
import ctypes
import os
from functools import partial

import numpy as np
import pytest
import torch

import cases
import depth_cases as DC
from octic_vits_amd import _lib, depth, dinov2_vit, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "depth_linear.npz"))
NEW = ("octic_depth_ok", "octic_depth_plan", "octic_depth_logits", "octic_depth_expect")
P = 1 << 20                       # a fake, 16-byte aligned device address: nothing is launched on a refused call


def test_symbols_are_declared_exported_documented_and_the_abi_number_stays():
    L = _lib.lib()
    declared = _lib.header_symbols()
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in NEW:
        assert s in declared and s in _lib._PROTOS and hasattr(L, s) and s in text, s
    assert L.octic_abi_version() == _lib.ABI_VERSION == 20
    header = open(_lib.HEADER_PATH).read()
    assert "Arithmetic contract" in header[header.index("octic_depth_plan"):]


@pytest.mark.parametrize("D,layers,bins,u,want", [
    (64, 1, 256, 4, 1), (4096, 4, 256, 1, 1), (1024, 4, 256, 4, 1), (384, 1, 256, 2, 1), (1536, 4, 256, 4, 1),
    (0, 1, 256, 4, 0), (32, 1, 256, 4, 0), (96, 1, 256, 4, 0), (4160, 1, 256, 4, 0), (-64, 1, 256, 4, 0),
    (64, 0, 256, 4, 0), (64, 5, 256, 4, 0), (64, 4, 128, 4, 0), (64, 4, 255, 4, 0), (64, 4, 512, 4, 0),
    (64, 4, 256, 0, 0), (64, 4, 256, 3, 0), (64, 4, 256, 8, 0), (64, 4, 256, -1, 0),
])
def test_depth_ok_at_the_edges_of_the_range(D, layers, bins, u, want):
    assert _lib.lib().octic_depth_ok(D, layers, bins, u) == want
    assert ops.depth_head_ok(D, layers, bins, u) is bool(want)


def test_plan_names_the_tile_and_refuses_what_the_launchers_refuse():
    tile, groups, chains, blocks = ops.depth_plan(3, 37, 37, 1024, 4)
    assert tile >= 16 and groups == 3 * -(-37 * 37 // tile) and chains == 4 * 1024 // 64 and blocks >= 1
    assert ops.depth_plan(1, 1, 1, 64, 1, 256, 1) == (tile, 1, 1, 1)
    for bad in ((0, 3, 3, 64, 1), (1, 0, 3, 64, 1), (1, 3, 0, 64, 1), (1, 3, 3, 96, 1), (1, 3, 3, 64, 5), (1, 3, 3, 64, 1, 128),
                (1, 3, 3, 64, 1, 256, 3), (1, 1 << 15, 1 << 15, 64, 1, 256, 4), (1 << 31, 1, 1, 64, 1)):
        assert ops.depth_plan(*bad) is None, bad


def _arr(kind, vals):
    a = kind()
    for i, v in enumerate(vals):
        a[i] = v
    return a


def _logits(patch=(P,), ldb=(640,), ldr=(64,), cls=(P,), cls_ldb=(640,), layers=1, B=2, h=3, w=3, D=64, W=P, bias=P, bins=256,
            image_bias=P, Lo=P):
    return _lib.lib().octic_depth_logits(_arr(_lib.PtrArray4, patch), _arr(_lib.I64Array4, ldb), _arr(_lib.I64Array4, ldr),
                                         _arr(_lib.PtrArray4, cls), _arr(_lib.I64Array4, cls_ldb), layers, B, h, w, D, W, bias,
                                         bins, image_bias, Lo, None)


def _expect(Lo=P, B=2, h=3, w=3, bins_n=256, u=4, bins=P, depth=P):
    return _lib.lib().octic_depth_expect(Lo, B, h, w, bins_n, u, bins, 0.001, 80.0, depth, None)


def test_launchers_refuse_before_any_launch():
    for kw in (dict(D=96), dict(D=0), dict(D=4160), dict(layers=0), dict(layers=5), dict(bins=128), dict(B=0), dict(h=0), dict(w=0),
               dict(ldr=(60,)), dict(ldb=(-640,)), dict(cls_ldb=(-640,))):
        assert _logits(**kw) == -1, kw
    for kw in (dict(patch=(P + 4,)), dict(cls=(P + 8,)), dict(ldb=(642,)), dict(ldr=(66,)), dict(cls_ldb=(641,)), dict(W=P + 4),
               dict(Lo=P + 4)):
        assert _logits(**kw) == -2, kw
    for kw in (dict(patch=(None,)), dict(cls=(None,)), dict(W=None), dict(bias=None), dict(image_bias=None), dict(Lo=None)):
        assert _logits(**kw) == -4, kw
    assert _logits(layers=2, patch=(P, None), ldb=(640, 640), ldr=(64, 64), cls=(P, P), cls_ldb=(640, 640)) == -4
    for kw in (dict(bins_n=128), dict(u=3), dict(u=0), dict(u=8), dict(B=0), dict(h=0), dict(w=0), dict(h=1 << 15, w=1 << 15)):
        assert _expect(**kw) == -1, kw
    for kw in (dict(Lo=P + 4), dict(bins=P + 4), dict(depth=P + 2)):
        assert _expect(**kw) == -2, kw
    for kw in (dict(Lo=None), dict(bins=None), dict(depth=None)):
        assert _expect(**kw) == -4, kw


def test_ops_refuse_cpu_tensors_and_wrong_operands():
    p, c = torch.zeros(2, 9, 64), torch.zeros(2, 64)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.depth_logits([(p, c)], torch.zeros(256, 128), torch.zeros(256), (3, 3))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.depth_expect(torch.zeros(2, 9, 256), (3, 3), 4, torch.zeros(256), 0.001, 80.0)
    with pytest.raises(ValueError, match="1 to 4 layers"):
        ops.depth_logits([], torch.zeros(256, 128), torch.zeros(256), (3, 3))


def test_state_dict_keys_and_shapes():
    head = depth._linear_depth_head(64, 4)
    sd = head.state_dict()
    assert sorted(sd) == ["conv_depth.bias", "conv_depth.weight"]
    assert tuple(sd["conv_depth.weight"].shape) == (256, 512, 1, 1) and tuple(sd["conv_depth.bias"].shape) == (256,)
    assert (head.min_depth, head.max_depth, head.upsample, head.in_index) == (0.001, 80, 4, [0, 1, 2, 3])
    one = depth._linear_depth_head(64, 1)
    assert tuple(one.conv_depth.weight.shape) == (256, 128, 1, 1) and one.in_index == [0]
    reg = depth.BNHead(in_channels=[8], channels=8, in_index=[0], max_depth=10)
    assert tuple(reg.conv_depth.weight.shape) == (1, 8, 1, 1)
    model = _model(4)
    assert {k for k in model.state_dict() if not k.startswith("backbone.")} == {"decode_head.conv_depth.weight",
                                                                                "decode_head.conv_depth.bias"}


@pytest.mark.parametrize("size", [1, 13, 14, 15])
def test_center_padding_pads_as_the_reference(size):
    x = torch.arange(1.0, 1 + 2 * size * (size + 1)).reshape(1, 2, size, size + 1)
    assert np.array_equal(depth.CenterPadding(14)(x).numpy(), GOLD[f"pad.{size}"])


def _backbone():
    m = dinov2_vit.DinoVisionTransformer(block_fn=partial(dinov2_vit.Block, attn_class=dinov2_vit.MemEffAttention), block_chunks=0,
                                         **DC.SPEC)
    return cases.fill_parameters(m, salt=DC.SALT)


def _model(layers):
    model = depth.linear_depther(_backbone(), layers=layers, out_index=DC.OUT_INDEX[layers]).eval()
    w, b = GOLD[f"L{layers}.conv_depth.weight"], GOLD[f"L{layers}.conv_depth.bias"]
    missing, unexpected = depth.load_head_state_dict(model, {"decode_head.conv_depth.weight": torch.from_numpy(w.astype(np.float32)),
                                                             "decode_head.conv_depth.bias": torch.from_numpy(b.astype(np.float32))})
    assert not unexpected and all(k.startswith("backbone.") for k in missing)
    return model


def _bound(layers, want):
    return 2 * DC.SPEC["embed_dim"] * layers * 2.0 ** -24 * float(np.abs(want).max())


@pytest.mark.parametrize("layers", [4, 1])
def test_cpu_composition_reproduces_the_reference(layers):
    got = DC.run(_model(layers), layers)
    for name, have in got.items():
        want = GOLD[name]
        assert have.shape == want.shape, name
        err = float(np.abs(have.astype(np.float64) - want).max())
        print(f"{name}: max |err| {err:.3e}, bound {_bound(layers, want):.3e}")
        assert err <= _bound(layers, want), name


def test_forward_on_nchw_pairs_is_forward_tokens_on_cpu():
    torch.manual_seed(0)
    head = depth._linear_depth_head(64, 4).eval()
    pairs = [(torch.randn(2, 12, 64), torch.randn(2, 64)) for _ in range(4)]
    maps = [(p.reshape(2, 3, 4, 64).permute(0, 3, 1, 2).contiguous(), c) for p, c in pairs]
    with torch.no_grad():
        assert not head.kernels_take(pairs)
        a, b = head.forward(maps), head.forward_tokens(pairs, (3, 4))
    assert tuple(a.shape) == (2, 1, 12, 16) and torch.equal(a.clamp(0.001, 80), b)


@pytest.mark.parametrize("kw", [dict(norm_strategy="softmax"), dict(norm_strategy="sigmoid"), dict(bins_strategy="SID", max_depth=1.5),
                                dict(classify=False), dict(classify=False, scale_up=True), dict(align_corners=True),
                                dict(upsample=3), dict(n_bins=128)])
def test_stock_composition_covers_the_other_options(kw):
    """Each option against the formula written out in float64."""
    torch.manual_seed(1)
    args = dict(classify=True, n_bins=256, upsample=2, in_channels=[8, 8], in_index=[0, 1], channels=32, min_depth=0.001,
                max_depth=80.0)
    args.update(kw)
    head = depth.BNHead(**args).eval().double()
    maps = [(torch.randn(2, 8, 3, 5, dtype=torch.float64), torch.randn(2, 8, dtype=torch.float64)) for _ in range(2)]
    with torch.no_grad():
        got = head(maps)
        u = args["upsample"]
        feat = torch.cat([torch.nn.functional.interpolate(torch.cat((x, c[:, :, None, None].expand_as(x)), 1), size=(3 * u, 5 * u),
                                                          mode="bilinear", align_corners=args.get("align_corners", False))
                          for x, c in maps], 1)
        logit = torch.einsum("bchw,kc->bkhw", feat, head.conv_depth.weight[:, :, 0, 0]) + head.conv_depth.bias[None, :, None, None]
        if not args["classify"]:
            want = torch.sigmoid(logit) * 80.0 if args.get("scale_up") else torch.relu(logit) + 0.001
        else:
            n = args["n_bins"]
            bins = (torch.logspace(0.001, 1.5, n) if args.get("bins_strategy") == "SID" else torch.linspace(0.001, 80.0, n)).double()
            norm = args.get("norm_strategy", "linear")
            z = torch.relu(logit) + 0.1 if norm == "linear" else torch.exp(logit) if norm == "softmax" else torch.sigmoid(logit)
            want = ((z / z.sum(1, keepdim=True)) * bins[None, :, None, None]).sum(1, keepdim=True)
    assert tuple(got.shape) == (2, 1, 3 * u, 5 * u)
    assert float((got - want).abs().max()) <= 1e-9 * float(want.abs().max())


def test_factories_tables_and_refusals(monkeypatch):
    built = {}

    def fake(name):
        def make(**kw):
            built[name] = kw
            m = _backbone()
            m.blocks = torch.nn.ModuleList([torch.nn.Identity() for _ in range(depth.LAYER_COUNT[name])])
            return m
        return make

    for name in depth.LAYER_COUNT:
        monkeypatch.setattr(dinov2_vit, name, fake(name))
    want4 = {"vit_small": [2, 5, 8, 11], "vit_base": [2, 5, 8, 11], "vit_large": [4, 11, 17, 23], "vit_giant2": [9, 19, 29, 39]}
    last = {"vit_small": 11, "vit_base": 11, "vit_large": 23, "vit_giant2": 39}
    for fn, name in ((depth.dinov2_vits14_ld, "vit_small"), (depth.dinov2_vitb14_ld, "vit_base"),
                     (depth.dinov2_vitl14_ld, "vit_large"), (depth.dinov2_vitg14_ld, "vit_giant2")):
        m = fn()
        assert m.features == dict(n=want4[name], return_class_token=True, norm=False) and m.pad.multiple == 14
        assert built[name]["patch_size"] == 14 and built[name]["img_size"] == 518 and built[name]["init_values"] == 1.0
        assert (m.decode_head.min_depth, m.decode_head.max_depth, m.decode_head.upsample) == (0.001, 80, 4)
        assert fn(layers=1, weights="KITTI", depth_range=(0.001, 10.0)).features["n"] == [last[name]]
        assert fn(layers=1).decode_head.max_depth == 80
        with pytest.raises(AssertionError, match="Unsupported number of layers: 3"):
            fn(layers=3)
        with pytest.raises(AssertionError, match="Unsupported weights"):
            fn(weights="SUN")
        with pytest.raises(RuntimeError, match="no pretrained weights"):
            fn(pretrained=True)
    assert built["vit_giant2"]["ffn_layer"] == "swiglufused"
    with pytest.raises(AssertionError, match="Unsupported number of layers"):
        depth.linear_depther(_backbone(), layers=2)
    assert depth.linear_depther(_backbone(), layers=4).features["n"] == [0, 1, 2, 3]
    assert depth.linear_depther(_backbone(), layers=1).features["n"] == [3]


def test_slide_needs_its_sizes_and_training_is_refused():
    model = _model(1)
    x = DC.image()
    with pytest.raises(ValueError, match="stride and crop_size"):
        model.inference(x, [DC.meta()] * 2, True, mode="slide")
    with pytest.raises(ValueError, match="stride and crop_size"):
        model.inference(x, [DC.meta()] * 2, True, mode="slide", stride=DC.STRIDE)
    with torch.no_grad():
        a = model.inference(x, [DC.meta()] * 2, True, mode="slide", stride=(30, 45), crop_size=(30, 45))
        assert torch.equal(a, model.inference(x, [DC.meta()] * 2, True))
        flipped = model.inference(x, [DC.meta(True)] * 2, True)
        assert torch.equal(flipped, a.flip(3))
        assert torch.equal(model.forward_dummy(x), a)
        one = model([x], [[DC.meta()] * 2])
        assert isinstance(one, list) and len(one) == 2 and np.array_equal(np.stack(one), a.numpy())
    for call in (lambda: model.forward_train(x, None, None), lambda: model.train_step({}, None), lambda: model.losses(None, None),
                 lambda: model(x, None, return_loss=True), lambda: model.decode_head.forward_train(x, None, None, None),
                 lambda: model.decode_head.losses(None, None)):
        with pytest.raises(NotImplementedError, match=r"loss_decode=\(\)"):
            call()
    with pytest.raises(TypeError, match="must be a list"):
        model.forward_test(x, [[DC.meta()]])
    with pytest.raises(ValueError, match="num of augmentations"):
        model.forward_test([x], [[DC.meta()], [DC.meta()]])


@pytest.mark.parametrize("wrapped", [False, True])
def test_checkpoints_load_non_strictly_with_and_without_the_wrapper(wrapped):
    model = depth.linear_depther(_backbone(), layers=1)
    w, b = DC.head_weights(1)
    state = {"decode_head.conv_depth.weight": w, "decode_head.conv_depth.bias": b, "decode_head.extra": torch.zeros(1)}
    res = depth.load_head_state_dict(model, {"state_dict": state, "meta": {}} if wrapped else state)
    assert res.unexpected_keys == ["decode_head.extra"] and all(k.startswith("backbone.") for k in res.missing_keys)
    assert torch.equal(model.decode_head.conv_depth.weight, w) and torch.equal(model.decode_head.conv_depth.bias, b)
