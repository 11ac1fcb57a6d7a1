"""The linear depth head on the GPU: csrc/depth.hip through ops.depth_logits / ops.depth_expect and octic_vits_amd/depth.py.

Bounds.
* Logits with small-integer operands are exact in float32 (|sum| <= 2 D layers 12 < 2^24): bit for bit against int64.
* Expectation from planted logits against float64: per bin a bilinear blend (3 products, 3 sums) and relu + 0.1f, then two sums
  of 256 positive terms and one division, every step rounded once - below 2 (256 + 8) 2^-24 relative to the largest depth.
* Whole head against float64 in the reference's order (resize the features, then project): the rule of
  tests/test_koleo_gpu.py::_bound - the larger of twice the stock float32 arm's own error on the same device and inputs (the two
  arms round sums of equal length in different orders) and (2 D layers) 2^-24 relative to the largest depth.  Both errors are
  printed.
* Engine arm against stock arm where no float64 value exists (the octic backbone): each is within (2 D layers) 2^-24 of the exact
  value of its own features, so they are within twice that of each other."""
import os
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cases
import depth_cases as DC

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINS = 256


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _tile():
    """Patch rows per workgroup of the logits launch, from the plan query (host-only: it is asked at collection too)."""
    from octic_vits_amd import ops
    return ops.depth_plan(1, 1, 1, 64, 1, BINS, 1)[0]


def _grid_of(n):
    """(h, w) with h w == n, as square as it goes."""
    h = max(d for d in range(1, int(n ** 0.5) + 1) if n % d == 0)
    return h, n // h


def _blocks(B, R, n, D, layers, seed, integer=False):
    """Block outputs [B, 1 + R + n, D] per layer and their (patch rows, class token) views."""
    g = _gen(seed)
    outs = []
    for _ in range(layers):
        t = torch.randint(-4, 5, (B, 1 + R + n, D), generator=g).float() if integer else torch.randn(B, 1 + R + n, D, generator=g)
        outs.append(t.to(DEV))
    return outs, [(o[:, 1 + R:], o[:, 0]) for o in outs]


# ------------------------------------------------------------------------------------------------ logits, exact
def _logit_cases():
    T = _tile()
    return [(64, 1, 1, 0, 1), (64, 1, 2, 0, T - 1), (64, 2, 3, 4, T), (64, 4, 2, 0, T + 1), (128, 1, 3, 4, T + 1), (128, 2, 1, 0, T),
            (128, 4, 3, 0, T - 1), (384, 1, 2, 4, T - 1), (384, 2, 2, 0, 1), (384, 4, 2, 4, T + 1), (64, 4, 3, 4, 2 * T + 1)]


@pytest.mark.parametrize("D,layers,B,R,n", _logit_cases())
def test_logits_are_exact_on_integer_operands(D, layers, B, R, n):
    from octic_vits_amd import ops
    h, w = _grid_of(n)
    outs, pairs = _blocks(B, R, n, D, layers, 100 + D + layers + n, integer=True)
    g = _gen(7 + D)
    W = torch.randint(-3, 4, (BINS, 2 * D * layers), generator=g)
    bias = torch.randint(-9, 10, (BINS,), generator=g)
    Lo = ops.depth_logits(pairs, W.float().to(DEV), bias.float().to(DEV), (h, w))
    assert Lo.shape == (B, n, BINS) and Lo.dtype == torch.float32
    want = bias[None, None, :].expand(B, n, BINS).clone()
    for l, o in enumerate(outs):
        o64 = o.cpu().long()
        Wp, Wc = W[:, 2 * D * l:2 * D * l + D], W[:, 2 * D * l + D:2 * D * (l + 1)]
        want += o64[:, 1 + R:] @ Wp.T + (o64[:, 0] @ Wc.T)[:, None, :]
    assert int(want.abs().max()) < 2 ** 24
    # class tokens differ per image and n is off the tile: a tile that straddles two images cannot give this
    assert B == 1 or not torch.equal(outs[0][0, 0], outs[0][1, 0])
    assert torch.equal(Lo.cpu().long(), want) and torch.equal(Lo.cpu(), want.float())


# ------------------------------------------------------------------------------------------------ expectation
def _expect64(Lo, h, w, u, bins, lo, hi):
    """F.interpolate + depth_pred + clamp in float64 from patch-level logits [B, h w, 256]."""
    B = Lo.shape[0]
    x = Lo.double().reshape(B, h, w, BINS).permute(0, 3, 1, 2)
    x = F.interpolate(x, size=(u * h, u * w), mode="bilinear", align_corners=False)
    z = torch.relu(x) + 0.1
    z = z / z.sum(dim=1, keepdim=True)
    return torch.einsum("ikmn,k->imn", z, bins.double()).unsqueeze(1).clamp(lo, hi)


@pytest.mark.parametrize("u", [1, 2, 4])
@pytest.mark.parametrize("h,w", [(1, 1), (1, 2), (2, 1), (2, 3), (3, 5), (5, 3)])
def test_expectation_geometry_from_planted_logits(h, w, u):
    from octic_vits_amd import ops
    B = 2
    Lo = torch.zeros(B, h * w, BINS)
    for b in range(B):
        for c in range(h * w):                                   # one hot bin per cell, a different bin for every cell
            Lo[b, c, (37 * c + 5 + 101 * b) % BINS] = 40.0 + 3.0 * c + b
            Lo[b, c, (37 * c + 6 + 101 * b) % BINS] = -7.0       # and one negative logit, for the relu
    Lo = Lo.to(DEV)
    bins = torch.linspace(0.001, 80, BINS, device=DEV)
    got = ops.depth_expect(Lo, (h, w), u, bins, 0.001, 80.0)
    want = _expect64(Lo, h, w, u, bins, 0.001, 80.0)
    assert got.shape == (B, 1, u * h, u * w) and got.dtype == torch.float32
    err = float((got.double() - want).abs().max())
    bound = 2 * (BINS + 8) * 2.0 ** -24 * float(want.abs().max())
    print(f"grid {h}x{w} u={u}: max |err| {err:.3e}, bound {bound:.3e}, depth range [{float(want.min()):.3f}, {float(want.max()):.3f}]")
    assert float(want.max()) - float(want.min()) > 1.0 or h * w == 1      # the planted cells are told apart
    assert err <= bound


def test_clamp_holds_the_range_and_nan_passes():
    from octic_vits_amd import ops
    Lo = torch.randn(1, 6, BINS, generator=_gen(3)).to(DEV)
    for value, want in ((100.0, 80.0), (-5.0, 0.001), (0.0, 0.001)):
        bins = torch.full((BINS,), value, device=DEV)
        got = ops.depth_expect(Lo, (2, 3), 4, bins, 0.001, 80.0)
        assert torch.equal(got, torch.full_like(got, want)), value
    Lo[0, 0, 17] = float("nan")
    got = ops.depth_expect(Lo, (2, 3), 4, torch.linspace(0.001, 80, BINS, device=DEV), 0.001, 80.0)
    assert bool(got[0, 0, 0, 0].isnan()) and not bool(got[0, 0, -1, -1].isnan())


# ------------------------------------------------------------------------------------------------ whole head
def _head(D, layers, u=4, **kw):
    from octic_vits_amd import depth
    args = dict(classify=True, n_bins=BINS, upsample=u, in_channels=[D] * layers, in_index=list(range(layers)),
                channels=2 * D * layers, min_depth=0.001, max_depth=80)
    args.update(kw)
    head = depth.BNHead(**args).eval()
    g = _gen(11 + D + layers)
    with torch.no_grad():
        head.conv_depth.weight.copy_(torch.randn(head.conv_depth.weight.shape, generator=g) * (2.0 / args["channels"] ** 0.5))
        head.conv_depth.bias.copy_(torch.randn(head.conv_depth.bias.shape, generator=g) * 0.5)
    return head.to(DEV)


@torch.no_grad()
def _head64(head, pairs, h, w):
    """The reference's order in float64: class token as channels, resize the features, concatenate, project, depth_pred."""
    u = head.upsample
    feats = []
    for i in head.in_index:
        p, c = pairs[i]
        B, _, D = p.shape
        x = p.double().reshape(B, h, w, D).permute(0, 3, 1, 2)
        x = torch.cat((x, c.double()[:, :, None, None].expand_as(x)), 1)
        feats.append(F.interpolate(x, size=(u * h, u * w), mode="bilinear", align_corners=head.align_corners))
    feat = torch.cat(feats, 1)
    Wt = head.conv_depth.weight.double()[:, :, 0, 0]
    logit = torch.einsum("bchw,kc->bkhw", feat, Wt) + head.conv_depth.bias.double()[None, :, None, None]
    if head.norm_strategy == "softmax":
        z = torch.softmax(logit, dim=1)
    else:
        z = torch.relu(logit) + 0.1
        z = z / z.sum(dim=1, keepdim=True)
    bins = torch.linspace(head.min_depth, head.max_depth, head.n_bins, device=logit.device).double()
    return torch.einsum("ikmn,k->imn", z, bins).unsqueeze(1).clamp(head.min_depth, head.max_depth)


def _arms(head, pairs, grid):
    """(engine arm, stock arm, launches of the logits kernel by the engine arm)."""
    from octic_vits_amd import depth, ops
    calls = []
    real = ops.depth_logits

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    ops.depth_logits = counted
    try:
        with torch.no_grad():
            got = head.forward_tokens(pairs, grid)
            n = len(calls)
            depth.DEPTH_HIP = False
            stock = head.forward_tokens(pairs, grid)
            assert len(calls) == n
    finally:
        depth.DEPTH_HIP = True
        ops.depth_logits = real
    return got, stock, n


def _bound(stock, ref, channels):
    return max(2.0 * float((stock.double() - ref).abs().max()), channels * 2.0 ** -24 * float(ref.abs().max()))


@pytest.mark.parametrize("D,layers,B,R,h,w,u", [(64, 4, 2, 0, 3, 5, 4), (384, 1, 1, 4, 12, 11, 4), (128, 4, 3, 0, 1, 1, 2),
                                                (64, 2, 2, 4, 2, 7, 1), (128, 1, 2, 0, 5, 3, 4)])
def test_whole_head_against_float64_in_the_reference_order(D, layers, B, R, h, w, u):
    head = _head(D, layers, u)
    _, pairs = _blocks(B, R, h * w, D, layers, 500 + D + layers)
    got, stock, n = _arms(head, pairs, (h, w))
    with torch.no_grad():
        assert n == 1 and head.kernels_take(pairs)
    ref = _head64(head, pairs, h, w)
    assert got.shape == stock.shape == ref.shape == (B, 1, u * h, u * w)
    e_hip, e_stock = float((got.double() - ref).abs().max()), float((stock.double() - ref).abs().max())
    bound = _bound(stock, ref, 2 * D * layers)
    print(f"D={D} layers={layers} grid {h}x{w} u={u}: engine {e_hip:.3e}, stock {e_stock:.3e}, bound {bound:.3e}, "
          f"depth [{float(ref.min()):.3f}, {float(ref.max()):.3f}]")
    assert e_hip <= bound
    # forward on the NCHW pairs is the stock arm before its clamp
    maps = [(p.reshape(B, h, w, D).permute(0, 3, 1, 2).contiguous(), c) for p, c in pairs]
    with torch.no_grad():
        assert torch.equal(head(maps).clamp(0.001, 80), stock)


def test_invariances_are_bitwise():
    from octic_vits_amd import depth
    D, layers, R, h, w = 64, 4, 4, 3, 5
    head = _head(D, layers)
    outs, pairs = _blocks(3, R, h * w, D, layers, 900)
    with torch.no_grad():
        a = head.forward_tokens(pairs, (h, w))
        assert torch.equal(a, head.forward_tokens(pairs, (h, w)))                                  # two calls
        order = [2, 0]                                                                             # batch mates and position
        moved = head.forward_tokens([(o[order][:, 1 + R:], o[order][:, 0]) for o in outs], (h, w))
        assert torch.equal(moved, a[order])
        alone = head.forward_tokens([(o[1:2, 1 + R:], o[1:2, 0]) for o in outs], (h, w))           # a sliced batch, in place
        assert torch.equal(alone, a[1:2])
        dense = head.forward_tokens([(p.contiguous(), c.contiguous()) for p, c in pairs], (h, w))  # strided views = copies
        assert torch.equal(dense, a)
        twice = [torch.cat((o, o), 0)[::2] for o in outs]                                          # images 0, 2, 1: batch stride 2 T D
        every_other = head.forward_tokens([(o[:, 1 + R:], o[:, 0]) for o in twice], (h, w))
        assert torch.equal(every_other, torch.stack([a[0], a[2], a[1]]))
        for o in outs:
            o[1] = float("nan")
        sick = head.forward_tokens(pairs, (h, w))
        assert bool(sick[1].isnan().all()) and torch.equal(sick[0], a[0]) and torch.equal(sick[2], a[2])
    assert depth.DEPTH_HIP


# ------------------------------------------------------------------------------------------------ module level
def _dino_model(layers):
    from octic_vits_amd import depth, dinov2_vit
    gold = np.load(os.path.join(ROOT, "tests", "golden", "depth_linear.npz"))
    m = dinov2_vit.DinoVisionTransformer(block_fn=partial(dinov2_vit.Block, attn_class=dinov2_vit.MemEffAttention), block_chunks=0,
                                         **DC.SPEC)
    cases.fill_parameters(m, salt=DC.SALT)
    model = depth.linear_depther(m, layers=layers, out_index=DC.OUT_INDEX[layers]).eval()
    depth.load_head_state_dict(model, {"state_dict": {
        "decode_head.conv_depth.weight": torch.from_numpy(gold[f"L{layers}.conv_depth.weight"].astype(np.float32)),
        "decode_head.conv_depth.bias": torch.from_numpy(gold[f"L{layers}.conv_depth.bias"].astype(np.float32))}})
    return model.to(DEV), gold


class _OnDevice:
    """depth_cases.run feeds CPU images: the model under test with its inputs moved to the GPU."""

    def __init__(self, model):
        self.m = model

    def whole_inference(self, x, *a, **k):
        return self.m.whole_inference(x.to(DEV), *a, **k)

    def slide_inference(self, x, *a, **k):
        return self.m.slide_inference(x.to(DEV), *a, **k)

    def aug_test(self, xs, *a, **k):
        return self.m.aug_test([x.to(DEV) for x in xs], *a, **k)

    def simple_test(self, x, *a, **k):
        return self.m.simple_test(x.to(DEV), *a, **k)


@pytest.mark.parametrize("layers", [4, 1])
def test_golden_cases_through_linear_depther(layers):
    """whole / sized / flipped aug_test / slide_inference / simple_test of the reference, engine arm and stock arm."""
    from octic_vits_amd import depth, ops
    model, gold = _dino_model(layers)
    calls = []
    real = ops.depth_expect
    ops.depth_expect = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        got = DC.run(_OnDevice(model), layers)
        n = len(calls)
        depth.DEPTH_HIP = False
        stock = DC.run(_OnDevice(model), layers)
        assert len(calls) == n and n >= 2
    finally:
        depth.DEPTH_HIP = True
        ops.depth_expect = real
    for name, have in got.items():
        want = gold[name].astype(np.float64)
        e_hip, e_stock = float(np.abs(have - want).max()), float(np.abs(stock[name] - want).max())
        bound = max(2.0 * e_stock, 2 * DC.SPEC["embed_dim"] * layers * 2.0 ** -24 * float(np.abs(want).max()))
        print(f"{name}: engine {e_hip:.3e}, stock {e_stock:.3e}, bound {bound:.3e}")
        assert have.shape == want.shape and e_hip <= bound, name


def test_octic_backbone_against_its_own_stock_arm():
    from octic_vits_amd import depth, dinov2_models
    m = dinov2_models._dinov2(4, 128, 10, 4, False, 0, dict(img_size=32))
    cases.fill_parameters(m, salt="depth.octic.")
    model = depth.linear_depther(m, layers=4, out_index=[6, 7, 8, 9]).eval()
    head = _head(128, 4)
    model.decode_head.load_state_dict(head.state_dict())
    model = model.to(DEV)
    x = cases.randn("depth.octic.img", 2, 3, 30, 29).to(DEV)
    with torch.no_grad():
        feats = model.extract_feat(x, reshape=False)
        assert model.decode_head.kernels_take(feats) and tuple(feats[0][0].shape) == (2, 64, 128)
        got = model.whole_inference(x, None, True)
        raw = model.whole_inference(x, None, False)
        depth.DEPTH_HIP = False
        try:
            stock, stock_raw = model.whole_inference(x, None, True), model.whole_inference(x, None, False)
        finally:
            depth.DEPTH_HIP = True
    assert got.shape == (2, 1, 30, 29) and raw.shape == (2, 1, 32, 32)
    bound = 2 * 1024 * 2.0 ** -24 * float(stock_raw.abs().max())
    for a, b in ((got, stock), (raw, stock_raw)):
        err = float((a - b).abs().max())
        print(f"octic: engine against stock {err:.3e}, bound {bound:.3e}, depth [{float(b.min()):.3f}, {float(b.max()):.3f}]")
        assert err <= bound
    assert float(stock_raw.max() - stock_raw.min()) > 1e-2


@pytest.mark.parametrize("case", ["cpu", "softmax", "bins128", "switch", "upsample3", "align_corners"])
def test_routing_takes_the_stock_arm_and_still_matches(case):
    from octic_vits_amd import depth, ops
    D, layers, h, w = 64, 2, 3, 4
    kw = {"softmax": dict(norm_strategy="softmax"), "bins128": dict(n_bins=128), "upsample3": dict(u=3),
          "align_corners": dict(align_corners=True)}.get(case, {})
    head = _head(D, layers, **kw)
    _, pairs = _blocks(2, 0, h * w, D, layers, 77)
    if case == "cpu":
        head, pairs = head.cpu(), [(p.cpu(), c.cpu()) for p, c in pairs]
    calls = []
    real = ops.depth_logits
    ops.depth_logits = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    depth.DEPTH_HIP = case != "switch"
    try:
        with torch.no_grad():
            assert not head.kernels_take(pairs)
            got = head.forward_tokens(pairs, (h, w))
    finally:
        depth.DEPTH_HIP = True
        ops.depth_logits = real
    assert not calls
    ref = _head64(head, pairs, h, w)
    err = float((got.double() - ref).abs().max())
    bound = 4 * 2 * D * layers * 2.0 ** -24 * float(ref.abs().max())       # one float32 evaluation: sums, resize, normalisation
    print(f"{case}: stock arm {err:.3e}, bound {bound:.3e}")
    assert got.shape == ref.shape and err <= bound


def test_bf16_tokens_are_cast_in_front_of_the_head():
    head = _head(64, 4)
    _, pairs = _blocks(2, 4, 12, 64, 4, 31)
    half = [(p.bfloat16(), c.bfloat16()) for p, c in pairs]
    with torch.no_grad():
        got, stock, n = _arms(head, half, (3, 4))
        want = head.forward_tokens([(p.float(), c.float()) for p, c in half], (3, 4))
    assert n == 1 and got.dtype == stock.dtype == torch.float32 and torch.equal(got, want)
    assert float((got - stock).abs().max()) <= 2 * 512 * 2.0 ** -24 * float(stock.abs().max())
