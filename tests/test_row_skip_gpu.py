"""Backward row passes that skip the rows of samples a stochastic-depth mask drops (include/octic_hip.h:
octic_dense_layernorm_bwd_tail_skip, octic_layernorm_d8_bwd_skip / _cast_skip, octic_dense_colsum_skip; the SKIP instantiations
of dense_ln_bwd_tail_kernel, ln_bwd_g8_kernel<WIDE> and dense_colsum_kernel).

sample_scale[b] == 0 promises that the cotangent rows of sample b are zero; the kernel then leaves those rows of the cotangent,
of the stream and of the statistics unread.  The yardstick throughout is the UNMASKED launch of the same build on inputs that
keep the promise, compared with torch.equal (which does not see the sign of an exact zero - the only difference there is).
The masked launch gets NaN in every element it may not read, so a read shows up as a non-finite result.

1. the dense tail kernel: d = 256 / 1280 (NV 1 / 5), samples of 1, 3, 37 and 257 rows, with and without dres, with and without
   rs, masks for ns and rs in which all four row classes occur; dx, gyb and the four finished parameter gradients;
2. the octic kernel: c = 32 / 96 / 160, M = B x {3, 37, 257}, plain and with the scaled bf16 copy (with / without its row
   factors), with and without dres; dx, the copy, d alpha and d beta;
3. the column sums: d = 384 / 3840 inside wider rows, row counts that run the 16-row trip, the tail loop, or both;
4. the shape refusals;
5. a two-block standard step and a two-block octic step through train.Trainer with the switch on and off, eagerly and captured."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
KEEP = 2.0                       # 1 / keep at drop_path 0.5
NAN = float("nan")


def _mask_pairs(B):
    """name -> (ns, rs): the factors of the branch the norm opens / of the branch that ends in front of it."""
    alt = [KEEP * (b & 1) for b in range(B)]
    pairs = [KEEP * ((b >> 1) & 1) for b in range(B)]
    out = {"all kept": ([KEEP] * B, [KEEP] * B), "all dropped": ([0.0] * B, [0.0] * B),
           "four classes": (alt, pairs),                                  # b = 0..3: (0,0) (K,0) (0,K) (K,K)
           "four classes, swapped": (pairs, alt),
           "ns dropped, rs kept": ([0.0] * B, [KEEP] * B), "ns kept, rs dropped": ([KEEP] * B, [0.0] * B)}
    for s in (1, 2):
        g = torch.Generator().manual_seed(300 + s)
        draw = lambda: (torch.bernoulli(torch.full((B,), 0.5), generator=g) * KEEP).tolist()
        out[f"bernoulli {s}"] = (draw(), draw())
    return out


def _t(v):
    return torch.tensor(v, dtype=torch.float32, device=DEV)


def _dead_rows(mask, rps):
    return (_t(mask) == 0).repeat_interleave(rps)


def _poison(t, dead):
    """A copy of t with NaN in the rows `dead` marks."""
    p = t.clone()
    p[dead] = NAN
    return p


def _same(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        if b is None:
            assert a is None, (what, i)
            continue
        for u, v in zip(a if isinstance(a, (list, tuple)) else [a], b if isinstance(b, (list, tuple)) else [b]):
            assert bool(torch.isfinite(u.float()).all()), f"{what}: output {i} is not finite"
            assert torch.equal(u, v), f"{what}: output {i}, {int((u != v).sum())} elements differ"


# ---- 1: dense tail kernel ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tail_operands(B, rps, d):
    from octic_vits_amd import ops
    rows = B * rps
    g = torch.Generator(device=DEV).manual_seed(rows * 3 + d)
    r = lambda *s: torch.randn(*s, generator=g, device=DEV)
    x = r(rows, d) * 1.5 + 0.25
    w, gamma = r(d) * 0.5 + 1.0, r(d) * 0.1
    _, stats = ops.dense_layernorm_fwd(x, w, None, 1e-6, torch.bfloat16)
    return x, w, gamma, stats, r(rows, d).bfloat16(), r(rows, d), r(rows, d).bfloat16()


@pytest.mark.parametrize("B,rps", [(7, 1), (6, 3), (7, 37), (5, 257), (8, 257)])
@pytest.mark.parametrize("d", [256, 1280])
def test_dense_tail_equals_the_unmasked_launch(d, B, rps):
    """Row counts 7, 18, 259, 1285 and 2056: none a multiple of the 8 waves of a workgroup or of waves x grid (one slab per 16
    rows); at 2056 rows some waves walk a second row."""
    from octic_vits_amd import ops
    x, w, gamma, stats, gy, dres, yb = _tail_operands(B, rps, d)
    for name, (ns, rs) in _mask_pairs(B).items():
        dead_n, dead_r = _dead_rows(ns, rps), _dead_rows(rs, rps)
        gyz = gy * (~dead_n)[:, None].to(gy.dtype)                        # the promise: zero rows where ns is 0
        xp, gyp, sp, ybp = _poison(x, dead_n), _poison(gyz, dead_n), _poison(stats, dead_n), _poison(yb, dead_r)
        for dr in (dres, None):
            for rsv in ((_t(rs), None) if name.startswith("four classes") else (_t(rs),)):
                want = ops.dense_layernorm_bwd_tail(gyz, x, w, stats, dr, yb, gamma, rsv, rps)
                got = ops.dense_layernorm_bwd_tail(gyp, xp, w, sp, dr, ybp if rsv is not None else yb, gamma, rsv, rps,
                                                   sample_scale=_t(ns), rows_per_sample=rps)
                _same(got, want, f"{name}, dres {dr is not None}, rs {rsv is not None}")
                if dr is None and not any(ns):
                    assert int(torch.count_nonzero(got[0])) == 0, name       # dx = LN'(0) = 0


# ---- 2: octic kernel ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _octic_operands(B, T, c):
    from octic_vits_amd import ops
    g = torch.Generator(device=DEV).manual_seed(B * 1000 + T * 7 + c)
    r = lambda *s: torch.randn(*s, generator=g, device=DEV)
    x = r(B, T, 8 * c) * 2 + 0.3
    alpha = tuple(torch.rand(c if i < 4 else 2 * c, generator=g, device=DEV) + 0.5 for i in range(5))
    _, stats = ops.layernorm_fwd(x, list(alpha), None, 1e-5, torch.bfloat16, c)
    return x, alpha, stats, r(B, T, 8 * c).bfloat16(), r(B, T, 8 * c)


@pytest.mark.parametrize("B,T", [(6, 3), (7, 37), (5, 257)])
@pytest.mark.parametrize("c", [32, 64, 96, 128, 160])          # every chunk count of the masked kernel
def test_octic_layernorm_bwd_equals_the_unmasked_launch(c, B, T):
    from octic_vits_amd import ops
    x, alpha, stats, g, dres = _octic_operands(B, T, c)
    alpha = list(alpha)
    for name, (ns, rs) in _mask_pairs(B).items():
        dead = _dead_rows(ns, T).view(B, T)
        gz = g * (~dead)[..., None].to(g.dtype)
        xp, gp, sp = _poison(x, dead), _poison(gz, dead), _poison(stats.view(B, T, 8), dead).view(stats.shape)
        for dr in (dres, None):
            want = ops.layernorm_bwd(gz, x, stats, alpha, dr, c)
            got = ops.layernorm_bwd(gp, xp, sp, alpha, dr, c, sample_scale=_t(ns), rows_per_sample=T)
            _same(got, want, f"plain: {name}, dres {dr is not None}")
            for crs in (_t(rs), None):
                want = ops.layernorm_bwd_cast(gz, x, stats, alpha, dr, c, crs, T)
                got = ops.layernorm_bwd_cast(gp, xp, sp, alpha, dr, c, crs, T, sample_scale=_t(ns), rows_per_sample=T)
                _same(got, want, f"cast: {name}, dres {dr is not None}, crs {crs is not None}")


# ---- 3: column sums ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,rps", [(7, 1), (6, 37), (5, 257), (8, 600), (8, 512)])
@pytest.mark.parametrize("d,ld", [(384, 392), (3840, 3904)])
def test_colsum_equals_the_unmasked_launch(d, ld, B, rps):
    """256 row blocks of ceil(rows / 256) rows, four row phases each: 7 / 222 / 1285 rows run the tail loop alone (at most 6 rows
    per block), 4800 rows (19 per block) one 16-row trip and then the tail loop in phases 0-2, 4096 rows (16 per block) the
    trip alone."""
    from octic_vits_amd import ops
    rows = B * rps
    gen = torch.Generator(device=DEV).manual_seed(rows + d)
    g = torch.randn(rows, ld, generator=gen, device=DEV).bfloat16()
    for name, (ns, _) in _mask_pairs(B).items():
        dead = _dead_rows(ns, rps)
        gz = (g * (~dead)[:, None].to(g.dtype))
        want = ops.dense_colsum(gz[:, :d])
        got = ops.dense_colsum(_poison(gz, dead)[:, :d], _t(ns), rps)
        assert bool(torch.isfinite(got).all()), name
        assert torch.equal(got, want), f"{name}: {int((got != want).sum())} columns differ"
        if not any(ns):
            assert int(torch.count_nonzero(got)) == 0, name


# ---- 4: refusals ---------------------------------------------------------------------------------------------------------------
def test_a_mask_needs_whole_samples():
    """rows_per_sample <= 0, or rows that are no multiple of it, with a mask: OCTIC_ESHAPE (-1) from all four entry points."""
    from octic_vits_amd import ops
    B, T, c = 4, 6, 32
    x, alpha, stats, g, dres = _octic_operands(B, T, c)
    xd, w, gamma, sd, gy, dr, yb = _tail_operands(4, 6, 256)
    ss = _t([KEEP, 0.0, KEEP, 0.0])
    for bad in (0, -3, 5, 7):
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            ops.layernorm_bwd(g, x, stats, list(alpha), dres, c, sample_scale=ss, rows_per_sample=bad)
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            ops.layernorm_bwd_cast(g, x, stats, list(alpha), dres, c, None, T, sample_scale=ss, rows_per_sample=bad)
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            ops.dense_layernorm_bwd_tail(gy, xd, w, sd, dr, yb, gamma, None, 6, sample_scale=ss, rows_per_sample=bad)
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            ops.dense_colsum(gy, ss, bad)
    # and without a mask the same numbers are not looked at
    ops.dense_colsum(gy, None, 5)
    ops.dense_layernorm_bwd_tail(gy, xd, w, sd, dr, yb, gamma, None, 6, sample_scale=None, rows_per_sample=5)
    torch.cuda.synchronize()


# ---- 5: training steps ---------------------------------------------------------------------------------------------------------
def _standard_model():
    from functools import partial
    from octic_vits_amd.vit_models import vit_models
    torch.manual_seed(0)
    return vit_models(img_size=56, patch_size=14, embed_dim=256, depth=2, num_heads=4, num_classes=10, mlp_ratio=4,
                      qkv_bias=True, drop_path_rate=0.5, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6)).to(DEV)


def _octic_model():
    from octic_vits_amd.d8_layers import Layer_scale_init_BlockD8
    from octic_vits_amd.model import OcticVisionTransformer
    from octic_vits_amd.vit import Layer_scale_init_Block
    torch.manual_seed(0)
    return OcticVisionTransformer(octic_block_layers=Layer_scale_init_BlockD8, standard_block_layers=Layer_scale_init_Block,
                                  img_size=224, patch_size=14, num_classes=10, embed_dim=512, depth=3, num_heads=8,
                                  qkv_bias=True, init_scale=0.1, drop_path_rate=0.5, octic_equi_break_layer=2).cuda()


@pytest.fixture
def injected_masks():
    """The same device-resident masks in every forward of a run (a captured step replays what it recorded)."""
    import octic_vits_amd.d8_layers as L
    calls, cache = [0], {}
    for k in range(16):                                              # made up front: nothing may be created while a step is captured
        g = torch.Generator().manual_seed(900 + k)
        cache[k] = (torch.bernoulli(torch.full((4,), 0.5), generator=g) * KEEP).to(DEV)
    cache[0] = torch.tensor([KEEP, 0.0, 0.0, KEEP], device=DEV)
    cache[1] = torch.tensor([0.0, KEEP, 0.0, KEEP], device=DEV)      # (with cache[0]: all four row classes in the first block)

    def source(B, keep, device):
        k = calls[0] % 16
        calls[0] += 1
        return cache[k]

    L.drop_path_mask_source = source
    yield calls
    L.drop_path_mask_source = None


@pytest.fixture
def row_switch():
    import octic_vits_amd.functional as OF
    before = OF.ROW_SKIP_DROPPED
    yield OF
    OF.ROW_SKIP_DROPPED = before


def _count_masked_launches(monkeypatch):
    from octic_vits_amd import ops
    seen = {}
    for name in ("dense_layernorm_bwd_tail", "layernorm_bwd", "layernorm_bwd_cast", "dense_colsum"):
        seen[name] = 0

        def counting(*a, _inner=getattr(ops, name), _name=name, **k):
            masked = k.get("sample_scale") is not None or (_name == "dense_colsum" and len(a) > 1 and a[1] is not None)
            seen[_name] += masked
            return _inner(*a, **k)

        monkeypatch.setattr(ops, name, counting)
    return seen


def _run_both_ways(make_model, batch, img, captured, switch, seen, expect, reset=None):
    from octic_vits_amd.train import Trainer, synthetic_batch
    x, y = synthetic_batch(batch, 10, DEV, seed=3, img_size=img)
    results = []
    for on in (True, False):
        switch.ROW_SKIP_DROPPED = on
        if reset is not None:
            reset[0] = 0
        tr = Trainer(make_model(), lr=1e-3)
        torch.manual_seed(11)                                       # the drop-path masks come from the device generator
        for k in seen:
            seen[k] = 0
        if captured:
            loss = tr.capture(x, y, warmup=1).replay(x, y).detach().clone()
        else:
            loss = tr.step(x, y).detach().clone()
            assert seen == (expect if on else dict.fromkeys(expect, 0)), seen
        torch.cuda.synchronize()
        results.append((loss, {n: p.grad.detach().clone() for n, p in tr.raw_model.named_parameters() if p.grad is not None},
                        [p.detach().clone() for p in tr.raw_model.parameters()]))
    (la, ga, pa), (lb, gb, pb) = results
    assert torch.equal(la, lb) and bool(torch.isfinite(la).all())
    assert set(ga) == set(gb) and len(ga) > 20
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)


@pytest.mark.parametrize("captured", [False, True])
def test_standard_step_is_bitwise_with_and_without_skipping(captured, row_switch, monkeypatch):
    """Two standard blocks (D = 256, 4 heads, MLP 1024, drop_path 0.5), 8 images of 17 tokens, bf16 autocast through
    train.Trainer.  Masked per step: the three fused tail passes (norm2 of both blocks out of proj's tail, norm1 of the second
    block out of the first MLP's tail, handed over through `_octic_prenorm`) and the two qkv bias sums."""
    seen = _count_masked_launches(monkeypatch)
    expect = {"dense_layernorm_bwd_tail": 3, "layernorm_bwd": 0, "layernorm_bwd_cast": 0, "dense_colsum": 2}
    _run_both_ways(_standard_model, 8, 56, captured, row_switch, seen, expect)


@pytest.mark.parametrize("captured", [False, True])
def test_octic_step_is_bitwise_with_and_without_skipping(captured, injected_masks, row_switch, monkeypatch):
    """224 x 224 (T = 257), 4 images, two octic blocks and a standard one at embed_dim 512 (c = 64).  Masked per step: norm1 of
    the first octic block (its own node), norm2 of both and norm1 of the second (fused into the GEMM in front); in the standard
    block norm2's tail pass and the qkv bias sums (its norm1 follows the hand-off and has no tail in front)."""
    seen = _count_masked_launches(monkeypatch)
    expect = {"dense_layernorm_bwd_tail": 1, "layernorm_bwd": 1, "layernorm_bwd_cast": 3, "dense_colsum": 1}
    _run_both_ways(_octic_model, 4, 224, captured, row_switch, seen, expect, reset=injected_masks)
