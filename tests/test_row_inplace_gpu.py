"""Row kernels that move only the bytes a dropped sample needs (include/octic_hip.h: octic_dense_layernorm_bwd_tail_inplace,
octic_layernorm_d8_bwd_cast_inplace, octic_dense_resid_layernorm_fwd_skip; the INPLACE instantiations of
dense_ln_bwd_tail_kernel and ln_bwd_g8_kernel<WIDE>, the SKIPY instantiation of dense_resid_ln_fwd_kernel).

In place, dres and dx are one buffer: a live row is read and rewritten, a dead row (its sample dropped by the branch the norm
opens) is not written, and not read either where the branch that ended in front of the norm dropped the sample too.  The
yardstick throughout is the out-of-place masked launch of the same build on the same operands and masks; everything is compared
bit for bit or with torch.equal (which does not see the sign of an exact zero - the only difference there is).

1. the dense tail kernel, in place against out of place: d = 256 ... 1280 (one to five chunks, each a compilation of its own),
   samples of 1, 3 and 37 rows, row totals that are no multiple of the 16 waves of a slab, independent masks for the two branches;
2. the octic kernel, the same: c = 32 ... 160;
3. unread means unread: NaN in every element the contract leaves unread;
4. the forward instantiation against the plain launch;
5. ownership: the tensor a caller hands to `.backward(g)` comes back untouched, for standard and for octic blocks;
6. a one-octic, two-standard step through train.Trainer with the switch on and off, eagerly and captured."""
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
           "alternating": (alt, pairs),                                   # b = 0..3: (0,0) (K,0) (0,K) (K,K)
           "alternating, swapped": (pairs, alt),
           "ns dropped, rs kept": ([0.0] * B, [KEEP] * B), "ns kept, rs dropped": ([KEEP] * B, [0.0] * B)}
    for s in (1, 2):
        g = torch.Generator().manual_seed(500 + s)
        draw = lambda: (torch.bernoulli(torch.full((B,), 0.5), generator=g) * KEEP).tolist()
        out[f"bernoulli {s}"] = (draw(), draw())
    return out


def _t(v):
    return torch.tensor(v, dtype=torch.float32, device=DEV)


def _dead_rows(mask, rps):
    return (_t(mask) == 0).repeat_interleave(rps)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check_stream(buf, want_dx, dres, dead, what):
    """The shared buffer after the launch: live rows hold the out-of-place dx, dead rows the bits they came with."""
    got, want, src = _bits(buf).view(dead.numel(), -1), _bits(want_dx).view(dead.numel(), -1), _bits(dres).view(dead.numel(), -1)
    assert torch.equal(got[~dead], want[~dead]), f"{what}: live rows of dx differ from the out-of-place launch"
    assert torch.equal(got[dead], src[dead]), f"{what}: a dead row of the shared buffer was written"


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
    g = torch.Generator(device=DEV).manual_seed(rows * 5 + d)
    r = lambda *s: torch.randn(*s, generator=g, device=DEV)
    x = r(rows, d) * 1.5 + 0.25
    w, gamma = r(d) * 0.5 + 1.0, r(d) * 0.1
    _, stats = ops.dense_layernorm_fwd(x, w, None, 1e-6, torch.bfloat16)
    return x, w, gamma, stats, r(rows, d).bfloat16(), r(rows, d), r(rows, d).bfloat16()


TAIL_SHAPES = [(7, 1), (6, 3), (5, 37), (9, 37)]     # 7, 18, 185 and 333 rows: none a multiple of 16; 333 rows are 21 slabs


@pytest.mark.parametrize("B,rps", TAIL_SHAPES)
@pytest.mark.parametrize("d", [256, 512, 768, 1024, 1280])      # every chunk count: each is a compilation of its own
def test_dense_tail_in_place_equals_out_of_place(d, B, rps):
    from octic_vits_amd import ops
    x, w, gamma, stats, gy, dres, yb = _tail_operands(B, rps, d)
    for name, (ns, rs) in _mask_pairs(B).items():
        dead = _dead_rows(ns, rps)
        gyz = gy * (~dead)[:, None].to(gy.dtype)                          # the promise: zero rows where ns is 0
        for rsv in ((_t(rs), None) if name.startswith("alternating") else (_t(rs),)):
            want = ops.dense_layernorm_bwd_tail(gyz, x, w, stats, dres, yb, gamma, rsv, rps, sample_scale=_t(ns),
                                                rows_per_sample=rps)
            buf = dres.clone()
            got = ops.dense_layernorm_bwd_tail(gyz, x, w, stats, buf, yb, gamma, rsv, rps, sample_scale=_t(ns),
                                               rows_per_sample=rps, inplace=True)
            what = f"{name}, rs {rsv is not None}"
            assert got[0] is buf, what                                    # no dx was allocated
            _same(got[1:], want[1:], what)                                # dw, db, gyb, dgamma, column sums
            _check_stream(buf, want[0], dres, dead, what)


def test_in_place_needs_a_mask_and_an_owned_float32_buffer():
    from octic_vits_amd import ops
    x, w, gamma, stats, gy, dres, yb = _tail_operands(6, 3, 256)
    ss = _t([KEEP, 0.0] * 3)
    with pytest.raises(ValueError):
        ops.dense_layernorm_bwd_tail(gy, x, w, stats, dres.clone(), yb, gamma, None, 3, inplace=True)          # no mask
    with pytest.raises(ValueError):
        ops.dense_layernorm_bwd_tail(gy, x, w, stats, None, yb, gamma, None, 3, sample_scale=ss, rows_per_sample=3,
                                     inplace=True)                                                              # no dres
    xo, alpha, so, g, dro = _octic_operands(6, 3, 32)
    with pytest.raises(ValueError):
        ops.layernorm_bwd_cast(g, xo, so, list(alpha), dro.clone(), 32, None, 3, inplace=True)
    with pytest.raises(RuntimeError, match=r"\(-1\)"):                    # rows that are no whole samples: OCTIC_ESHAPE
        ops.dense_layernorm_bwd_tail(gy, x, w, stats, dres.clone(), yb, gamma, None, 3, sample_scale=ss, rows_per_sample=5,
                                     inplace=True)
    torch.cuda.synchronize()


# ---- 2: octic kernel ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _octic_operands(B, T, c):
    from octic_vits_amd import ops
    g = torch.Generator(device=DEV).manual_seed(B * 1000 + T * 11 + c)
    r = lambda *s: torch.randn(*s, generator=g, device=DEV)
    x = r(B, T, 8 * c) * 2 + 0.3
    alpha = tuple(torch.rand(c if i < 4 else 2 * c, generator=g, device=DEV) + 0.5 for i in range(5))
    _, stats = ops.layernorm_fwd(x, list(alpha), None, 1e-5, torch.bfloat16, c)
    return x, alpha, stats, r(B, T, 8 * c).bfloat16(), r(B, T, 8 * c)


@pytest.mark.parametrize("B,T", [(7, 1), (6, 3), (5, 37), (9, 37)])
@pytest.mark.parametrize("c", [32, 64, 96, 128, 160])           # every chunk count of the wide kernel
def test_octic_layernorm_bwd_cast_in_place_equals_out_of_place(c, B, T):
    from octic_vits_amd import ops
    x, alpha, stats, g, dres = _octic_operands(B, T, c)
    alpha = list(alpha)
    for name, (ns, rs) in _mask_pairs(B).items():
        dead = _dead_rows(ns, T)
        gz = g * (~dead).view(B, T, 1).to(g.dtype)
        for crs in ((_t(rs), None) if name.startswith("alternating") else (_t(rs),)):
            want = ops.layernorm_bwd_cast(gz, x, stats, alpha, dres, c, crs, T, sample_scale=_t(ns), rows_per_sample=T)
            buf = dres.clone()
            got = ops.layernorm_bwd_cast(gz, x, stats, alpha, buf, c, crs, T, sample_scale=_t(ns), rows_per_sample=T,
                                         inplace=True)
            what = f"{name}, crs {crs is not None}"
            assert got[0] is buf, what
            _same(got[1:], want[1:], what)                                # the five d alpha, d beta, the scaled bf16 copy
            _check_stream(buf, want[0], dres, dead, what)


# ---- 3: unread means unread ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,rps", [(6, 3), (5, 37)])
@pytest.mark.parametrize("d", [256, 1280])
def test_dense_tail_leaves_unread_what_the_contract_says(d, B, rps):
    """NaN in dres where both factors are 0 and in yb where rs is 0 (and, as before, in gy, x and stats where ns is 0): every
    other row and every parameter gradient equals the clean launch, the poisoned dres rows come back bit for bit."""
    from octic_vits_amd import ops
    x, w, gamma, stats, gy, dres, yb = _tail_operands(B, rps, d)
    for name, (ns, rs) in _mask_pairs(B).items():
        dead_n, dead_r = _dead_rows(ns, rps), _dead_rows(rs, rps)
        both = dead_n & dead_r
        gyz = gy * (~dead_n)[:, None].to(gy.dtype)
        clean = dres.clone()
        want = ops.dense_layernorm_bwd_tail(gyz, x, w, stats, clean, yb, gamma, _t(rs), rps, sample_scale=_t(ns),
                                            rows_per_sample=rps, inplace=True)
        xp, gyp, sp, ybp, buf = x.clone(), gyz.clone(), stats.clone(), yb.clone(), dres.clone()
        xp[dead_n], gyp[dead_n], sp[dead_n], ybp[dead_r], buf[both] = NAN, NAN, NAN, NAN, NAN
        before = _bits(buf).clone()
        got = ops.dense_layernorm_bwd_tail(gyp, xp, w, sp, buf, ybp, gamma, _t(rs), rps, sample_scale=_t(ns),
                                           rows_per_sample=rps, inplace=True)
        _same(got[1:], want[1:], name)
        assert torch.equal(_bits(buf)[both], before[both]), name
        assert torch.equal(_bits(buf)[~both], _bits(clean)[~both]), name
        assert bool(torch.isfinite(buf[~both]).all()), name


@pytest.mark.parametrize("B,T", [(6, 3), (5, 37)])
@pytest.mark.parametrize("c", [32, 160])
def test_octic_kernel_leaves_unread_what_the_contract_says(c, B, T):
    from octic_vits_amd import ops
    x, alpha, stats, g, dres = _octic_operands(B, T, c)
    alpha = list(alpha)
    for name, (ns, rs) in _mask_pairs(B).items():
        dead_n = _dead_rows(ns, T).view(B, T)
        both = dead_n & _dead_rows(rs, T).view(B, T)
        gz = g * (~dead_n)[..., None].to(g.dtype)
        clean = dres.clone()
        want = ops.layernorm_bwd_cast(gz, x, stats, alpha, clean, c, _t(rs), T, sample_scale=_t(ns), rows_per_sample=T,
                                      inplace=True)
        xp, gp, sp, buf = x.clone(), gz.clone(), stats.clone().view(B, T, 8), dres.clone()
        xp[dead_n], gp[dead_n], sp[dead_n], buf[both] = NAN, NAN, NAN, NAN
        before = _bits(buf).clone()
        got = ops.layernorm_bwd_cast(gp, xp, sp.view(stats.shape), alpha, buf, c, _t(rs), T, sample_scale=_t(ns),
                                     rows_per_sample=T, inplace=True)
        _same(got[1:], want[1:], name)
        assert torch.equal(_bits(buf)[both], before[both]), name
        assert torch.equal(_bits(buf)[~both], _bits(clean)[~both]), name
        assert bool(torch.isfinite(buf[~both]).all()), name


# ---- 4: forward ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fwd_operands(B, rps, d):
    rows = B * rps
    g = torch.Generator(device=DEV).manual_seed(rows * 13 + d)
    r = lambda *s: torch.randn(*s, generator=g, device=DEV)
    return r(rows, d) * 1.5 + 0.25, r(rows, d).bfloat16(), r(d) * 0.1, r(d) * 0.5 + 1.0, r(d) * 0.2


@pytest.mark.parametrize("B,rps", [(7, 1), (6, 3), (5, 37), (9, 37)])
@pytest.mark.parametrize("d", [256, 512, 1280, 320])            # whole chunks (all loads up front) and the predicated loop
def test_resid_layernorm_fwd_skip_equals_the_plain_launch(d, B, rps):
    """All kept: no branch is taken and xout, y and stats equal the plain launch bit for bit (a change of FMA contraction in the
    new instantiation would show here).  Mixed masks: equal as values, with NaN in the rows of yb that stay unread."""
    from octic_vits_amd import ops
    x, yb, gamma, w, b = _fwd_operands(B, rps, d)
    for name, (_, rs) in _mask_pairs(B).items():
        dead = _dead_rows(rs, rps)
        want = ops.dense_resid_layernorm_fwd(x, yb, gamma, _t(rs), rps, w, b, 1e-6, torch.bfloat16)
        got = ops.dense_resid_layernorm_fwd(x, yb, gamma, _t(rs), rps, w, b, 1e-6, torch.bfloat16, skip_yb=True)
        _same(got, want, name)
        if not bool(dead.any()):
            for u, v in zip(got, want):
                assert torch.equal(u.view(torch.int16 if u.dtype == torch.bfloat16 else torch.int32),
                                   v.view(torch.int16 if v.dtype == torch.bfloat16 else torch.int32)), name
        ybp = yb.clone()
        ybp[dead] = NAN
        _same(ops.dense_resid_layernorm_fwd(x, ybp, gamma, _t(rs), rps, w, b, 1e-6, torch.bfloat16, skip_yb=True), want,
              name + ", poisoned")
    # float32 branch and float32 result take the same instantiation family
    rs = _t(_mask_pairs(B)["alternating"][1])
    want = ops.dense_resid_layernorm_fwd(x, yb.float(), gamma, rs, rps, w, b, 1e-6, torch.float32)
    _same(ops.dense_resid_layernorm_fwd(x, yb.float(), gamma, rs, rps, w, b, 1e-6, torch.float32, skip_yb=True), want, "f32")


# ---- 5: ownership ------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def inplace_switch():
    import octic_vits_amd.functional as OF
    before = OF.ROW_INPLACE
    yield OF
    OF.ROW_INPLACE = before


def _count_inplace_launches(monkeypatch):
    from octic_vits_amd import ops
    seen = {}
    for name in ("dense_layernorm_bwd_tail", "layernorm_bwd_cast"):
        seen[name] = 0

        def counting(*a, _inner=getattr(ops, name), _name=name, **k):
            seen[_name] += bool(k.get("inplace"))
            return _inner(*a, **k)

        monkeypatch.setattr(ops, name, counting)
    return seen


def _backward_both_ways(run, params, g, OF, seen, name):
    """run() -> (output, input leaf).  Returns nothing; asserts that g survives and that the gradients do not depend on the
    switch."""
    res = {}
    for on in (True, False):
        OF.ROW_INPLACE = on
        for p in params:
            p.grad = None
        for k in seen:
            seen[k] = 0
        torch.manual_seed(21)                                             # the drop-path masks come from the device generator
        out, leaf = run()
        keep = g.clone()
        out.backward(g)
        torch.cuda.synchronize()
        assert torch.equal(_bits(g), _bits(keep)), f"the caller's cotangent was written (switch {on})"
        assert (seen[name] > 0) == on, (on, seen)                         # the path under test did run
        assert OF.STREAM_GRADS.storage is None                            # nothing is held past the end of the pass
        res[on] = [leaf.grad.clone()] + [p.grad.clone() for p in params if p.grad is not None]
    assert len(res[True]) == len(res[False]) > 10
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)


def test_standard_blocks_leave_the_callers_cotangent_alone(inplace_switch, monkeypatch):
    """Three chained standard blocks at drop_path 0.5.  The last block's MLP tail has no norm behind it and hands the caller's g
    on as its stream cotangent: the tail pass that receives it must not write into it.  The passes further up receive buffers
    the package allocated and do update them in place."""
    from octic_vits_amd.vit import Layer_scale_init_Block, link_blocks
    seen = _count_inplace_launches(monkeypatch)
    torch.manual_seed(0)
    blk = torch.nn.Sequential(*[Layer_scale_init_Block(dim=256, num_heads=4, qkv_bias=True, init_values=0.5, drop_path=0.5)
                                for _ in range(3)]).cuda().train()
    link_blocks(blk)                                                      # norm1 of the next block out of the MLP's tail
    x = torch.randn(6, 17, 256, device=DEV)
    g = torch.randn(6, 17, 256, device=DEV)

    def run():
        xi = x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return blk(xi), xi

    _backward_both_ways(run, list(blk.parameters()), g, inplace_switch, seen, "dense_layernorm_bwd_tail")


def test_octic_blocks_leave_the_callers_cotangent_alone(inplace_switch, monkeypatch):
    import octic_vits_amd.d8_layers as L
    import octic_vits_amd.functional as OF
    seen = _count_inplace_launches(monkeypatch)
    torch.manual_seed(5)
    dim = 8 * 32
    blocks = torch.nn.ModuleList([L.Layer_scale_init_BlockD8(dim, 4, drop_path=0.5, init_values=0.5) for _ in range(3)]).cuda()
    L.link_octic_blocks(blocks)
    blocks.train()
    x = torch.randn(6, 17, dim, device=DEV)
    g = torch.randn(6, 17, dim, device=DEV)

    def run():
        xi = x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            h = OF.Octic(xi, dim // 8)
            for b in blocks:
                h = b(h)
        return h.packed, xi

    _backward_both_ways(run, list(blocks.parameters()), g, inplace_switch, seen, "layernorm_bwd_cast")


# ---- 6: training step ------------------------------------------------------------------------------------------------------------
def _hybrid_model():
    from octic_vits_amd.d8_layers import Layer_scale_init_BlockD8
    from octic_vits_amd.model import OcticVisionTransformer
    from octic_vits_amd.vit import Layer_scale_init_Block
    torch.manual_seed(0)
    return OcticVisionTransformer(octic_block_layers=Layer_scale_init_BlockD8, standard_block_layers=Layer_scale_init_Block,
                                  img_size=224, patch_size=14, num_classes=10, embed_dim=512, depth=3, num_heads=8,
                                  qkv_bias=True, init_scale=0.1, drop_path_rate=0.5, octic_equi_break_layer=1).cuda()


@pytest.fixture
def injected_masks():
    """The same device-resident masks in every forward of a run (a captured step replays what it recorded)."""
    import octic_vits_amd.d8_layers as L
    calls, cache = [0], {}
    for k in range(16):                                              # made up front: nothing may be created while a step is captured
        g = torch.Generator().manual_seed(700 + k)
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


@pytest.mark.parametrize("captured", [False, True])
def test_train_step_is_bitwise_with_and_without_in_place_rows(captured, injected_masks, inplace_switch, monkeypatch):
    """224 x 224 (T = 257), 4 images, one octic block and two standard ones at embed_dim 512, drop_path 0.5, through
    train.Trainer: loss, every gradient and every parameter after the step do not depend on OCTIC_ROW_INPLACE."""
    from octic_vits_amd.train import Trainer, synthetic_batch
    seen = _count_inplace_launches(monkeypatch)
    x, y = synthetic_batch(4, 10, DEV, seed=3, img_size=224)
    results = []
    for on in (True, False):
        inplace_switch.ROW_INPLACE = on
        injected_masks[0] = 0
        tr = Trainer(_hybrid_model(), lr=1e-3)
        torch.manual_seed(11)
        for k in seen:
            seen[k] = 0
        if captured:
            loss = tr.capture(x, y, warmup=1).replay(x, y).detach().clone()
        else:
            loss = tr.step(x, y).detach().clone()
            assert (sum(seen.values()) > 0) == on, (on, seen)
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
