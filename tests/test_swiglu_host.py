"""CPU-only: DINOv2's SwiGLU FFN (vit.SwiGLUFFN / SwiGLUFFNFused, ``ffn_layer="swiglu" | "swiglufused"``) and the ViT-g/14
factory - the hidden-width rule, state_dict keys and shapes, the f32 CPU forward against the reference's golden
(tests/golden/make_swiglu_golden.py), the plumbing the fused optimizer and the weight caches rely on, and the argument checks of
csrc/swiglu.hip's entry points before any launch.  No kernel runs."""
import ctypes

import numpy as np
import pytest
import torch

import swiglu_cases as SC


def _make(**kw):
    from octic_vits_amd.dinov2_vit import DinoVisionTransformer
    return DinoVisionTransformer(**kw)


@pytest.mark.parametrize("dim,hidden,H", [(128, 512, 344), (192, 768, 512), (1024, 4096, 2736), (1536, 6144, 4096)])
def test_hidden_width_rule(dim, hidden, H):
    """swiglu_ffn.py:66: (int(hidden * 2 / 3) + 7) // 8 * 8; the plain SwiGLUFFN keeps the width it is given."""
    from octic_vits_amd.vit import SwiGLUFFN, SwiGLUFFNFused
    with torch.device("meta"):
        f, p = SwiGLUFFNFused(dim, hidden), SwiGLUFFN(dim, hidden)
    assert tuple(f.w12.weight.shape) == (2 * H, dim) and tuple(f.w3.weight.shape) == (dim, H)
    assert tuple(f.w12.bias.shape) == (2 * H,) and tuple(f.w3.bias.shape) == (dim,)
    assert tuple(p.w12.weight.shape) == (2 * hidden, dim) and tuple(p.w3.weight.shape) == (dim, hidden)
    assert sorted(f.state_dict()) == ["w12.bias", "w12.weight", "w3.bias", "w3.weight"]
    assert f.fusable() and p.fusable()


def test_block_honours_ffn_layer_and_ffn_bias():
    from octic_vits_amd import vit
    with torch.device("meta"):
        swi = vit.NestedTensorBlock(dim=192, num_heads=3, ffn_layer=vit.SwiGLUFFNFused, init_values=1.0)
        nob = vit.NestedTensorBlock(dim=192, num_heads=3, ffn_layer=vit.SwiGLUFFNFused, ffn_bias=False)
        mlp = [vit.NestedTensorBlock(dim=192, num_heads=3, ffn_layer=f) for f in (None, vit.Mlp)]
    assert type(swi.mlp) is vit.SwiGLUFFNFused and tuple(swi.mlp.w12.weight.shape) == (1024, 192)
    assert nob.mlp.w12.bias is None and nob.mlp.w3.bias is None
    assert sorted(k for k in nob.state_dict() if k.startswith("mlp.")) == ["mlp.w12.weight", "mlp.w3.weight"]
    for b in mlp:                                     # None / Mlp: the block as it always was
        assert type(b.mlp) is vit.Mlp and sorted(k for k in b.state_dict() if k.startswith("mlp.")) == [
            "mlp.fc1.bias", "mlp.fc1.weight", "mlp.fc2.bias", "mlp.fc2.weight"]


def test_vit_giant2_layout_and_the_refusals_that_stay():
    from octic_vits_amd import deit_models, dinov2_vit, vit
    with torch.device("meta"):
        g = dinov2_vit.vit_giant2()
        hub = dinov2_vit.vit_giant2(patch_size=14, img_size=518, ffn_layer="swiglufused", init_values=1e-5, block_chunks=0)
        plain = dinov2_vit.vit_giant2(ffn_layer="mlp")
        s, b = dinov2_vit.vit_small(patch_size=14), dinov2_vit.vit_base(patch_size=14)
        alias = _make(embed_dim=192, depth=1, num_heads=3, ffn_layer="swiglu")
    assert len(g.blocks) == 40 and g.embed_dim == 1536
    blk = g.blocks[0]
    assert type(blk.mlp) is vit.SwiGLUFFNFused and blk.attn.num_heads == 24
    assert tuple(blk.mlp.w12.weight.shape) == (8192, 1536) and tuple(blk.mlp.w3.weight.shape) == (1536, 4096)
    assert sum(p.numel() for p in blk.parameters()) == 28_336_640 - 2 * 1536          # no init_values: no layer scales
    assert sum(p.numel() for p in hub.blocks[0].parameters()) == 28_336_640              # the published model's block
    assert type(hub.blocks[0].mlp) is vit.SwiGLUFFNFused and hub.patch_size == 14 and type(plain.blocks[0].mlp) is vit.Mlp
    assert (s.embed_dim, len(s.blocks), s.blocks[0].attn.num_heads) == (384, 12, 6)
    assert (b.embed_dim, len(b.blocks), b.blocks[0].attn.num_heads) == (768, 12, 12)
    assert type(s.blocks[0].mlp) is vit.Mlp                     # ffn_layer="mlp" stays the default
    assert type(alias.blocks[0].mlp) is vit.SwiGLUFFNFused      # "swiglu" builds the fused width too (vision_transformer.py:124)
    for name in ("vit_small", "vit_base", "vit_giant2"):
        assert name in deit_models._LOCAL_REGISTRY
    with pytest.raises(NotImplementedError):
        _make(embed_dim=64, depth=1, num_heads=2, ffn_layer="identity")
    with pytest.raises(NotImplementedError):
        _make(embed_dim=64, depth=1, num_heads=2, ffn_layer="swiglufused", block_chunks=4)
    with pytest.raises(NotImplementedError, match="embed_dim >= 128"):      # below the dense GEMMs' minimum width: still refused
        _make(embed_dim=64, depth=1, num_heads=2, ffn_layer="swiglufused")
    with torch.device("meta"):
        assert type(_make(embed_dim=128, depth=1, num_heads=2, ffn_layer="swiglufused").blocks[0].mlp) is vit.SwiGLUFFNFused
    with pytest.raises(RuntimeError):
        dinov2_vit.vit_giant2(pretrained=True)


@pytest.mark.parametrize("name", list(SC.CASES))
def test_f32_cpu_forward_matches_the_reference_golden(name):
    """Fails on a tree without the SwiGLU FFN with NotImplementedError.  The state_dict has the reference's keys and shapes
    (its sorted 'key:shape' list is part of the golden), so a reference checkpoint loads with strict=True; where the reference
    itself can be imported that load is made for real."""
    m = SC.build(_make, name)
    want = np.load(SC.GOLDEN)
    assert list(SC.state_keys(m)) == list(want[f"{name}.state_keys"])
    from _ref_import import reference_available
    if reference_available():
        import importlib
        from functools import partial
        from _ref_import import load_reference
        load_reference()
        vt = importlib.import_module("dinov2.models.vision_transformer")
        ref = SC.build(lambda **kw: vt.DinoVisionTransformer(block_fn=partial(vt.Block, attn_class=vt.MemEffAttention),
                                                             block_chunks=0, **kw), name)
        m2 = _make(**dict(SC.SPEC, **SC.CASES[name]))
        m2.load_state_dict(ref.state_dict(), strict=True)
        for (k, a), b in zip(m.state_dict().items(), m2.state_dict().values()):
            assert torch.equal(a, b), k
        m = m2.eval()
    got = SC.run_model(m, name)
    assert np.array_equal(got[f"{name}.img"], want[f"{name}.img"])
    SC.check_golden(got, tol=1e-3)


def test_eager_forward_is_the_reference_composition():
    from octic_vits_amd.vit import SwiGLUFFNFused
    import torch.nn.functional as F
    torch.manual_seed(0)
    f = SwiGLUFFNFused(64, 256)
    x = torch.randn(3, 5, 64)
    x1, x2 = F.linear(x, f.w12.weight, f.w12.bias).chunk(2, dim=-1)
    assert torch.equal(f(x), F.linear(F.silu(x1) * x2, f.w3.weight, f.w3.bias))


def test_optimizer_and_cache_plumbing_sees_the_swiglu_projections():
    from octic_vits_amd import functional as OF
    from octic_vits_amd import train
    m = _make(img_size=28, patch_size=14, embed_dim=192, depth=2, num_heads=3, ffn_layer="swiglufused")
    layers = train.library_gemm_layers(m)
    roles = [(r, tuple(lin.weight.shape)) for lin, _, r in layers]
    assert roles == [("qkv", (576, 192)), ("proj", (192, 192)), ("fc1", (1024, 192)), ("fc2", (192, 512))] * 2
    ffn = m.blocks[0].mlp
    assert layers[2][0] is ffn.w12 and layers[2][1] is ffn._c1 and layers[3][0] is ffn.w3 and layers[3][1] is ffn._c2
    ffn._c1.get(ffn.w12.weight, ffn.w12.bias, torch.bfloat16)
    assert ffn._c1.key is not None
    assert OF.invalidate_weight_caches(m) == 8 and ffn._c1.key is None


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """H % 8, a row stride off 8 elements or shorter than the row, a base pointer off 16 bytes, NULL operands; rows == 0 is a
    no-op.  (Fake addresses: nothing is dereferenced on these paths.)"""
    from octic_vits_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p
    a, b, c = 4096, 8192, 16384
    assert L.octic_swiglu_blocks() > 0
    assert set(_lib.header_symbols()) >= {"octic_swiglu_blocks", "octic_swiglu_fwd", "octic_swiglu_bwd"}
    assert L.octic_swiglu_fwd(p(a), 24, p(b), 12, 4, 12, None) == -1                   # H % 8
    assert L.octic_swiglu_fwd(p(a), 32, p(b), 16, 4, 0, None) == -1
    assert L.octic_swiglu_fwd(p(a), 24, p(b), 16, 4, 16, None) == -1                   # ld12 < 2H
    assert L.octic_swiglu_fwd(p(a), 32, p(b), 8, 4, 16, None) == -1                    # lda < H
    assert L.octic_swiglu_fwd(p(a), 33, p(b), 16, 4, 16, None) == -2                   # odd row stride
    assert L.octic_swiglu_fwd(p(a), 32, p(b), 20, 4, 16, None) == -2
    assert L.octic_swiglu_fwd(p(a + 2), 32, p(b), 16, 4, 16, None) == -2               # one element off
    assert L.octic_swiglu_fwd(p(a), 32, p(b + 2), 16, 4, 16, None) == -2
    assert L.octic_swiglu_fwd(None, 32, p(b), 16, 4, 16, None) == -4
    assert L.octic_swiglu_fwd(p(a), 32, None, 16, 4, 16, None) == -4
    assert L.octic_swiglu_fwd(None, 33, None, 3, 0, 12, None) == 0                     # rows == 0: nothing to do
    assert L.octic_swiglu_bwd(p(a), 24, p(b), 12, p(c), 24, None, 4, 12, None) == -1
    assert L.octic_swiglu_bwd(p(a), 32, p(b), 16, p(c), 24, None, 4, 16, None) == -1   # ldd < 2H
    assert L.octic_swiglu_bwd(p(a), 32, p(b), 8, p(c), 32, None, 4, 16, None) == -1    # ldg < H
    assert L.octic_swiglu_bwd(p(a), 32, p(b), 17, p(c), 32, None, 4, 16, None) == -2
    assert L.octic_swiglu_bwd(p(a), 32, p(b), 16, p(c), 36, None, 4, 16, None) == -2
    assert L.octic_swiglu_bwd(p(a), 32, p(b), 16, p(c + 2), 32, None, 4, 16, None) == -2
    assert L.octic_swiglu_bwd(p(a), 32, p(b + 2), 16, p(c), 32, None, 4, 16, None) == -2
    assert L.octic_swiglu_bwd(None, 32, p(b), 16, p(c), 32, None, 4, 16, None) == -4
    assert L.octic_swiglu_bwd(p(a), 32, None, 16, p(c), 32, None, 4, 16, None) == -4
    assert L.octic_swiglu_bwd(p(a), 32, p(b), 16, None, 32, None, 4, 16, None) == -4
    assert L.octic_swiglu_bwd(None, 0, None, 0, None, 0, None, 0, 16, None) == 0
    assert L.octic_swiglu_bwd(p(a), 32, p(b), 16, p(c), 32, None, -1, 16, None) == -1


def test_sigmoid_is_exactly_one_from_17_in_float32():
    """What the bitwise rounding checks of tests/test_swiglu_gpu.py rest on: 1 + exp(-x) == 1 in f32 for x >= 17."""
    assert np.float32(1.0) + np.exp(np.float32(-17.0)) == np.float32(1.0)
    assert np.float32(1.0) + np.exp(np.float32(-16.0)) != np.float32(1.0)


def test_ops_refuse_cpu_tensors():
    from octic_vits_amd import ops
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.swiglu_fwd(torch.zeros(2, 16, dtype=torch.bfloat16), 8)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.swiglu_bwd(torch.zeros(2, 16, dtype=torch.bfloat16), torch.zeros(2, 8, dtype=torch.bfloat16))
