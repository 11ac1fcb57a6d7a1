"""Standard DeiT-III ViT (``vit_models``, deit/vit.py:256-392) on the HIP engine: the baseline the octic hybrids are
measured against (experiments/complexity.py:19-28).  Same constructor keywords, ``state_dict`` keys, shapes and init as
the reference, so its checkpoints load unchanged.

Forward on the GPU = the octic models' own kernels without the octic half: the patch embedding is ONE lift GEMM
(functional.LiftFn: im2col + GEMM against ``proj.weight`` viewed as [D, Cin p p], bias + positional embedding + class row in
the epilogue), then ``vit.Layer_scale_init_Block``s linked for the next-norm fusion (vit.link_blocks), then the final norm
and the head (ATen, as in the hybrids)."""
from functools import partial

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import functional as OF
from .functional import compute_dtype
from .vit import Layer_scale_init_Block, Attention, Mlp, link_blocks


def trunc_normal_(tensor, mean=0., std=1., a=-2., b=2.):
    return nn.init.trunc_normal_(tensor, mean=mean, std=std, a=a, b=b)


def _2tuple(x):
    return tuple(x) if isinstance(x, (tuple, list)) else (x, x)


class PatchEmbed(nn.Module):
    """timm's / dinov2's PatchEmbed (Conv2d patch projection, keys ``proj.weight`` [D, Cin, p, p] and ``proj.bias``).

    ``tokens`` is the engine path: on the GPU the convolution is the lift GEMM of the octic models (im2col columns in
    Conv2d's (c, kh, kw) order, K = Cin p p padded to a multiple of 8) with bias, positional rows and class row fused into
    its epilogue; on the CPU it is the stock convolution."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768, norm_layer=None, flatten_embedding=True):
        super().__init__()
        self.img_size = _2tuple(img_size)
        self.patch_size = _2tuple(patch_size)
        if self.patch_size[0] != self.patch_size[1]:
            raise NotImplementedError("PatchEmbed: square patches only")
        self.grid_size = (self.img_size[0] // self.patch_size[0], self.img_size[1] // self.patch_size[1])
        self.num_patches = self.grid_size[0] * self.grid_size[1]
        self.in_chans, self.embed_dim = in_chans, embed_dim
        self.flatten_embedding = flatten_embedding
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=self.patch_size, stride=self.patch_size)
        self.norm = norm_layer(embed_dim) if norm_layer else nn.Identity()

    def _check(self, x):
        _, _, H, W = x.shape
        p = self.patch_size[0]
        if H % p or W % p:
            raise ValueError(f"PatchEmbed: input {H}x{W} is not a multiple of the patch size {p}")

    def tokens(self, x, pos=None, cls_row=None):
        """[B, (1+)G*G, D] f32: proj(x) flattened, + pos [G*G, D] on the patch rows, cls_row [D] as row 0."""
        self._check(x)
        if not isinstance(self.norm, nn.Identity):
            raise NotImplementedError("PatchEmbed.tokens: a norm after the projection is not fused")
        p = self.patch_size[0]
        D = self.proj.out_channels
        w = self.proj.weight.view(D, -1)
        if x.is_cuda:
            if torch.compiler.is_compiling():
                from . import dispatch as _D   # noqa: F401
                return torch.ops.octic.lift(x, w, self.proj.bias, pos, cls_row, p, compute_dtype(x) == torch.bfloat16)[0]
            return OF.LiftFn.apply(x, w, self.proj.bias, pos, cls_row, p, compute_dtype(x))
        t = self.proj(x).flatten(2).transpose(1, 2)
        if pos is not None:
            t = t + pos
        if cls_row is not None:
            t = torch.cat((cls_row.to(t.dtype).expand(t.shape[0], 1, -1), t), dim=1)
        return t

    def forward(self, x):
        self._check(x)
        x = self.proj(x)
        if not self.flatten_embedding:
            return self.norm(x)
        return self.norm(x.flatten(2).transpose(1, 2))


class vit_models(nn.Module):
    """deit/vit.py:256-392 with the engine's blocks (``block_layers`` defaults to vit.Layer_scale_init_Block, the block of
    every ``_LS`` factory)."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=1000, embed_dim=768, depth=12, num_heads=12,
                 mlp_ratio=4., qkv_bias=False, qk_scale=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.,
                 norm_layer=nn.LayerNorm, global_pool=None, block_layers=Layer_scale_init_Block, Patch_layer=PatchEmbed,
                 act_layer=nn.GELU, Attention_block=Attention, Mlp_block=Mlp, dpr_constant=True, init_scale=1e-4,
                 use_fused_attn=True, **kwargs):
        super().__init__()
        self.dropout_rate = drop_rate
        self.num_classes = num_classes
        self.num_features = self.embed_dim = embed_dim
        self.patch_embed = Patch_layer(img_size=img_size, patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim)
        num_patches = self.patch_embed.num_patches
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, num_patches, embed_dim))
        dpr = [drop_path_rate for _ in range(depth)]
        self.blocks = nn.ModuleList([
            block_layers(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale,
                         drop=0.0, attn_drop=attn_drop_rate, drop_path=dpr[i], norm_layer=norm_layer, act_layer=act_layer,
                         Attention_block=Attention_block, Mlp_block=Mlp_block, init_values=init_scale,
                         use_fused_attn=use_fused_attn)
            for i in range(depth)])
        self.norm = norm_layer(embed_dim)
        self.feature_info = [dict(num_chs=embed_dim, reduction=0, module='head')]
        self.head = nn.Linear(embed_dim, num_classes) if num_classes > 0 else nn.Identity()
        link_blocks(self.blocks)                     # residual add + next norm1 as one row pass, across the whole stack
        # (the glue code reads the octic / standard split: a baseline is all standard blocks)
        self.octic_equi_break_layer = 0
        self.invariant = False
        self.global_pool = False
        trunc_normal_(self.pos_embed, std=.02)
        trunc_normal_(self.cls_token, std=.02)
        self.apply(self._init_weights)

    def _init_weights(self, m):
        if isinstance(m, nn.Linear):
            trunc_normal_(m.weight, std=.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    @torch.jit.ignore
    def no_weight_decay(self):
        base_names = ['pos_embed', 'cls_token']
        return set(base_names + [f'_orig_mod.{name}' for name in base_names])

    def get_classifier(self):
        return self.head

    def get_num_layers(self):
        return len(self.blocks)

    def reset_classifier(self, num_classes, global_pool=''):
        self.num_classes = num_classes
        self.head = nn.Linear(self.embed_dim, num_classes) if num_classes > 0 else nn.Identity()

    def invalidate_weight_caches(self):
        """See functional.invalidate_weight_caches (optimizers that write ``p.data`` behind the version counters)."""
        return OF.invalidate_weight_caches(self)

    def forward_features(self, x):
        from .d8_layers import arm_drop_path_pool
        _, _, H, W = x.shape
        if (H, W) != tuple(self.patch_embed.img_size):
            # the reference adds pos_embed without interpolation (deit/vit.py:371) and fails on the shape mismatch
            raise ValueError(f"vit_models: input {H}x{W} differs from the native resolution "
                             f"{self.patch_embed.img_size[0]}x{self.patch_embed.img_size[1]} (no position interpolation)")
        arm_drop_path_pool(True)
        try:
            # deit/vit.py:365-380: position on the patch tokens only, then the class token in front - both in the lift epilogue
            x = self.patch_embed.tokens(x, self.pos_embed[0], self.cls_token.flatten())
            for blk in self.blocks:
                x = blk(x)
        finally:
            arm_drop_path_pool(False)
        from . import d8_layers as _L
        if _L.COMPACT_DROP_PATH:
            return self.norm(x[:, 0])                # (row-wise norm: the class rows alone, model.py's opt-in shortcut)
        return self.norm(x)[:, 0]

    def forward(self, x):
        x = self.forward_features(x)
        if self.dropout_rate:
            x = F.dropout(x, p=float(self.dropout_rate), training=self.training)
        return self.head(x)


def _deit_ls(pretrained, img_size, patch_size, embed_dim, depth, num_heads, kwargs):
    if pretrained:
        raise RuntimeError("no pretrained weights are bundled (load a reference checkpoint with load_state_dict)")
    kwargs.pop("pretrained_21k", None)
    return vit_models(img_size=img_size, patch_size=patch_size, embed_dim=embed_dim, depth=depth, num_heads=num_heads,
                      mlp_ratio=4, qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6),
                      block_layers=Layer_scale_init_Block, **kwargs)


# DeiT III: Revenge of the ViT (deit/vit.py:396-546), the regular `_LS` models
def deit_tiny_patch16_LS(pretrained=False, img_size=224, **kwargs):
    return _deit_ls(pretrained, img_size, 16, 192, 12, 3, kwargs)


def deit_small_patch16_LS(pretrained=False, img_size=224, **kwargs):
    return _deit_ls(pretrained, img_size, 16, 384, 12, 6, kwargs)


def deit_medium_patch16_LS(pretrained=False, img_size=224, **kwargs):
    return _deit_ls(pretrained, img_size, 16, 512, 12, 8, kwargs)


def deit_base_patch16_LS(pretrained=False, img_size=224, **kwargs):
    return _deit_ls(pretrained, img_size, 16, 768, 12, 12, kwargs)


def deit_large_patch16_LS(pretrained=False, img_size=224, **kwargs):
    return _deit_ls(pretrained, img_size, 16, 1024, 24, 16, kwargs)


def deit_huge_patch14_LS(pretrained=False, img_size=224, **kwargs):
    return _deit_ls(pretrained, img_size, 14, 1280, 32, 16, kwargs)


LS_FACTORIES = (deit_tiny_patch16_LS, deit_small_patch16_LS, deit_medium_patch16_LS, deit_base_patch16_LS,
                deit_large_patch16_LS, deit_huge_patch14_LS)
