"""The standard DINOv2 ViT (``DinoVisionTransformer``, dinov2/models/vision_transformer.py:43-339) on the HIP engine: the
baseline of the octic DINOv2 models, ``vit_large`` / ``vit_huge`` (:342-367) next to ``hybrid_vit_large`` /
``hybrid_vit_huge`` (configs train/vitl16.yaml, train/vith16.yaml).  Same constructor keywords, methods, output
dictionaries and ``state_dict`` keys as the reference for ``ffn_layer="mlp"`` / ``"swiglu"`` / ``"swiglufused"`` (the
SwiGLU FFN of ViT-g/14: vit.SwiGLUFFNFused) and ``block_chunks=0``.

Token assembly follows ``dinov2_models.OcticDinoVisionTransformer.prepare_tokens_with_masks``: without masks or register
tokens everything (bias, positional rows, class row + class position) is fused into the lift GEMM's epilogue; otherwise the
lift runs without position, then the mask ``where``, the position and the ``cat``.  The blocks are ``vit.NestedTensorBlock``
(layer scale, batch-subset stochastic depth); a list of crop sets runs as ONE row tensor (ragged.py)."""
import math
from functools import partial
from typing import Sequence, Union

import torch
import torch.nn as nn

from . import functional as OF
from .deit_models import register_model
from .vit import MemEffAttention, NestedTensorBlock as Block
from .vit_models import PatchEmbed, trunc_normal_

_RESIZE = {}


def _resize_matrix(M, w0, h0, kwargs, device):
    """interpolate_pos_encoding's bicubic resize of an [M, M] grid as one [w0 h0, M M] matrix: pushing the identity through
    F.interpolate with the reference's own arguments (the scale factor, when interpolate_offset is set, moves the sample
    positions) gives exactly the weights it applies; the resize is then one GEMM on the position table."""
    key = (M, w0, h0, tuple(sorted((k, tuple(v) if isinstance(v, tuple) else v) for k, v in kwargs.items())), str(device))
    m = _RESIZE.get(key)
    if m is None:
        with torch.no_grad():
            eye = torch.eye(M * M, dtype=torch.float32).view(M * M, 1, M, M)
            m = nn.functional.interpolate(eye, mode="bicubic", **kwargs)
            assert (w0, h0) == m.shape[-2:]
            m = m.reshape(M * M, w0 * h0).t().contiguous().to(device)
        if len(_RESIZE) > 32:
            _RESIZE.clear()
        _RESIZE[key] = m
    return m


class DinoVisionTransformer(nn.Module):
    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4.0,
                 qkv_bias=True, ffn_bias=True, proj_bias=True, drop_path_rate=0.0, drop_path_uniform=False,
                 init_values=None, embed_layer=PatchEmbed, act_layer=nn.GELU, block_fn=Block, ffn_layer="mlp",
                 block_chunks=0, num_register_tokens=0, interpolate_antialias=False, interpolate_offset=0.1):
        super().__init__()
        if ffn_layer in ("swiglu", "swiglufused"):          # vision_transformer.py:124-126: both names build the fused width
            if embed_dim < 128:
                # ops.dense_gemm_ok wants N >= 128 and K >= 128: below that width none of the FFN's four GEMMs (K = embed_dim
                # forward of w12 and backward of w3, N = embed_dim the other way) can run on csrc/dense_gemm.hip in either
                # direction, and no config is that narrow - such a model stays refused, as before the SwiGLU FFN existed
                raise NotImplementedError(f"DinoVisionTransformer: ffn_layer={ffn_layer!r} needs embed_dim >= 128 (got "
                                          f"{embed_dim}): narrower, no GEMM of the FFN fits the engine's dense kernels")
            from .vit import SwiGLUFFNFused
            block_fn = partial(block_fn, ffn_layer=SwiGLUFFNFused)
        elif ffn_layer != "mlp":
            raise NotImplementedError(f"DinoVisionTransformer: ffn_layer={ffn_layer!r} (only 'mlp', 'swiglu' and "
                                      "'swiglufused' run on the engine)")
        if block_chunks > 0:
            raise NotImplementedError("DinoVisionTransformer: block_chunks > 0 (FSDP chunking) is not supported")
        norm_layer = partial(nn.LayerNorm, eps=1e-6)
        self.num_features = self.embed_dim = embed_dim
        self.num_tokens = 1
        self.n_blocks = depth
        self.num_heads = num_heads
        self.patch_size = patch_size
        self.num_register_tokens = num_register_tokens
        self.interpolate_antialias = interpolate_antialias
        self.interpolate_offset = interpolate_offset
        self.patch_embed = embed_layer(img_size=img_size, patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim)
        num_patches = self.patch_embed.num_patches
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, num_patches + self.num_tokens, embed_dim))
        assert num_register_tokens >= 0
        self.register_tokens = (nn.Parameter(torch.zeros(1, num_register_tokens, embed_dim))
                                if num_register_tokens else None)
        if drop_path_uniform is True:
            dpr = [drop_path_rate] * depth
        else:
            dpr = [x.item() for x in torch.linspace(0, drop_path_rate, depth, device="cpu")]   # stochastic depth decay rule
        self.chunked_blocks = False
        self.blocks = nn.ModuleList([
            block_fn(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, proj_bias=proj_bias,
                     ffn_bias=ffn_bias, drop_path=dpr[i], norm_layer=norm_layer, act_layer=act_layer, init_values=init_values)
            for i in range(depth)])
        self.norm = norm_layer(embed_dim)
        self.head = nn.Identity()
        self.mask_token = nn.Parameter(torch.zeros(1, embed_dim))
        # (the glue code reads the octic / standard split: a baseline is all standard blocks)
        self.octic_equi_break_layer = 0
        self.invariant = False
        self.init_weights()

    def init_weights(self):
        trunc_normal_(self.pos_embed, std=0.02)
        nn.init.normal_(self.cls_token, std=1e-6)
        if self.register_tokens is not None:
            nn.init.normal_(self.register_tokens, std=1e-6)
        for m in self.modules():                      # named_apply(init_weights_vit_timm): Linear layers only
            if isinstance(m, nn.Linear):
                trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    # ------------------------------------------------------------------------------------------ tokens
    def interpolate_pos_encoding(self, x, w, h):
        """vision_transformer.py:181-214 for x = the [B, 1 + n, D] tokens of a (w, h) input: [1, 1 + n', D]."""
        previous_dtype = x.dtype
        npatch = x.shape[1] - 1
        N = self.pos_embed.shape[1] - 1
        if npatch == N and w == h:
            return self.pos_embed
        pos = self._pos_rows(w, h)
        return pos.unsqueeze(0).to(previous_dtype)

    def _pos_rows(self, w, h):
        """The (interpolated) position table as [1 + w0 h0, D] f32 rows: class position first."""
        pos_embed = self.pos_embed.float()[0]
        N = pos_embed.shape[0] - 1
        w0, h0 = w // self.patch_size, h // self.patch_size
        if w0 * h0 == N and w == h:
            return pos_embed
        M = int(math.sqrt(N))
        assert N == M * M
        if self.interpolate_offset:
            # (the reference's historical offset: the scale factor, not the size, sets the bicubic sample positions)
            kwargs = {"scale_factor": (float(w0 + self.interpolate_offset) / M, float(h0 + self.interpolate_offset) / M)}
        else:
            kwargs = {"size": (w0, h0)}
        if self.interpolate_antialias:
            kwargs["antialias"] = True
        r = _resize_matrix(M, w0, h0, kwargs, pos_embed.device)
        with torch.autocast(pos_embed.device.type, enabled=False):      # f32, as F.interpolate on .float() computes it
            return torch.cat((pos_embed[:1], r @ pos_embed[1:]), dim=0)

    def prepare_tokens_with_masks(self, x, masks=None):
        """[B, 1 + registers + n, D] f32 token rows (vision_transformer.py:216-235)."""
        B, _, w, h = x.shape
        pos = self._pos_rows(w, h)
        cls_row = self.cls_token.flatten() + pos[0]
        if masks is None and self.register_tokens is None:
            return self.patch_embed.tokens(x, pos[1:], cls_row)           # everything fused in the lift epilogue
        tok = self.patch_embed.tokens(x)                                  # [B, n, D] f32: proj + bias only
        if masks is not None:
            tok = torch.where(masks.unsqueeze(-1), self.mask_token.to(tok.dtype).unsqueeze(0), tok)
        tok = tok + pos[1:].to(tok.dtype)
        rows = [cls_row.to(tok.dtype).expand(B, 1, -1)]
        if self.register_tokens is not None:
            rows.append(self.register_tokens.to(tok.dtype).expand(B, -1, -1))
        return torch.cat(rows + [tok], dim=1).contiguous()

    def _out(self, x_norm, x, masks):
        r = self.num_register_tokens
        return {"x_norm_clstoken": x_norm[:, 0], "x_norm_regtokens": x_norm[:, 1:r + 1],
                "x_norm_patchtokens": x_norm[:, r + 1:], "x_prenorm": x, "masks": masks}

    # ------------------------------------------------------------------------------------------ forward
    def forward_features_list(self, x_list, masks_list):
        xs = [self.prepare_tokens_with_masks(x, m) for x, m in zip(x_list, masks_list)]
        # (ssl.SSLTrainer: gradients of block parameters may be written at the END of backward only if every block module
        # contributed one gradient - true for the one-row-tensor pass, false for the set-by-set loop)
        self._single_use_pass = False
        from . import dinov2_models
        if dinov2_models.RAGGED_LISTS and self._ragged_ok(xs):
            self._single_use_pass = True
            return self._forward_features_ragged(xs, masks_list)
        from . import ops
        if ops.GRAD_DEST is not None and torch.is_grad_enabled():
            # a gradient reducer hands each weight ONE destination per pass; the set-by-set loop launches two weight
            # gradients per block weight into it (ADVICE: the second overwrites the first) - never take that combination
            raise RuntimeError("DinoVisionTransformer: a list of crop sets outside the single-row-tensor pass (ragged.py) "
                               "cannot run under a gradient reducer (SSLTrainer(distributed=True, own_reducer=True)); "
                               "use bf16 autocast on the GPU with attention shapes the engine takes, or own_reducer=False")
        from . import vit
        prev, vit.STREAM_OWNED[0] = vit.STREAM_OWNED[0], True
        try:
            for blk in self.blocks:
                xs = blk(xs)
        finally:
            vit.STREAM_OWNED[0] = prev
        return [self._out(self.norm(x), x, m) for x, m in zip(xs, masks_list)]

    def _ragged_ok(self, xs):
        """Can the crop sets run as ONE row tensor (ragged.py)?  The engine's bf16 regime on the GPU, every block a stock
        NestedTensorBlock whose fused path takes every set's sequence length (vit.NestedTensorBlock._ragged's conditions)."""
        from . import vit
        t = xs[0]
        if not (len(xs) > 1 and t.is_cuda and t.dtype == torch.float32 and torch.is_autocast_enabled("cuda")
                and torch.get_autocast_dtype("cuda") == torch.bfloat16 and not torch.compiler.is_compiling()):
            return False
        d = t.shape[-1]
        bf = torch.bfloat16
        for b in self.blocks:
            if not isinstance(b, vit.NestedTensorBlock) or not isinstance(b.attn, vit.Attention) \
                    or not isinstance(b.mlp, (vit.Mlp, vit.SwiGLUFFN)) or not b.mlp.fusable():
                return False
            if any(type(n) is not nn.LayerNorm or tuple(n.normalized_shape) != (d,) or d % 4 or d > 2048
                   for n in (b.norm1, b.norm2)):
                return False
            if not all(isinstance(ls, nn.Identity) or (isinstance(ls, vit.LayerScale) and not ls.inplace)
                       for ls in (b.ls1, b.ls2)):
                return False
            if not all(b.attn.fusable(x.shape[1], bf) for x in xs):
                return False
        return True

    def _forward_features_ragged(self, xs, masks_list):
        """All blocks on the token rows of all crop sets at once (dinov2_models._forward_features_ragged without the octic
        half and the hand-off): every row-wise kernel of a block runs once, every parameter enters the graph once, attention
        walks the sets."""
        from . import ragged as R
        from . import vit
        # (one fresh [1, R, D] tensor, not a view of the concatenation: the batch-subset stochastic depth edits the stream in place)
        rows = torch.cat([x.reshape(1, -1, x.shape[-1]) for x in xs], dim=1)
        rag = R.Ragged([(x.shape[0], x.shape[1]) for x in xs])
        prev_r, prev_o = OF.RAGGED, vit.STREAM_OWNED[0]
        OF.RAGGED, vit.STREAM_OWNED[0] = rag, True
        try:
            if self.training:                        # the batch subsets of the whole pass up front
                sub = [b for b in self.blocks if b.sample_drop_ratio > 0.1]
                if sub:
                    ratios = {b.sample_drop_ratio for b in sub}
                    keeps = ([max(int(B * (1 - sub[0].sample_drop_ratio)), 1) for B, _, _ in rag.sets]
                             if len(ratios) == 1 else None)        # one ratio for all blocks (drop_path_uniform)
                    rag.draw_perms(2 * len(sub), rows.device, keeps)
            x = rows
            for blk in self.blocks:
                x = blk(x)
            xn = self.norm(x)
        finally:
            OF.RAGGED, vit.STREAM_OWNED[0] = prev_r, prev_o
        return [self._out(n, p, m) for n, p, m in zip(rag.views(xn), rag.views(x), masks_list)]

    def forward_features(self, x, masks=None):
        if isinstance(x, list):
            return self.forward_features_list(x, masks)
        x = self.prepare_tokens_with_masks(x, masks)
        x = self._run_blocks(x)
        return self._out(self.norm(x), x, masks)

    def _run_blocks(self, x):
        """The block loop owns the stream it hands from block to block (vit.STREAM_OWNED: no defensive copy in front of the
        batch-subset stochastic depth)."""
        from . import vit
        prev, vit.STREAM_OWNED[0] = vit.STREAM_OWNED[0], True
        try:
            for blk in self.blocks:
                x = blk(x)
        finally:
            vit.STREAM_OWNED[0] = prev
        return x

    def _get_intermediate_layers_not_chunked(self, x, n=1):
        x = self.prepare_tokens_with_masks(x)
        output, total_block_len = [], len(self.blocks)
        blocks_to_take = range(total_block_len - n, total_block_len) if isinstance(n, int) else n
        for i, blk in enumerate(self.blocks):
            x = blk(x)
            if i in blocks_to_take:
                output.append(x)
        assert len(output) == len(blocks_to_take), f"only {len(output)} / {len(blocks_to_take)} blocks found"
        return output

    def get_intermediate_layers(self, x: torch.Tensor, n: Union[int, Sequence] = 1, reshape: bool = False,
                                return_class_token: bool = False, norm=True):
        outputs = self._get_intermediate_layers_not_chunked(x, n)
        if norm:
            outputs = [self.norm(out) for out in outputs]
        class_tokens = [out[:, 0] for out in outputs]
        outputs = [out[:, 1 + self.num_register_tokens:] for out in outputs]
        if reshape:
            B, _, w, h = x.shape
            outputs = [out.reshape(B, w // self.patch_size, h // self.patch_size, -1).permute(0, 3, 1, 2).contiguous()
                       for out in outputs]
        if return_class_token:
            return tuple(zip(outputs, class_tokens))
        return tuple(outputs)

    def forward(self, *args, is_training=False, **kwargs):
        ret = self.forward_features(*args, **kwargs)
        return ret if is_training else self.head(ret["x_norm_clstoken"])

    def invalidate_weight_caches(self):
        return OF.invalidate_weight_caches(self)

    @torch.jit.ignore
    def no_weight_decay(self):
        base_names = ['pos_embed', 'cls_token']
        return set(base_names + [f'_orig_mod.{name}' for name in base_names])


def _refuse_pretrained(pretrained):
    if pretrained:
        raise RuntimeError("no pretrained weights are bundled (load a reference checkpoint with load_state_dict)")


def _dino_vit(embed_dim, depth, num_heads, patch_size, num_register_tokens, pretrained, kwargs):
    _refuse_pretrained(pretrained)
    return DinoVisionTransformer(patch_size=patch_size, embed_dim=embed_dim, depth=depth, num_heads=num_heads, mlp_ratio=4,
                                 block_fn=partial(Block, attn_class=MemEffAttention),
                                 num_register_tokens=num_register_tokens, **kwargs)


# The factories the reference's hub code asks for by name (hub/backbones.py:42: vits.__dict__[arch_name]) beside the two its
# models file defines; the numbers are upstream DINOv2's (ViT-S/14, ViT-B/14, ViT-g/14 - the last with ffn_layer="swiglufused").
@register_model
def vit_small(patch_size=16, num_register_tokens=0, pretrained=False, **kwargs):
    return _dino_vit(384, 12, 6, patch_size, num_register_tokens, pretrained, kwargs)


@register_model
def vit_base(patch_size=16, num_register_tokens=0, pretrained=False, **kwargs):
    return _dino_vit(768, 12, 12, patch_size, num_register_tokens, pretrained, kwargs)


@register_model
def vit_giant2(patch_size=16, num_register_tokens=0, pretrained=False, **kwargs):
    """ViT-g/14's backbone: embed_dim 1536, 40 blocks, 24 heads of 64; with ffn_layer="swiglufused" the FFN's hidden width is
    4096 (w12 [8192, 1536], w3 [1536, 4096]).  That is the only FFN ViT-g/14 was published with, so it is this factory's default
    (the hub code passes it explicitly); ffn_layer="mlp" still builds the plain MLP."""
    kwargs.setdefault("ffn_layer", "swiglufused")
    return _dino_vit(1536, 40, 24, patch_size, num_register_tokens, pretrained, kwargs)


@register_model
def vit_large(patch_size=16, num_register_tokens=0, pretrained=False, **kwargs):
    _refuse_pretrained(pretrained)
    return DinoVisionTransformer(patch_size=patch_size, embed_dim=1024, depth=24, num_heads=16, mlp_ratio=4,
                                 block_fn=partial(Block, attn_class=MemEffAttention),
                                 num_register_tokens=num_register_tokens, **kwargs)


@register_model
def vit_huge(patch_size=16, num_register_tokens=0, pretrained=False, **kwargs):
    _refuse_pretrained(pretrained)
    return DinoVisionTransformer(patch_size=patch_size, embed_dim=1280, depth=32, num_heads=16, mlp_ratio=4,
                                 block_fn=partial(Block, attn_class=MemEffAttention),
                                 num_register_tokens=num_register_tokens, **kwargs)
