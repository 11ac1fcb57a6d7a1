"""The linear depth estimators of the DINOv2 hub on the HIP engine.

Restates ``dinov2/hub/depthers.py`` (``_make_dinov2_linear_depther`` and the four ``dinov2_vit*14_ld`` factories),
``hub/depth/decode_heads.py`` (``DepthBaseDecodeHead.depth_pred``, ``BNHead``), ``hub/depth/encoder_decoder.py`` (its test-time
paths) and ``hub/utils.py:CenterPadding``.

What the reference computes for one image: the patch map and the broadcast class token of 1 or 4 layers are concatenated
(``2 D layers`` channels), resized ``upsample = 4`` times bilinearly, projected to 256 bins by a 1x1 convolution, and the bins
are normalised (relu, + 0.1, divide by the sum) and averaged against ``linspace(min_depth, max_depth, 256)``.  For ViT-L/14 at
518 x 518 the resized tensor is 8192 x 148 x 148 floats (717 MB) and the projection 92 GFLOP.

The projection and the resize are both linear, and bilinear weights sum to 1 at the clamped borders too, so
``conv(up(x)) = up(conv(x))``; the class-token channels are constant over an image, so their share of the projection is one
bias vector per image.  ``BNHead.forward_tokens`` therefore runs two kernels of ``csrc/depth.hip``:

* ``ops.depth_logits``: the bin logits at patch resolution (1/16 of the FLOPs, 1/32 with the class-token half as a bias) on the
  exact-f32 MFMA, reading the token rows of the backbone's block outputs where they lie - no NCHW permute, no ``cat``, no
  resized feature tensor;
* ``ops.depth_expect``: resize, relu, normalisation, expectation and the clamp of ``encode_decode`` in one pass that never
  stores ``[B, 256, 4 h, 4 w]``.

The kernels run for GPU float32 tokens with the hub's head (``classify``, ``UD`` bins, ``linear`` norm, 256 bins,
``align_corners=False``, ``resize_concat``, ``upsample`` 1 | 2 | 4, ``ops.depth_head_ok``) outside ``torch.compile`` tracing,
while ``DEPTH_HIP`` is true and while no gradient is recorded (under ``torch.no_grad()`` / ``inference_mode``, or with nothing
that requires one: the kernels have no backward); every other configuration takes ``BNHead.forward``, the stock composition,
which is complete for every option of the reference and differentiable.  The final ``rescale`` resize of the 1-channel map in
``DepthEncoderDecoder.encode_decode`` stays ``F.interpolate``: one small launch on a map 1/256 the size of the tensor the
kernels removed.

Out of scope: the DPT head (``DPTHead``, ``ReassembleBlocks``, the fusion blocks - 3x3 and transposed convolutions, a different
project), training and the losses (the hub builds its heads with ``loss_decode=()``), datasets, the ONNX branches, and bf16
features (they are cast to float32 in front of the head).
"""
import math
from typing import Optional, Sequence, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .dinov2_vit import _refuse_pretrained

DEPTH_HIP = True          # False: forward_tokens always takes the stock composition


class CenterPadding(nn.Module):
    """Zero-pad the trailing two (H, W) axes up to the next multiple, the odd pixel on the right / bottom
    (hub/utils.py:23-39)."""

    def __init__(self, multiple):
        super().__init__()
        self.multiple = multiple

    def _get_pad(self, size):
        pad = math.ceil(size / self.multiple) * self.multiple - size
        return pad // 2, pad - pad // 2

    def forward(self, x):
        pads = [p for size in x.shape[:1:-1] for p in self._get_pad(size)]    # (W left, W right, H top, H bottom)
        return F.pad(x, pads)


class BNHead(nn.Module):
    """The reference's ``BNHead`` ("just a batchnorm" that was never one): an optional resize + concat of the selected inputs
    and a 1x1 convolution, read as bins of a depth distribution (``classify``) or as the depth itself.  Constructor arguments
    and state-dict keys (``conv_depth.weight [n_bins, channels, 1, 1]``, ``conv_depth.bias``) are the reference's, so the
    published ``*_linear_head.pth`` / ``*_linear4_head.pth`` files load."""

    def __init__(self, in_channels, input_transform="resize_concat", in_index=(0, 1, 2, 3), upsample=1, conv_layer=None,
                 act_layer=nn.ReLU, channels=96, loss_decode=(), sampler=None, align_corners=False, min_depth=1e-3,
                 max_depth=None, norm_layer=None, classify=False, n_bins=256, bins_strategy="UD", norm_strategy="linear",
                 scale_up=False):
        super().__init__()
        self.in_channels, self.channels = in_channels, channels
        self.conv_layer, self.act_layer, self.norm_layer, self.sampler = conv_layer, act_layer, norm_layer, sampler
        self.loss_decode = loss_decode
        self.align_corners = align_corners
        self.min_depth, self.max_depth = min_depth, max_depth
        self.classify, self.n_bins, self.scale_up = classify, n_bins, scale_up
        self.input_transform, self.in_index, self.upsample = input_transform, in_index, upsample
        if classify:
            assert bins_strategy in ["UD", "SID"], "Support bins_strategy: UD, SID"
            assert norm_strategy in ["linear", "softmax", "sigmoid"], "Support norm_strategy: linear, softmax, sigmoid"
            self.bins_strategy, self.norm_strategy = bins_strategy, norm_strategy
        self.conv_depth = nn.Conv2d(channels, n_bins if classify else 1, kernel_size=1, padding=0, stride=1)

    # ---- the stock composition (decode_heads.py:149-178, 237-296)
    def _bins(self, device):
        if self.bins_strategy == "UD":
            return torch.linspace(self.min_depth, self.max_depth, self.n_bins, device=device)
        return torch.logspace(self.min_depth, self.max_depth, self.n_bins, device=device)

    def depth_pred(self, feat):
        if not self.classify:
            if self.scale_up:
                return torch.sigmoid(self.conv_depth(feat)) * self.max_depth
            return torch.relu(self.conv_depth(feat)) + self.min_depth
        logit = self.conv_depth(feat)
        bins = self._bins(feat.device).to(logit.dtype)      # float32 values, as the reference's (a no-op for f32 features)
        if self.norm_strategy == "linear":          # following AdaBins
            logit = torch.relu(logit) + 0.1
            logit = logit / logit.sum(dim=1, keepdim=True)
        elif self.norm_strategy == "softmax":
            logit = torch.softmax(logit, dim=1)
        else:
            logit = torch.sigmoid(logit)
            logit = logit / logit.sum(dim=1, keepdim=True)
        return torch.einsum("ikmn,k->imn", [logit, bins]).unsqueeze(dim=1)

    def _transform_inputs(self, inputs):
        if "concat" in self.input_transform:
            inputs = [inputs[i] for i in self.in_index]
            if "resize" in self.input_transform:
                size = [s * self.upsample for s in inputs[0].shape[2:]]
                inputs = [F.interpolate(x, size=size, mode="bilinear", align_corners=self.align_corners) for x in inputs]
            return torch.cat(inputs, dim=1)
        if self.input_transform == "multiple_select":
            return [inputs[i] for i in self.in_index]
        return inputs[self.in_index]

    def _forward_feature(self, inputs):
        inputs = list(inputs)
        for i, x in enumerate(inputs):
            if len(x) == 2:                         # (patch map, class token): the token rides as extra channels
                x, cls_token = x[0], x[1]
                if x.dim() == 2:
                    x = x[:, :, None, None]
                inputs[i] = torch.cat((x, cls_token[:, :, None, None].expand_as(x)), 1)
            else:
                x = x[0]
                inputs[i] = x[:, :, None, None] if x.dim() == 2 else x
        return self._transform_inputs(inputs)

    def forward(self, inputs, img_metas=None, **kwargs):
        """inputs: per layer (NCHW patch map, class token [B, D]) -> depth [B, 1, upsample h, upsample w], not clamped."""
        return self.depth_pred(self._forward_feature(inputs))

    def forward_test(self, inputs, img_metas=None):
        return self.forward(inputs, img_metas)

    def forward_train(self, *args, **kwargs):
        raise NotImplementedError("BNHead.forward_train: training is out of scope - the hub builds its depth heads with "
                                  "loss_decode=(), there is no loss to compute")

    def losses(self, *args, **kwargs):
        raise NotImplementedError("BNHead.losses: the hub builds its depth heads with loss_decode=(), there is no loss")

    # ---- the engine's path
    def kernels_take(self, pairs):
        """forward_tokens runs csrc/depth.hip for these token-major pairs (module docstring: which heads, which tensors)."""
        if not (DEPTH_HIP and self.classify and self.bins_strategy == "UD" and self.norm_strategy == "linear"
                and not self.align_corners and self.input_transform == "resize_concat") or torch.compiler.is_compiling():
            return False
        layers = len(self.in_index)
        if not 1 <= layers <= 4 or max(self.in_index) >= len(pairs) or min(self.in_index) < 0:
            return False
        p0 = pairs[self.in_index[0]][0]
        if not ops.depth_head_ok(p0.shape[-1], layers, self.n_bins, self.upsample):
            return False
        if self.channels != 2 * p0.shape[-1] * layers or self.max_depth is None:
            return False
        w = self.conv_depth.weight
        if not (w.is_cuda and w.dtype == torch.float32 and all(len(pr) == 2 and pr[0].is_cuda and pr[1].is_cuda
                                                               and pr[0].dim() == 3 for pr in pairs)):
            return False
        # the kernels have no backward: a call that records a gradient takes the stock composition
        return not (torch.is_grad_enabled() and (w.requires_grad or any(t.requires_grad for pr in pairs for t in pr)))

    def forward_tokens(self, pairs, grid):
        """pairs: per layer (patch rows [B, h w, D] - any view with contiguous channels, such as ``out[:, 1 + R:]`` of a block
        output - and class token [B, D]); grid = (h, w).  Depth [B, 1, upsample h, upsample w], clamped to
        [min_depth, max_depth] (the clamp of ``encode_decode``) on both arms.  bf16 features are cast to the weight's float32."""
        h, w = int(grid[0]), int(grid[1])
        dtype = self.conv_depth.weight.dtype
        pairs = [(p.to(dtype), c.to(dtype)) for p, c in pairs]                     # a no-op for float32 features
        if self.kernels_take(pairs):
            sel = []
            for i in self.in_index:
                p, c = pairs[i][0].detach(), pairs[i][1].detach()
                if p.stride(-1) != 1 or p.data_ptr() % 16 or any(s % 4 for s in p.stride()[:-1]):
                    p = p.contiguous()
                if c.stride(-1) != 1 or c.data_ptr() % 16 or c.stride(0) % 4:
                    c = c.contiguous()
                sel.append((p, c))
            weight = self.conv_depth.weight.detach().view(self.n_bins, self.channels)   # the 2-D view, read in place
            Lo = ops.depth_logits(sel, weight, self.conv_depth.bias.detach(), (h, w))
            return ops.depth_expect(Lo, (h, w), self.upsample, self._bins(Lo.device), self.min_depth, self.max_depth)
        maps = [(p.reshape(p.shape[0], h, w, p.shape[-1]).permute(0, 3, 1, 2).contiguous(), c) for p, c in pairs]
        out = self.forward(maps)
        return torch.clamp(out, min=self.min_depth, max=self.max_depth)


class DepthEncoderDecoder(nn.Module):
    """Backbone + decode head with the reference's test-time entry points (hub/depth/encoder_decoder.py).  ``features`` (set by
    ``linear_depther``) holds the keyword arguments of ``backbone.get_intermediate_layers`` and ``pad`` the ``CenterPadding`` in
    front of it - what the reference does by replacing ``backbone.forward`` and registering a pre-hook; without them
    ``extract_feat`` calls the backbone as it is."""

    def __init__(self, backbone, decode_head):
        super().__init__()
        self.backbone = backbone
        self.decode_head = decode_head
        self.align_corners = decode_head.align_corners
        self.features = None
        self.pad = None

    def extract_feat(self, img, reshape=True):
        if self.features is None:
            return self.backbone(img)
        if self.pad is not None:
            img = self.pad(img)
        return self.backbone.get_intermediate_layers(img, reshape=reshape, **self.features)

    def _takes_tokens(self):
        return self.features is not None and hasattr(self.decode_head, "forward_tokens")

    def encode_decode(self, img, img_metas, rescale=True, size=None):
        """Depth map of the images, clamped to the head's range; ``rescale`` resizes it to ``size``, else to the first
        meta's ``ori_shape``, else to the input's size.  That last resize is ``F.interpolate`` on the 1-channel map."""
        head = self.decode_head
        if self._takes_tokens():
            x = self.extract_feat(img, reshape=False)
            p = _patch_size(self.backbone)
            ph, pw = (img.shape[2:] if self.pad is None else [math.ceil(s / self.pad.multiple) * self.pad.multiple
                                                                for s in img.shape[2:]])
            out = head.forward_tokens(x, (ph // p, pw // p))
        else:
            out = head.forward_test(self.extract_feat(img), img_metas)
            out = torch.clamp(out, min=head.min_depth, max=head.max_depth)
        if rescale:
            if size is None:
                size = img_metas[0]["ori_shape"][:2] if img_metas is not None else img.shape[2:]
            out = F.interpolate(out, size=tuple(size), mode="bilinear", align_corners=self.align_corners)
        return out

    def forward_dummy(self, img):
        return self.encode_decode(img, None)

    def whole_inference(self, img, img_meta, rescale, size=None):
        return self.encode_decode(img, img_meta, rescale, size=size)

    def slide_inference(self, img, img_meta, rescale, stride, crop_size):
        """Overlapping windows of crop_size every stride pixels, the predictions averaged where they overlap; a window larger
        than the image is the image."""
        (h_stride, w_stride), (h_crop, w_crop) = stride, crop_size
        batch, _, h_img, w_img = img.shape
        h_grids = max(h_img - h_crop + h_stride - 1, 0) // h_stride + 1
        w_grids = max(w_img - w_crop + w_stride - 1, 0) // w_stride + 1
        preds = img.new_zeros((batch, 1, h_img, w_img))
        count = img.new_zeros((batch, 1, h_img, w_img))
        for hi in range(h_grids):
            for wi in range(w_grids):
                y2, x2 = min(hi * h_stride + h_crop, h_img), min(wi * w_stride + w_crop, w_img)
                y1, x1 = max(y2 - h_crop, 0), max(x2 - w_crop, 0)
                pred = self.encode_decode(img[:, :, y1:y2, x1:x2], img_meta, rescale)
                preds += F.pad(pred, (x1, w_img - x2, y1, h_img - y2))
                count[:, :, y1:y2, x1:x2] += 1
        assert (count == 0).sum() == 0
        return preds / count

    def inference(self, img, img_meta, rescale, size=None, mode="whole", stride=None, crop_size=None):
        """``mode="slide"`` needs stride and crop_size (the reference calls slide_inference without them and fails with a
        TypeError as shipped); a meta with ``flip`` set has its prediction flipped back."""
        assert mode in ["slide", "whole"]
        ori_shape = img_meta[0]["ori_shape"]
        assert all(m["ori_shape"] == ori_shape for m in img_meta)
        if mode == "slide":
            if stride is None or crop_size is None:
                raise ValueError('inference(mode="slide") needs stride and crop_size')
            out = self.slide_inference(img, img_meta, rescale, stride, crop_size)
        else:
            out = self.whole_inference(img, img_meta, rescale, size=size)
        if img_meta[0]["flip"]:
            direction = img_meta[0]["flip_direction"]
            assert direction in ["horizontal", "vertical"]
            out = out.flip(dims=(3,) if direction == "horizontal" else (2,))
        return out

    def simple_test(self, img, img_meta, rescale=True):
        return list(self.inference(img, img_meta, rescale).cpu().numpy())

    def aug_test(self, imgs, img_metas, rescale=True):
        """Mean over the augmented views, each brought back to the first one's size (only rescale=True)."""
        assert rescale
        out = self.inference(imgs[0], img_metas[0], rescale)
        for i in range(1, len(imgs)):
            out += self.inference(imgs[i], img_metas[i], rescale, size=out.shape[-2:])
        out /= len(imgs)
        return list(out.cpu().numpy())

    def forward_test(self, imgs, img_metas, **kwargs):
        for var, name in [(imgs, "imgs"), (img_metas, "img_metas")]:
            if not isinstance(var, list):
                raise TypeError(f"{name} must be a list, but got {type(var)}")
        if len(imgs) != len(img_metas):
            raise ValueError(f"num of augmentations ({len(imgs)}) != num of image meta ({len(img_metas)})")
        for metas in img_metas:                     # one augmentation = one batch of equal shapes
            for key in ("ori_shape", "img_shape", "pad_shape"):
                assert all(m[key] == metas[0][key] for m in metas)
        if len(imgs) == 1:
            return self.simple_test(imgs[0], img_metas[0], **kwargs)
        return self.aug_test(imgs, img_metas, **kwargs)

    def forward(self, img, img_metas, return_loss=False, **kwargs):
        if return_loss:
            return self.forward_train(img, img_metas, **kwargs)
        return self.forward_test(img, img_metas, **kwargs)

    def forward_train(self, *args, **kwargs):
        raise NotImplementedError("DepthEncoderDecoder.forward_train: training is out of scope - the hub builds its depth heads "
                                  "with loss_decode=(), there is no loss to train on")

    def train_step(self, *args, **kwargs):
        raise NotImplementedError("DepthEncoderDecoder.train_step: training is out of scope - the hub builds its depth heads "
                                  "with loss_decode=(), there is no loss to train on")

    def losses(self, *args, **kwargs):
        raise NotImplementedError("DepthEncoderDecoder.losses: the hub builds its depth heads with loss_decode=(), there is no "
                                  "loss")


def _patch_size(backbone):
    p = getattr(backbone, "patch_size", None)
    if p is None:
        p = backbone.patch_embed.patch_size
    return int(p[0] if isinstance(p, (tuple, list)) else p)


def _linear_depth_head(embed_dim, layers):
    """_make_dinov2_linear_depth_head: the range in the head is 0.001 .. 80 whatever depth_range the caller chose."""
    if layers not in (1, 4):
        raise AssertionError(f"Unsupported number of layers: {layers}")
    in_index = [0] if layers == 1 else [0, 1, 2, 3]
    return BNHead(classify=True, n_bins=256, bins_strategy="UD", norm_strategy="linear", upsample=4,
                  in_channels=[embed_dim] * layers, in_index=in_index, input_transform="resize_concat",
                  channels=embed_dim * layers * 2, align_corners=False, min_depth=0.001, max_depth=80, loss_decode=())


def linear_depther(backbone, layers: int = 4, out_index: Optional[Sequence[int]] = None,
                   depth_range: Optional[Tuple[float, float]] = None):
    """A linear depth estimator on any backbone with ``get_intermediate_layers`` and ``embed_dim`` (DinoVisionTransformer,
    OcticDinoVisionTransformer): the hub's BNHead on the blocks ``out_index`` (default: ``layers`` blocks spread evenly, the last
    one included; the named factories pass the reference's tables).  ``depth_range`` is accepted and, as in the reference, does
    not reach the head."""
    if layers not in (1, 4):
        raise AssertionError(f"Unsupported number of layers: {layers}")
    n = len(backbone.blocks)
    if out_index is None:
        out_index = [n - 1] if layers == 1 else [n * (i + 1) // layers - 1 for i in range(layers)]
    if len(out_index) != layers:
        raise ValueError(f"out_index must name {layers} blocks, got {list(out_index)}")
    model = DepthEncoderDecoder(backbone, _linear_depth_head(backbone.embed_dim, layers))
    model.features = dict(n=list(out_index), return_class_token=True, norm=False)
    model.pad = CenterPadding(_patch_size(backbone))
    return model


LAYER_COUNT = {"vit_small": 12, "vit_base": 12, "vit_large": 24, "vit_giant2": 40}
OUT_INDEX = {"vit_small": [2, 5, 8, 11], "vit_base": [2, 5, 8, 11], "vit_large": [4, 11, 17, 23], "vit_giant2": [9, 19, 29, 39]}
WEIGHTS = ("NYU", "KITTI")


def _hub_depther(arch_name, layers, pretrained, weights, depth_range=None, **kwargs):
    from . import dinov2_vit
    if layers not in (1, 4):
        raise AssertionError(f"Unsupported number of layers: {layers}")
    if str(getattr(weights, "value", weights)) not in WEIGHTS:
        raise AssertionError(f"Unsupported weights: {weights}")
    _refuse_pretrained(pretrained)
    kw = dict(patch_size=14, img_size=518, init_values=1.0, block_chunks=0)       # hub/backbones.py:27-35
    kw.update(kwargs)
    backbone = getattr(dinov2_vit, arch_name)(**kw)
    out_index = OUT_INDEX[arch_name] if layers == 4 else [LAYER_COUNT[arch_name] - 1]
    return linear_depther(backbone, layers=layers, out_index=out_index, depth_range=depth_range)


def dinov2_vits14_ld(*, layers=4, pretrained=False, weights="NYU", **kwargs):
    return _hub_depther("vit_small", layers, pretrained, weights, **kwargs)


def dinov2_vitb14_ld(*, layers=4, pretrained=False, weights="NYU", **kwargs):
    return _hub_depther("vit_base", layers, pretrained, weights, **kwargs)


def dinov2_vitl14_ld(*, layers=4, pretrained=False, weights="NYU", **kwargs):
    return _hub_depther("vit_large", layers, pretrained, weights, **kwargs)


def dinov2_vitg14_ld(*, layers=4, pretrained=False, weights="NYU", **kwargs):
    return _hub_depther("vit_giant2", layers, pretrained, weights, ffn_layer="swiglufused", **kwargs)


def load_head_state_dict(model, checkpoint):
    """Load a published ``*_linear_head.pth`` / ``*_linear4_head.pth`` (a dict with or without the ``"state_dict"`` wrapper)
    non-strictly, as depthers.py:135-138 does; returns load_state_dict's missing / unexpected keys."""
    state = checkpoint["state_dict"] if "state_dict" in checkpoint else checkpoint
    return model.load_state_dict(state, strict=False)
