"""The depth estimators of the DINOv2 hub: the linear ones on the HIP engine, the DPT ones as modules.

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

The DPT estimators (``dinov2_vit*14_dd``: ``DPTHead``, ``ReassembleBlocks``, ``PreActResidualConvUnit``, ``FeatureFusionBlock``,
``HeadDepth`` of decode_heads.py:512-747) share the encoder-decoder and the factories' tables.  ``DPTHead.forward`` is the stock
NCHW composition in the reference's order of operations and ``DPTHead.forward_tokens`` calls it, ON THE CPU ONLY: this head has
no kernel path yet, and the stock composition is not a supported GPU path either - a GPU process that ran a channels-last
kernel arm next to it ended in an illegal memory access that was reported from inside this composition and whose cause is open
(NOTES, 'DPT depth head').  A GPU tensor or a head moved to the GPU is refused with an error before anything is launched
(``DPTHead.refuse_gpu``; ``DepthEncoderDecoder.encode_decode`` asks before it runs the backbone).  What the modules are for until
the kernels exist: the reference's state-dict layout (the published ``*_dpt_head.pth`` files load) and a CPU evaluation that
reproduces the reference's numbers (tests/golden/dpt_head.npz).

Out of scope: the DPT head on the GPU, training and the losses (the hub builds its heads with ``loss_decode=()``),
``norm_layer`` in the DPT head (the reference's branch cannot be imported), datasets, the ONNX branches, and bf16 features
(they are cast to float32 in front of the head).
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
        if hasattr(head, "refuse_gpu"):             # a head without a GPU path says so before the backbone runs
            head.refuse_gpu(img)
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


def _hub_backbone(arch_name, pretrained, weights, kwargs):
    """What the hub's linear and DPT depthers share: the weights check, the refusal of downloads and the backbone."""
    from . import dinov2_vit
    if str(getattr(weights, "value", weights)) not in WEIGHTS:
        raise AssertionError(f"Unsupported weights: {weights}")
    _refuse_pretrained(pretrained)
    kw = dict(patch_size=14, img_size=518, init_values=1.0, block_chunks=0)       # hub/backbones.py:27-35
    kw.update(kwargs)
    return getattr(dinov2_vit, arch_name)(**kw)


def _hub_depther(arch_name, layers, pretrained, weights, depth_range=None, **kwargs):
    if layers not in (1, 4):
        raise AssertionError(f"Unsupported number of layers: {layers}")
    backbone = _hub_backbone(arch_name, pretrained, weights, kwargs)
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


# ------------------------------------------------------------------------------------------------ the DPT head
class _ConvModule(nn.Module):
    """The reference's conv block as the DPT head uses it: ``conv`` (the state-dict key) and an optional in-place activation in
    ``order`` ("conv" before or after "act").  ``norm_layer`` is refused: the reference's own branch for it imports
    ``torch.nnModules`` and cannot run."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True, norm_layer=None, act_layer=nn.ReLU,
                 order=("conv", "norm", "act")):
        super().__init__()
        if norm_layer is not None:
            raise NotImplementedError("DPT head: norm_layer is not supported (the reference's branch for it cannot be imported)")
        self.order = order
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, stride=stride, padding=padding, bias=bias)
        self.with_activation = act_layer is not None
        if self.with_activation:
            self.activate = act_layer() if isinstance(act_layer, type) and issubclass(act_layer, (nn.Tanh, nn.PReLU, nn.Sigmoid, nn.GELU)) \
                else act_layer(inplace=True)
        nn.init.kaiming_normal_(self.conv.weight, a=0, mode="fan_out", nonlinearity="relu")
        if self.conv.bias is not None:
            nn.init.constant_(self.conv.bias, 0)

    def forward(self, x):
        for layer in self.order:
            if layer == "conv":
                x = self.conv(x)
            elif layer == "act" and self.with_activation:
                x = self.activate(x)
        return x


class _Interpolate(nn.Module):
    def __init__(self, scale_factor, mode, align_corners=False):
        super().__init__()
        self.scale_factor, self.mode, self.align_corners = scale_factor, mode, align_corners

    def forward(self, x):
        return F.interpolate(x, scale_factor=self.scale_factor, mode=self.mode, align_corners=self.align_corners)


class HeadDepth(nn.Module):
    """3x3 conv to features // 2, x2 bilinear (align_corners=True), 3x3 conv to 32, ReLU, 1x1 conv to 1 (decode_heads.py:512-525)."""

    def __init__(self, features):
        super().__init__()
        self.head = nn.Sequential(nn.Conv2d(features, features // 2, kernel_size=3, stride=1, padding=1),
                                  _Interpolate(scale_factor=2, mode="bilinear", align_corners=True),
                                  nn.Conv2d(features // 2, 32, kernel_size=3, stride=1, padding=1), nn.ReLU(),
                                  nn.Conv2d(32, 1, kernel_size=1, stride=1, padding=0))

    def forward(self, x):
        return self.head(x)


class ReassembleBlocks(nn.Module):
    """Readout of the class token ("ignore" | "add" | "project"), a 1x1 projection per stage and the resize layers: transposed
    convolutions x4 and x2, identity, a 3x3 stride-2 convolution (decode_heads.py:528-597)."""

    def __init__(self, in_channels=768, out_channels=(96, 192, 384, 768), readout_type="ignore", patch_size=16):
        super().__init__()
        assert readout_type in ["ignore", "add", "project"]
        self.readout_type, self.patch_size = readout_type, patch_size
        oc = list(out_channels)
        self.projects = nn.ModuleList([_ConvModule(in_channels, c, kernel_size=1, act_layer=None) for c in oc])
        self.resize_layers = nn.ModuleList([nn.ConvTranspose2d(oc[0], oc[0], kernel_size=4, stride=4, padding=0),
                                            nn.ConvTranspose2d(oc[1], oc[1], kernel_size=2, stride=2, padding=0),
                                            nn.Identity(),
                                            nn.Conv2d(oc[3], oc[3], kernel_size=3, stride=2, padding=1)])
        if readout_type == "project":
            self.readout_projects = nn.ModuleList([nn.Sequential(nn.Linear(2 * in_channels, in_channels), nn.GELU())
                                                   for _ in range(len(self.projects))])

    def _readout(self, i, fmap, cls):
        """Stage i's map [B, D, h, w] with its class token [B, D] read out into it."""
        if self.readout_type == "ignore":
            return fmap
        if self.readout_type == "add":
            return fmap + cls[:, :, None, None]
        rows = fmap.flatten(2).transpose(1, 2)                                   # [B, h w, D]
        rows = self.readout_projects[i](torch.cat((rows, cls[:, None, :].expand_as(rows)), dim=-1))
        return rows.transpose(1, 2).reshape(fmap.shape)

    def forward(self, inputs):
        """inputs: per stage (patch map [B, D, h, w], class token [B, D]) -> the four maps at 4 h, 2 h, h and ceil(h / 2)."""
        if len(inputs) != len(self.projects) or any(len(pair) != 2 for pair in inputs):
            raise ValueError(f"ReassembleBlocks: {len(self.projects)} (patch map, class token) pairs expected")
        return [resize(project(self._readout(i, fmap, cls)))
                for i, ((fmap, cls), project, resize) in enumerate(zip(inputs, self.projects, self.resize_layers))]


class PreActResidualConvUnit(nn.Module):
    """relu, conv, relu, conv, + input.  The first ReLU is in place, as the reference's: the CALLER's tensor is rectified, the
    skip is the un-rectified clone taken before it (decode_heads.py:600-641)."""

    def __init__(self, in_channels, act_layer, norm_layer, stride=1, dilation=1):
        super().__init__()
        if dilation != 1:
            raise NotImplementedError("PreActResidualConvUnit: dilation 1 only")
        kw = dict(norm_layer=norm_layer, act_layer=act_layer, bias=False, order=("act", "conv", "norm"))
        self.conv1 = _ConvModule(in_channels, in_channels, 3, stride=stride, padding=1, **kw)
        self.conv2 = _ConvModule(in_channels, in_channels, 3, padding=1, **kw)

    def forward(self, inputs):
        inputs_ = inputs.clone()
        return self.conv2(self.conv1(inputs)) + inputs_


class FeatureFusionBlock(nn.Module):
    """x + unit1(skip resized to x), unit2, x2 bilinear upsample, 1x1 project (decode_heads.py:644-687)."""

    def __init__(self, in_channels, act_layer, norm_layer, expand=False, align_corners=True):
        super().__init__()
        self.in_channels, self.expand, self.align_corners = in_channels, expand, align_corners
        self.out_channels = in_channels // 2 if expand else in_channels
        self.project = _ConvModule(self.in_channels, self.out_channels, kernel_size=1, act_layer=None, bias=True)
        self.res_conv_unit1 = PreActResidualConvUnit(in_channels, act_layer, norm_layer)
        self.res_conv_unit2 = PreActResidualConvUnit(in_channels, act_layer, norm_layer)

    def forward(self, *inputs):
        x = inputs[0]
        if len(inputs) == 2:
            res = inputs[1]
            if x.shape != res.shape:
                res = F.interpolate(res, size=(x.shape[2], x.shape[3]), mode="bilinear", align_corners=False)
            x = x + self.res_conv_unit1(res)
        x = self.res_conv_unit2(x)
        x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=self.align_corners)
        return self.project(x)


class DPTHead(nn.Module):
    """The reference's ``DPTHead`` (decode_heads.py:690-747) with its constructor arguments and state-dict keys, so the published
    ``*_dpt_head.pth`` files load.  ``forward`` is the stock composition on NCHW pairs in the reference's order of operations;
    ``forward_tokens`` brings the token rows a ``DepthEncoderDecoder`` hands over into that form and clamps.  CPU only (module
    docstring): ``refuse_gpu`` turns a GPU tensor or a head on the GPU into an error."""

    def __init__(self, embed_dims=768, post_process_channels=(96, 192, 384, 768), readout_type="ignore", patch_size=16,
                 expand_channels=False, *, in_channels, conv_layer=None, act_layer=nn.ReLU, channels=96, loss_decode=(), sampler=None,
                 align_corners=False, min_depth=1e-3, max_depth=None, norm_layer=None, classify=False, n_bins=256,
                 bins_strategy="UD", norm_strategy="linear", scale_up=False):
        super().__init__()
        if norm_layer is not None:
            raise NotImplementedError("DPTHead: norm_layer is not supported (the reference's branch for it cannot be imported)")
        self.in_channels, self.channels = in_channels, channels
        self.conv_layer, self.act_layer, self.norm_layer, self.sampler = conv_layer, act_layer, norm_layer, sampler
        self.loss_decode = loss_decode
        self.align_corners = align_corners
        self.min_depth, self.max_depth = min_depth, max_depth
        self.classify, self.n_bins, self.scale_up = classify, n_bins, scale_up
        if classify:
            assert bins_strategy in ["UD", "SID"], "Support bins_strategy: UD, SID"
            assert norm_strategy in ["linear", "softmax", "sigmoid"], "Support norm_strategy: linear, softmax, sigmoid"
            self.bins_strategy, self.norm_strategy = bins_strategy, norm_strategy
        self.embed_dims, self.expand_channels = embed_dims, expand_channels
        ppc = list(post_process_channels)
        self.reassemble_blocks = ReassembleBlocks(embed_dims, ppc, readout_type, patch_size)
        self.post_process_channels = [c * 2 ** i if expand_channels else c for i, c in enumerate(ppc)]
        self.convs = nn.ModuleList([_ConvModule(c, channels, kernel_size=3, padding=1, act_layer=None, bias=False)
                                    for c in self.post_process_channels])
        self.fusion_blocks = nn.ModuleList([FeatureFusionBlock(channels, act_layer, norm_layer) for _ in range(len(self.convs))])
        self.fusion_blocks[0].res_conv_unit1 = None
        self.project = _ConvModule(channels, channels, kernel_size=3, padding=1, norm_layer=norm_layer)
        self.num_fusion_blocks = self.num_reassemble_blocks = self.num_post_process_channels = len(self.convs)   # the reference's names
        if len(self.reassemble_blocks.resize_layers) != len(self.convs):
            raise ValueError("DPTHead: post_process_channels names four stages")
        self.conv_depth = HeadDepth(channels)

    # ---- the stock composition
    def depth_pred(self, feat):
        """depth_pred's regression branches (decode_heads.py:173-177); the hub's DPT heads are built with classify=False."""
        if self.classify:
            raise NotImplementedError("DPTHead.depth_pred: classify=True would put 256 bins through HeadDepth's 1-channel output")
        if self.scale_up:
            return torch.sigmoid(self.conv_depth(feat)) * self.max_depth
        return torch.relu(self.conv_depth(feat)) + self.min_depth

    def refuse_gpu(self, *tensors):
        """This head has no supported GPU path (module docstring): a GPU tensor or a head moved to the GPU is an error, raised
        before anything is launched.  ``DepthEncoderDecoder.encode_decode`` asks before it runs the backbone."""
        if any(t.is_cuda for t in tensors) or any(p.is_cuda for p in self.parameters()):
            raise RuntimeError("DPTHead: the DPT depth head has no GPU path yet - its kernels are not in this package and the stock "
                               "composition is not supported on the GPU (NOTES, 'DPT depth head'); run the head on the CPU")

    def forward(self, inputs, img_metas=None, **kwargs):
        """inputs: 4 pairs (NCHW patch map, class token [B, D]) on the CPU -> depth [B, 1, 32 h', 32 w'] (h' = ceil(h / 2)), not
        clamped.  Coarse to fine: the last stage opens the chain, every fusion block takes the next finer stage as its skip.  The
        in-place ReLUs of the residual units rectify tensors this method made itself, never the caller's."""
        self.refuse_gpu(*[t for pair in inputs for t in pair])
        stages = [conv(fmap) for conv, fmap in zip(self.convs, self.reassemble_blocks(list(inputs)))]
        fused = self.fusion_blocks[0](stages[-1])
        for block, skip in zip(self.fusion_blocks[1:], reversed(stages[:-1])):
            fused = block(fused, skip)
        return self.depth_pred(self.project(fused))

    def forward_test(self, inputs, img_metas=None):
        return self.forward(inputs, img_metas)

    def forward_train(self, *args, **kwargs):
        raise NotImplementedError("DPTHead.forward_train: training is out of scope - the hub builds its depth heads with "
                                  "loss_decode=(), there is no loss to compute")

    def losses(self, *args, **kwargs):
        raise NotImplementedError("DPTHead.losses: the hub builds its depth heads with loss_decode=(), there is no loss")

    def forward_tokens(self, pairs, grid):
        """pairs: 4 x (patch rows [B, h w, D] - such as ``out[:, 1 + R:]`` of a block output - and class token [B, D]);
        grid = (h, w), on the CPU.  Depth [B, 1, 32 h', 32 w'] (h' = ceil(h / 2)) from the stock composition, clamped to
        [min_depth, max_depth] (the clamp of ``encode_decode``).  bf16 features are cast to the weights' float32."""
        self.refuse_gpu(*[t for pair in pairs for t in pair])
        h, w = int(grid[0]), int(grid[1])
        dtype = self.conv_depth.head[4].weight.dtype
        maps = [(p.to(dtype).reshape(p.shape[0], h, w, p.shape[-1]).permute(0, 3, 1, 2).contiguous(), c.to(dtype)) for p, c in pairs]
        out = self.forward(maps)
        return torch.clamp(out, min=self.min_depth, max=self.max_depth)


def _dpt_depth_head(embed_dim, min_depth, max_depth):
    """_make_dinov2_dpt_depth_head."""
    return DPTHead(in_channels=[embed_dim] * 4, channels=256, embed_dims=embed_dim,
                   post_process_channels=[embed_dim // 2 ** (3 - i) for i in range(4)], readout_type="project",
                   min_depth=min_depth, max_depth=max_depth, loss_decode=())


def dpt_depther(backbone, out_index: Optional[Sequence[int]] = None, min_depth=0.001, max_depth=10.0):
    """A DPT depth estimator on any backbone with ``get_intermediate_layers`` and ``embed_dim``: the hub's DPTHead (channels 256,
    post_process_channels [D / 8, D / 4, D / 2, D], the "project" readout) on the four blocks ``out_index`` (default: spread
    evenly, the last one included; the named factories pass the reference's tables)."""
    n = len(backbone.blocks)
    if out_index is None:
        out_index = [n * (i + 1) // 4 - 1 for i in range(4)]
    if len(out_index) != 4:
        raise ValueError(f"out_index must name 4 blocks, got {list(out_index)}")
    model = DepthEncoderDecoder(backbone, _dpt_depth_head(backbone.embed_dim, min_depth, max_depth))
    model.features = dict(n=list(out_index), return_class_token=True, norm=False)
    model.pad = CenterPadding(_patch_size(backbone))
    return model


def _hub_dpt_depther(arch_name, pretrained, weights, depth_range=None, **kwargs):
    backbone = _hub_backbone(arch_name, pretrained, weights, kwargs)
    lo, hi = depth_range if depth_range is not None else (0.001, 10.0)    # _get_depth_range of an untrained head, NYU or KITTI
    return dpt_depther(backbone, out_index=OUT_INDEX[arch_name], min_depth=lo, max_depth=hi)


def dinov2_vits14_dd(*, pretrained=False, weights="NYU", depth_range=None, **kwargs):
    return _hub_dpt_depther("vit_small", pretrained, weights, depth_range, **kwargs)


def dinov2_vitb14_dd(*, pretrained=False, weights="NYU", depth_range=None, **kwargs):
    return _hub_dpt_depther("vit_base", pretrained, weights, depth_range, **kwargs)


def dinov2_vitl14_dd(*, pretrained=False, weights="NYU", depth_range=None, **kwargs):
    return _hub_dpt_depther("vit_large", pretrained, weights, depth_range, **kwargs)


def dinov2_vitg14_dd(*, pretrained=False, weights="NYU", depth_range=None, **kwargs):
    return _hub_dpt_depther("vit_giant2", pretrained, weights, depth_range, ffn_layer="swiglufused", **kwargs)


def load_head_state_dict(model, checkpoint):
    """Load a published ``*_linear_head.pth`` / ``*_linear4_head.pth`` / ``*_dpt_head.pth`` (a dict with or without the ``"state_dict"`` wrapper)
    non-strictly, as depthers.py:135-138 does; returns load_state_dict's missing / unexpected keys."""
    state = checkpoint["state_dict"] if "state_dict" in checkpoint else checkpoint
    return model.load_state_dict(state, strict=False)
