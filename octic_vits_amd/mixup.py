"""Mixup / CutMix on the device, and the BCE loss of the DeiT-III recipe without materialised targets.

``Mixup`` has the signature of timm's ``timm.data.mixup.Mixup`` and consumes ``numpy.random`` exactly as it does: the
same variates in the same order, so ``numpy.random.seed(s)`` reproduces timm's stream.  timm is not a dependency of this
project; parity is pinned to the following restatement of ``timm/data/mixup.py``, written from the published algorithm
(the same arrangement as the apex LAMB restatement in ``train.Lamb``).  THIS IS THE CONTRACT:

* ``batch`` mode: ``lam = 1``, ``cut = False``.  If enabled (an alpha > 0) and ``rand() < prob``: with both alphas > 0,
  ``cut = rand() < switch_prob`` then one ``beta(a, a)`` with the cutmix alpha if ``cut`` else the mixup alpha; with only the
  mixup alpha ``beta(mixup_alpha)``; with only the cutmix alpha ``cut = True``, ``beta(cutmix_alpha)``.  ``lam == 1``: nothing
  is mixed.  With ``cut`` one box is drawn for the whole batch and ``lam`` corrected.  The partner of sample i is B-1-i.
* ``elem`` mode: vectors of size B drawn in this order - ``rand(B) < switch_prob``; ``beta(cutmix, size=B)``;
  ``beta(mixup, size=B)`` (selected with ``np.where``: both are always drawn when both alphas are > 0);
  ``rand(B) < prob`` selecting ``lam_mix.astype(float32)`` or 1.  Then for i = 0..B-1 with ``lam_i != 1`` and ``cut_i`` one box
  per such element, in index order.  Partner B-1-i.
* ``pair`` mode: the ``elem`` parameters for B/2; element i and its partner B-1-i share ``lam`` and the box;
  ``lam_batch = concat(lam, lam[::-1])``.
* box (``rand_bbox``): ``ratio = sqrt(1-lam)``; ``cut_h, cut_w = int(H*ratio), int(W*ratio)``; ``cy = randint(0, H)`` then
  ``cx = randint(0, W)``; ``yl, yh = clip(cy - cut_h//2, 0, H), clip(cy + cut_h//2, 0, H)``, x likewise.
* box with ``cutmix_minmax`` (``rand_bbox_minmax``; the cutmix alpha is forced to 1): ``cut_h = randint(int(H*min),
  int(H*max))`` then ``cut_w`` likewise; ``yl = randint(0, H-cut_h)``, ``xl = randint(0, W-cut_w)``; ``yh = yl+cut_h``,
  ``xh = xl+cut_w``.
* corrected ``lam``: if ``correct_lam`` or min/max is set, ``lam = 1 - (yh-yl)(xh-xl)/(H W)``.
* targets (``mixup_target``): ``off = s/num_classes``, ``on = 1 - s + off``;
  ``t = lam * onehot(y, on, off) + (1-lam) * onehot(y.flip(0), on, off)``, ``lam`` per row in ``elem`` / ``pair`` modes.  With
  ``binarize`` (the recipe's ``--bce-loss``, deit/engine.py:53-54) ``t = (t > 0)``.  The reference's quirk, kept: with label
  smoothing ``s > 0`` every entry is positive, so EVERY binarised entry is 1 (the recipe runs ``smoothing=0.0``).
* odd B raises ``ValueError`` (timm asserts).

Differences from timm, all on the device side: the mix is out of place (``apply`` returns a new batch, the input is left
alone); the kernels take ``lam`` as the f32 value of ``MixParams.lam`` and form ``1 - lam`` in f32 (timm's ``batch`` mode rounds
the f64 ``1 - lam`` instead: the last bit of a weight); a sample whose f32 ``lam`` is 1 is not mixed at all.
"""
from dataclasses import dataclass

import numpy as np
import torch

from . import ops

__all__ = ["Mixup", "MixParams", "mix_images", "mix_targets", "mix_bce_loss", "mix_ce_loss", "cosub_bce_loss", "smoothing_on_off",
           "TableUploader"]


@dataclass
class MixParams:
    """One draw for a batch of B samples: ``partner`` int32 [B], ``lam`` float32 [B] (the weight of the sample itself),
    ``cut`` bool [B] (CutMix: paste the box; else blend) and ``box`` int32 [B, 4] = yl, yh, xl, xh.  A sample with
    ``lam == 1`` is not mixed: ``cut`` False and an empty box."""
    partner: np.ndarray
    lam: np.ndarray
    cut: np.ndarray
    box: np.ndarray

    def __post_init__(self):
        self.partner = np.ascontiguousarray(self.partner, dtype=np.int32)
        self.lam = np.ascontiguousarray(self.lam, dtype=np.float32)
        self.cut = np.ascontiguousarray(self.cut, dtype=bool)
        self.box = np.ascontiguousarray(self.box, dtype=np.int32).reshape(-1, 4)
        B = self.partner.shape[0]
        if self.lam.shape != (B,) or self.cut.shape != (B,) or self.box.shape != (B, 4):
            raise ValueError("MixParams: partner, lam, cut must be [B] and box [B, 4]")

    @classmethod
    def identity(cls, B):
        return cls(np.arange(B, dtype=np.int32), np.ones(B, np.float32), np.zeros(B, bool), np.zeros((B, 4), np.int32))

    def __len__(self):
        return int(self.partner.shape[0])

    def __eq__(self, other):
        return (isinstance(other, MixParams) and np.array_equal(self.partner, other.partner)
                and np.array_equal(self.lam, other.lam) and np.array_equal(self.cut, other.cut)
                and np.array_equal(self.box, other.box))

    def table(self):
        """The packed rows the kernels read (``octic_mix_row``, include/octic_hip.h): int32 [B, 8] =
        partner | lam (f32 bits) | cut | yl | yh | xl | xh | 0."""
        B = len(self)
        t = np.zeros((B, 8), dtype=np.int32)
        t[:, 0] = self.partner
        t[:, 1] = self.lam.view(np.int32)
        t[:, 2] = self.cut
        t[:, 3:7] = self.box
        return t


class Mixup:
    """timm's ``Mixup`` (signature, draws and targets; see the module docstring for the contract) on the HIP kernels of
    csrc/mixup.hip.  ``rng=None`` draws from the ``numpy.random`` module functions as timm does; a
    ``numpy.random.RandomState`` may be passed instead (data parallel: one per rank, seeded ``seed + rank``)."""

    def __init__(self, mixup_alpha=1.0, cutmix_alpha=0.0, cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode="batch",
                 correct_lam=True, label_smoothing=0.1, num_classes=1000, rng=None):
        if mode not in ("batch", "pair", "elem"):
            raise ValueError(f"Mixup: mode must be 'batch', 'pair' or 'elem', got {mode!r}")
        self.mixup_alpha = mixup_alpha
        self.cutmix_alpha = cutmix_alpha
        self.cutmix_minmax = cutmix_minmax
        if self.cutmix_minmax is not None:
            if len(self.cutmix_minmax) != 2:
                raise ValueError("Mixup: cutmix_minmax must be (min, max)")
            self.cutmix_alpha = 1.0                    # timm: min/max forces the cutmix alpha to 1
        self.mix_prob = prob
        self.switch_prob = switch_prob
        self.label_smoothing = label_smoothing
        self.num_classes = int(num_classes)
        self.mode = mode
        self.correct_lam = correct_lam
        self.mixup_enabled = True
        self.rng = np.random if rng is None else rng

    # ---- the host side: plain numpy ------------------------------------------------------------------------------------
    @property
    def _active(self):
        return self.mixup_enabled and (self.mixup_alpha > 0. or self.cutmix_alpha > 0.)

    def on_off(self):
        """The one-hot values of ``mixup_target``: (on, off)."""
        off = self.label_smoothing / self.num_classes
        return 1. - self.label_smoothing + off, off

    def _rand_bbox(self, H, W, lam):
        r = self.rng
        ratio = np.sqrt(1 - lam)
        cut_h, cut_w = int(H * ratio), int(W * ratio)
        cy = r.randint(0, H)
        cx = r.randint(0, W)
        yl, yh = np.clip(cy - cut_h // 2, 0, H), np.clip(cy + cut_h // 2, 0, H)
        xl, xh = np.clip(cx - cut_w // 2, 0, W), np.clip(cx + cut_w // 2, 0, W)
        return yl, yh, xl, xh

    def _rand_bbox_minmax(self, H, W):
        r = self.rng
        lo, hi = self.cutmix_minmax
        cut_h = r.randint(int(H * lo), int(H * hi))
        cut_w = r.randint(int(W * lo), int(W * hi))
        yl = r.randint(0, H - cut_h)
        xl = r.randint(0, W - cut_w)
        return yl, yl + cut_h, xl, xl + cut_w

    def _bbox_and_lam(self, H, W, lam):
        if self.cutmix_minmax is not None:
            yl, yh, xl, xh = self._rand_bbox_minmax(H, W)
        else:
            yl, yh, xl, xh = self._rand_bbox(H, W, lam)
        if self.correct_lam or self.cutmix_minmax is not None:
            lam = 1. - (yh - yl) * (xh - xl) / float(H * W)
        return (int(yl), int(yh), int(xl), int(xh)), lam

    def _params_per_elem(self, n):
        r = self.rng
        lam = np.ones(n, dtype=np.float32)
        use_cutmix = np.zeros(n, dtype=bool)
        if self._active:
            if self.mixup_alpha > 0. and self.cutmix_alpha > 0.:
                use_cutmix = r.rand(n) < self.switch_prob
                lam_mix = np.where(use_cutmix, r.beta(self.cutmix_alpha, self.cutmix_alpha, size=n),
                                   r.beta(self.mixup_alpha, self.mixup_alpha, size=n))
            elif self.mixup_alpha > 0.:
                lam_mix = r.beta(self.mixup_alpha, self.mixup_alpha, size=n)
            else:
                use_cutmix = np.ones(n, dtype=bool)
                lam_mix = r.beta(self.cutmix_alpha, self.cutmix_alpha, size=n)
            lam = np.where(r.rand(n) < self.mix_prob, lam_mix.astype(np.float32), lam)
        return lam, use_cutmix

    def _params_per_batch(self):
        r = self.rng
        lam, use_cutmix = 1., False
        if self._active and r.rand() < self.mix_prob:
            if self.mixup_alpha > 0. and self.cutmix_alpha > 0.:
                use_cutmix = r.rand() < self.switch_prob
                lam_mix = r.beta(self.cutmix_alpha, self.cutmix_alpha) if use_cutmix else \
                    r.beta(self.mixup_alpha, self.mixup_alpha)
            elif self.mixup_alpha > 0.:
                lam_mix = r.beta(self.mixup_alpha, self.mixup_alpha)
            else:
                use_cutmix = True
                lam_mix = r.beta(self.cutmix_alpha, self.cutmix_alpha)
            lam = float(lam_mix)
        return lam, bool(use_cutmix)

    def draw(self, B, H, W):
        """One draw for a batch of B images of H x W: consumes the random stream exactly as timm's ``Mixup.__call__``."""
        B, H, W = int(B), int(H), int(W)
        if B <= 0 or B % 2 != 0:
            raise ValueError(f"Mixup: batch size should be even when using this, got {B}")
        p = MixParams.identity(B)
        p.partner = np.arange(B - 1, -1, -1, dtype=np.int32)
        if self.mode == "batch":
            lam, cut = self._params_per_batch()
            if lam != 1.:
                box = (0, 0, 0, 0)
                if cut:
                    box, lam = self._bbox_and_lam(H, W, lam)
                p.lam[:] = lam
                p.cut[:] = cut
                p.box[:] = box
        else:
            n = B if self.mode == "elem" else B // 2
            lam_batch, use_cutmix = self._params_per_elem(n)
            box = np.zeros((n, 4), dtype=np.int32)
            cut = np.zeros(n, dtype=bool)
            for i in range(n):
                lam = lam_batch[i]
                if lam != 1. and use_cutmix[i]:
                    box[i], lam = self._bbox_and_lam(H, W, lam)
                    lam_batch[i] = lam
                    cut[i] = True
            if self.mode == "pair":
                lam_batch = np.concatenate((lam_batch, lam_batch[::-1]))
                cut = np.concatenate((cut, cut[::-1]))
                box = np.concatenate((box, box[::-1]))
            p.lam[:], p.cut[:], p.box[:] = lam_batch, cut, box
        same = p.lam == 1.                              # (an f32 lam of 1: the kernels do not touch the sample)
        p.cut[same] = False
        p.box[same] = 0
        return p

    # ---- the device side -----------------------------------------------------------------------------------------------
    def apply(self, images, labels, params=None, out=None, binarize=False):
        """(mixed images, targets [B, num_classes] f32) for f32 images [B, C, H, W] and int64 labels [B] on the GPU.
        params: a ``MixParams`` (default: a fresh ``draw``); out: the buffer for the mixed images (must not overlap the
        input); binarize: ``targets.gt(0)`` as the recipe's BCE loss takes them."""
        ops._require_cuda(images)
        ops._require_cuda(labels)
        if images.dim() != 4:
            raise ValueError("Mixup.apply: images must be [B, C, H, W]")
        B, _, H, W = images.shape
        if params is None:
            params = self.draw(B, H, W)
        elif len(params) != B:
            raise ValueError("Mixup.apply: the parameters were drawn for another batch size")
        table = torch.from_numpy(params.table()).to(images.device)
        mixed = mix_images(images, table, out=out)
        on, off = self.on_off()
        return mixed, mix_targets(labels, table, self.num_classes, on=on, off=off, binarize=binarize)

    def __call__(self, x, target):
        """timm's call: a fresh draw, soft targets.  Out of place: returns the mixed batch, ``x`` is left alone."""
        return self.apply(x, target)


def mix_images(images, table, out=None):
    """The batch ``images`` (f32 [B, C, H, W]) mixed as the device ``table`` (``MixParams.table()`` on the GPU) says; a new
    tensor, or ``out``."""
    ops._require_cuda(images)
    if out is None:
        out = torch.empty_like(images, memory_format=torch.contiguous_format)
    return ops.mix_images(images, table, out)


def mix_targets(labels, table, num_classes, on=1.0, off=0.0, binarize=False, row0=0, rows=None, out=None):
    """Targets f32 [rows, num_classes] of the batch rows ``row0 .. row0 + rows - 1`` (default: all) from int64 ``labels`` [B]:
    ``lam onehot(y, on, off) + (1 - lam) onehot(y[partner], on, off)``, ``> 0`` when ``binarize``.  Partners are indexed in the
    whole batch.  A label outside [0, num_classes) gives an all-``off`` one-hot row."""
    ops._require_cuda(labels)
    rows = labels.numel() - row0 if rows is None else rows
    if out is None:
        out = torch.empty(rows, num_classes, dtype=torch.float32, device=labels.device)
    return ops.mix_targets(labels, table, num_classes, on, off, binarize, out, row0=row0)


class _MixBceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, table, on, off, binarize, row0):
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        ws = torch.empty(logits.shape[0], dtype=torch.float64, device=logits.device)
        ops.mix_bce(logits, labels, table, on, off, binarize, row0=row0, loss=loss, workspace=ws)
        ctx.save_for_backward(logits, labels, table)
        ctx.args = (on, off, binarize, row0)
        return loss

    @staticmethod
    def backward(ctx, grad):
        logits, labels, table = ctx.saved_tensors
        on, off, binarize, row0 = ctx.args
        # the incoming gradient stays on the device: the kernel multiplies by it (no host read, capturable)
        g = grad.to(torch.float32).reshape(1).contiguous()
        d = torch.empty(logits.shape, dtype=logits.dtype, device=logits.device)
        ops.mix_bce(logits, labels, table, on, off, binarize, row0=row0, gscale=g, dlogits=d)
        return d, None, None, None, None, None, None


def mix_bce_loss(logits, labels, table, on=1.0, off=0.0, binarize=True, row0=0):
    """``nn.BCEWithLogitsLoss()(logits.float(), targets)`` for the targets ``mix_targets(labels, table, C, on, off, binarize,
    row0, rows)`` without materialising them; logits f32 or bf16 [rows, C], differentiable in the logits (the gradient comes
    back in their dtype, scaled by the incoming gradient on the device)."""
    ops._require_cuda(logits)
    if logits.dim() != 2:
        raise ValueError("mix_bce_loss: logits must be [rows, num_classes]")
    if logits.stride(1) != 1:
        logits = logits.contiguous()
    return _MixBceFn.apply(logits, labels, table, float(on), float(off), bool(binarize), int(row0))


def smoothing_on_off(smoothing, num_classes):
    """timm's one-hot values for label smoothing ``s`` over C classes: ``off = s / C``, ``on = 1 - s + off``; returns (on, off).
    ``mix_ce_loss`` with these and the identity table (``MixParams.identity(B)``) is ``LabelSmoothingCrossEntropy(s)``, at
    ``s = 0`` plain cross entropy."""
    off = smoothing / num_classes
    return 1. - smoothing + off, off


def _loss_logits(what, logits, rows_multiple=1):
    ops._require_cuda(logits)
    if logits.dim() != 2 or logits.shape[0] % rows_multiple:
        raise ValueError(f"{what}: logits must be [{'2 ' if rows_multiple == 2 else ''}rows, num_classes]")
    return logits if logits.stride(1) == 1 else logits.contiguous()


class _MixCeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, table, on, off, row0):
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        ws = torch.empty(logits.shape[0], dtype=torch.float64, device=logits.device)
        ops.mix_ce(logits, labels, table, on, off, row0=row0, loss=loss, workspace=ws)
        ctx.save_for_backward(logits, labels, table)
        ctx.args = (on, off, row0)
        return loss

    @staticmethod
    def backward(ctx, grad):
        logits, labels, table = ctx.saved_tensors
        on, off, row0 = ctx.args
        g = grad.to(torch.float32).reshape(1).contiguous()     # (stays on the device, as in _MixBceFn)
        d = torch.empty(logits.shape, dtype=logits.dtype, device=logits.device)
        ops.mix_ce(logits, labels, table, on, off, row0=row0, gscale=g, dlogits=d)
        return d, None, None, None, None, None


def mix_ce_loss(logits, labels, table, on=1.0, off=0.0, row0=0):
    """timm's ``SoftTargetCrossEntropy()(logits.float(), targets)`` = ``sum(-targets * log_softmax(logits), -1).mean()`` for the
    NON-binarised targets ``mix_targets(labels, table, C, on, off, False, row0, rows)`` without materialising them; logits f32 or
    bf16 [rows, C], differentiable in the logits (the gradient comes back in their dtype, scaled by the incoming gradient on the
    device).  With the identity table and ``smoothing_on_off(s, C)`` it is ``LabelSmoothingCrossEntropy(s)``."""
    logits = _loss_logits("mix_ce_loss", logits)
    return _MixCeFn.apply(logits, labels, table, float(on), float(off), int(row0))


class _CosubBceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, table, on, off, binarize, row0):
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        ws = torch.empty(logits.shape[0] // 2, dtype=torch.float64, device=logits.device)
        ops.cosub_bce(logits, labels, table, on, off, binarize, row0=row0, loss=loss, workspace=ws)
        ctx.save_for_backward(logits, labels, table)
        ctx.args = (on, off, binarize, row0)
        return loss

    @staticmethod
    def backward(ctx, grad):
        logits, labels, table = ctx.saved_tensors
        on, off, binarize, row0 = ctx.args
        g = grad.to(torch.float32).reshape(1).contiguous()
        d = torch.empty(logits.shape, dtype=logits.dtype, device=logits.device)
        ops.cosub_bce(logits, labels, table, on, off, binarize, row0=row0, gscale=g, dlogits=d)
        return d, None, None, None, None, None, None


def cosub_bce_loss(logits, labels, table, on, off, binarize, row0=0):
    """The loss of the reference's ``--cosub`` (deit/engine.py:60-65) for logits [2 rows, C] of a batch that was doubled with
    ``torch.cat((x, x))`` - ``a, b = logits.chunk(2)`` are the two stochastic-depth passes of the same samples:
    ``0.25 (bce(a, t) + bce(b, t) + bce(a, sigmoid(b).detach()) + bce(b, sigmoid(a).detach()))`` with ``bce`` =
    ``nn.BCEWithLogitsLoss()`` and t the targets ``mix_targets(labels, table, C, on, off, binarize, row0, rows)``, never
    materialised.  One launch for the value, one for both halves' gradient (in the logits' dtype)."""
    logits = _loss_logits("cosub_bce_loss", logits, 2)
    return _CosubBceFn.apply(logits, labels, table, float(on), float(off), bool(binarize), int(row0))


class TableUploader:
    """The device table of one batch size and its refills without a stream drain: ``slots`` pinned host tables in rotation,
    each guarded by an event recorded behind its H2D copy - a slot is rewritten only after its copy has executed, so the
    host may run several steps ahead of the device (as ``FusedLamb.push_hyper`` does for the schedules).  ``table`` keeps its
    address: a captured step reads it at every replay."""

    def __init__(self, B, device, slots=4):
        self.table = torch.from_numpy(MixParams.identity(B).table()).to(device)
        self._ring = [[torch.empty(B, 8, dtype=torch.int32).pin_memory(), None] for _ in range(slots)]
        self._i = 0

    def upload(self, params):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("TableUploader.upload: not while a stream is capturing (upload in front of the replay)")
        slot = self._ring[self._i]
        self._i = (self._i + 1) % len(self._ring)
        if slot[1] is not None:
            slot[1].synchronize()
        slot[0].copy_(torch.from_numpy(params.table()))
        self.table.copy_(slot[0], non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record()
        return self.table
