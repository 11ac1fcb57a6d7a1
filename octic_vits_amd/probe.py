"""Linear-probe evaluation of a frozen DINOv2 backbone on the HIP engine (reference: experiments/eval_dinov2_classification.py
-> dinov2/eval/linear.py).

The reference trains a GRID of linear classifiers on frozen features: learning rates x ``n_last_blocks`` x ``avgpool``
(linear.py:237-258), all of them in every iteration, with ``torch.optim.SGD(momentum=0.9, weight_decay=0)`` under
``CosineAnnealingLR`` (linear.py:344-366, 519-521), and reports the best classifier's top-1 accuracy on the validation
set (linear.py:262-312).  Here the grid is four launches per iteration (csrc/probe.hip):

* every classifier's input is a column range of ONE f32 feature row ``[cls(L-4) | cls(L-3) | cls(L-2) | cls(L-1) |
  mean patch(L-1)]`` - no concatenation is materialised (``create_linear_input`` below is the plain-torch statement of
  the same thing and works on CPU tensors);
* the weight gradient is formed per tile of ``W`` in registers and applied at once (momentum + update): it never goes to
  memory.

Naming follows the reference's own format expression INCLUDING ITS COLLISIONS: at batch 128 on one GPU the scaled rates
5e-6 and 1e-5 both print as ``0_00001``; the later classifier replaces the earlier one in the ``ModuleDict`` (keeping the
earlier one's position), so the reference trains 48 heads while its optimizer holds 52 parameter groups, four of them
orphaned.  ``classifier_grid`` does the same; the orphaned groups are not materialised (they own no classifier anybody
can evaluate)."""
import gc
from collections import OrderedDict

import numpy as np
import torch

DEFAULT_LEARNING_RATES = (1e-5, 2e-5, 5e-5, 1e-4, 2e-4, 5e-4, 1e-3, 2e-3, 5e-3, 1e-2, 2e-2, 5e-2, 0.1)
STATE_PREFIX = "classifiers_dict."


def create_linear_input(x_tokens_list, use_n_blocks, use_avgpool):
    """linear.py:173-185.  x_tokens_list: (patch tokens [B, P, D], class token [B, D]) per block, oldest first."""
    last = x_tokens_list[-use_n_blocks:]
    parts = [cls for _, cls in last]
    if use_avgpool:
        parts.append(last[-1][0].mean(dim=1))
    out = torch.cat(parts, dim=-1)
    return out.reshape(out.shape[0], -1).float()


def scale_lr(learning_rate, batch_size, world_size=1):
    """linear.py:233-234: the rate for a global batch of 256, scaled linearly."""
    return learning_rate * (batch_size * world_size) / 256.0


def classifier_name(n_blocks, avgpool, lr):
    return f"classifier_{n_blocks}_blocks_avgpool_{avgpool}_lr_{lr:.5f}".replace(".", "_")


def classifier_grid(embed_dim, n_last_blocks_list=(1, 4), learning_rates=DEFAULT_LEARNING_RATES, batch_size=128, world_size=1):
    """The classifiers setup_linear_classifiers would train, in its ModuleDict's order: name -> dict(n_blocks, avgpool, lr,
    out_dim).  Returns (heads, n_groups): n_groups counts the parameter groups the reference's optimizer would hold
    (one per loop iteration, orphaned ones included)."""
    heads, n_groups = OrderedDict(), 0
    for n in n_last_blocks_list:
        for avgpool in (False, True):
            for base in learning_rates:
                lr = scale_lr(base, batch_size, world_size)
                # a repeated name replaces the entry and keeps the first one's position (dict semantics)
                heads[classifier_name(n, avgpool, lr)] = dict(n_blocks=n, avgpool=avgpool, lr=lr,
                                                              out_dim=(n + int(avgpool)) * embed_dim)
                n_groups += 1
    return heads, n_groups


_HEAD_DTYPE = np.dtype([("w", "<u8"), ("b", "<u8"), ("mw", "<u8"), ("mb", "<u8"), ("col0", "<i4"), ("K", "<i4"),
                        ("lr_index", "<i4"), ("tile0", "<i4")])     # octic_probe_head (include/octic_hip.h)


class LinearProbe:
    """The classifier grid on top of ``model`` (anything with ``get_intermediate_layers`` and ``embed_dim``: the hybrid /
    invariant DINOv2 factories and the ``dinov2_vit`` baselines, with or without register tokens).

    Weights and momentum live in two flat f32 buffers (``flat`` / ``momentum``; all weight matrices, then all biases) with one
    ``[C, K]`` view per classifier in ``weights[name]`` / ``biases[name]``.  ``state_dict`` / ``load_state_dict`` use the
    reference's keys (``classifiers_dict.<name>.linear.weight|bias``), so classifier checkpoints move both ways."""

    def __init__(self, model, n_last_blocks_list=(1, 4), learning_rates=DEFAULT_LEARNING_RATES, batch_size=128, num_classes=1000,
                 autocast_dtype=torch.bfloat16, world_size=1, device=None, generator=None, embed_dim=None):
        self.model = model                       # None (with embed_dim=): a probe on resident feature rows only
        self.autocast_dtype = autocast_dtype
        self.batch_size, self.num_classes = int(batch_size), int(num_classes)
        D = self.embed_dim = int(model.embed_dim if model is not None else embed_dim)
        if D % 64:
            raise ValueError(f"LinearProbe: embed_dim {D} must be a multiple of 64")
        self.n_blocks = max(n_last_blocks_list)
        if not 1 <= self.n_blocks <= 4 or min(n_last_blocks_list) < 1:
            raise ValueError("LinearProbe: n_last_blocks within 1 .. 4")
        self.heads, self.n_reference_groups = classifier_grid(D, n_last_blocks_list, learning_rates, batch_size, world_size)
        self.names = list(self.heads)
        if device is None:
            device = next(self.model.parameters()).device if self.model is not None else torch.device("cpu")
        self.device = torch.device(device)
        C, nh = self.num_classes, len(self.names)
        self.width = (self.n_blocks + 1) * D
        self.sum_k = sum(h["out_dim"] for h in self.heads.values())
        self.total_ktiles = self.sum_k // 64
        n_w = C * self.sum_k
        self.flat = torch.zeros(n_w + nh * C, dtype=torch.float32, device=self.device)
        self.momentum = torch.zeros_like(self.flat)
        self.weights, self.biases, self.momentum_w, self.momentum_b = OrderedDict(), OrderedDict(), OrderedDict(), OrderedDict()
        off = 0
        for i, (name, h) in enumerate(self.heads.items()):
            K = h["out_dim"]
            h["col0"] = (self.n_blocks - h["n_blocks"]) * D
            self.weights[name] = self.flat[off:off + C * K].view(C, K)
            self.momentum_w[name] = self.momentum[off:off + C * K].view(C, K)
            self.biases[name] = self.flat[n_w + i * C:n_w + (i + 1) * C]
            self.momentum_b[name] = self.momentum[n_w + i * C:n_w + (i + 1) * C]
            off += C * K
            self.weights[name].normal_(mean=0.0, std=0.01, generator=generator)     # LinearClassifier.__init__
        self.lr = torch.zeros(nh, dtype=torch.float32, device=self.device)
        self.optimizer = None
        self._cap = 0
        self._table = None
        self._have_grad, self._last_F = False, None
        if self.device.type == "cuda":
            tab = np.zeros(nh, dtype=_HEAD_DTYPE)
            tile0 = 0
            for i, (name, h) in enumerate(self.heads.items()):
                tab[i] = (self.weights[name].data_ptr(), self.biases[name].data_ptr(), self.momentum_w[name].data_ptr(),
                          self.momentum_b[name].data_ptr(), h["col0"], h["out_dim"], i, tile0)
                tile0 += h["out_dim"] // 64
            self._table = torch.from_numpy(tab.view(np.uint8).copy()).to(self.device)
            self.loss = torch.zeros(nh, dtype=torch.float32, device=self.device)          # per-classifier batch mean
            self.loss_sum = torch.zeros(nh, dtype=torch.float32, device=self.device)      # evaluation accumulators
            self.topk = torch.zeros(nh, 2, dtype=torch.int32, device=self.device)
            self._reserve(self.batch_size)

    def __len__(self):
        return len(self.names)

    # ------------------------------------------------------------------------------------------ buffers
    def _reserve(self, B):
        if B <= self._cap:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("LinearProbe: a batch larger than the reserved buffers during graph capture")
        nh, C = len(self.names), self.num_classes
        self.features = torch.zeros(B, self.width, dtype=torch.float32, device=self.device)
        self._logits = torch.empty(nh * B * C, dtype=torch.float32, device=self.device)
        self._dlogits = torch.empty(nh * B * C, dtype=torch.float32, device=self.device)
        self._rowloss = torch.empty(nh * B, dtype=torch.float32, device=self.device)
        self._rowrank = torch.empty(nh * B, dtype=torch.int32, device=self.device)
        self._cap = B

    def _need_gpu(self):
        if self._table is None:
            raise RuntimeError("LinearProbe: the probe kernels run on the GPU only (no CPU fallback)")

    def logits(self, B):
        """The last forward's logits as [classifiers, B, C] (a view of the probe's buffer)."""
        nh, C = len(self.names), self.num_classes
        return self._logits[:nh * B * C].view(nh, B, C)

    def dlogits(self, B):
        nh, C = len(self.names), self.num_classes
        return self._dlogits[:nh * B * C].view(nh, B, C)

    # ------------------------------------------------------------------------------------------ stages
    def extract(self, images):
        """Backbone forward in eval mode (no_grad, autocast) and the feature kernel: returns the [B, (n+1) D] f32 rows (a
        view of the probe's own buffer).  no_grad rather than inference_mode, as serve.GraphedForward: the octic blocks key
        their cached compute-dtype copies on tensor version counters, which inference tensors do not have."""
        self._need_gpu()
        if self.model is None:
            raise RuntimeError("LinearProbe: built without a backbone (feature rows only)")
        self.model.eval()
        B = images.shape[0]
        self._reserve(B)
        with torch.no_grad():
            if self.autocast_dtype is None:
                pairs = self.model.get_intermediate_layers(images, self.n_blocks, return_class_token=True)
            else:
                with torch.autocast("cuda", dtype=self.autocast_dtype):
                    pairs = self.model.get_intermediate_layers(images, self.n_blocks, return_class_token=True)
            return self.features_from_tokens(pairs)

    def features_from_tokens(self, pairs):
        from . import ops
        self._need_gpu()
        B = pairs[-1][0].shape[0]
        self._reserve(B)
        if len(pairs) != self.n_blocks or pairs[-1][0].shape[-1] != self.embed_dim:
            raise ValueError(f"LinearProbe: expected {self.n_blocks} (patch tokens, class token) pairs of width {self.embed_dim}")
        F = self.features[:B]
        ops.probe_features(pairs, F)
        return F

    def _check_features(self, F):
        if (not F.is_cuda or F.dtype != torch.float32 or F.dim() != 2 or F.shape[1] != self.width or F.stride(1) != 1
                or F.stride(0) % 4 or F.data_ptr() % 16):
            raise ValueError(f"LinearProbe: features must be a CUDA f32 [B, {self.width}] tensor with 16-byte aligned rows")

    def forward_features(self, F):
        """All classifiers on feature rows F: logits [classifiers, B, C]."""
        from . import ops
        self._need_gpu()
        self._check_features(F)
        B = F.shape[0]
        self._reserve(B)
        ops.probe_forward(self._table, len(self.names), F, B, self.num_classes, self._logits, self.sum_k)
        self._last_F = F
        return self.logits(B)

    def loss_and_grad(self, labels, B, train=True):
        """Cross entropy of the last logits.  train: writes dlogits and ``self.loss`` (batch means); else accumulates the
        evaluation counters (``loss_sum``, ``topk``)."""
        from . import ops
        nh = len(self.names)
        if train:
            ops.probe_ce(self._logits, labels, nh, B, self.num_classes, self._dlogits, self._rowloss, self._rowrank,
                         loss_mean=self.loss)
            self._grad_F, self._grad_B, self._have_grad = self._last_F, B, True
        else:
            ops.probe_ce(self._logits, labels, nh, B, self.num_classes, None, self._rowloss, self._rowrank,
                         loss_sum=self.loss_sum, topk=self.topk)

    def step_features(self, F, labels):
        """One training iteration on resident feature rows: forward, cross entropy, fused gradient + SGD update.  Returns
        the per-classifier losses (device tensor, overwritten by the next step; no synchronisation)."""
        if self.optimizer is None:
            raise RuntimeError("LinearProbe.step: build a ProbeSGD(probe) first")
        self.forward_features(F)
        self.loss_and_grad(labels, F.shape[0], train=True)
        self.optimizer.step()
        return self.loss

    def step(self, images, labels):
        """linear.py:351-365 for one batch: frozen backbone -> features -> classifiers -> cross entropy -> SGD."""
        return self.step_features(self.extract(images), labels)

    def capture(self, example_images, example_labels, warmup=2):
        """Record ``step`` once as a hipGraph on one stream; returns a callable ``replay(images, labels)``."""
        return CapturedProbeStep(self, example_images, example_labels, warmup)

    # ------------------------------------------------------------------------------------------ evaluation
    def evaluate(self, batches, metric_type="mean_accuracy", class_mapping=None, on_features=False):
        """evaluate_linear_classifiers (linear.py:262-312) for MetricType.MEAN_ACCURACY: top-1 / top-5 per classifier from
        device counters (one read-back at the end; batches may differ in size) and the reference's best-classifier rule:
        the first strict maximum of top-1 in dictionary order, starting from 0.  batches: iterable of (images, labels), or
        of (feature rows, labels) with on_features=True."""
        if str(getattr(metric_type, "value", metric_type)) != "mean_accuracy":
            raise NotImplementedError(f"LinearProbe.evaluate: metric type {metric_type!r} (only mean_accuracy; every other type "
                                      "is octic_vits_amd.metrics.evaluate_linear_classifiers)")
        if class_mapping is not None:
            raise NotImplementedError("LinearProbe.evaluate: class mappings (octic_vits_amd.metrics.evaluate_linear_classifiers "
                                      "takes one)")
        self._need_gpu()
        self.loss_sum.zero_()
        self.topk.zero_()
        n = 0
        for x, labels in batches:
            F = x if on_features else self.extract(x)
            self.forward_features(F)
            self.loss_and_grad(labels, F.shape[0], train=False)
            n += F.shape[0]
        topk = self.topk.cpu()
        loss = self.loss_sum.cpu()
        results, best, best_acc = OrderedDict(), "", 0
        for i, name in enumerate(self.names):
            top1 = topk[i, 0].item() / max(n, 1)
            results[name] = {"top-1": top1, "top-5": topk[i, 1].item() / max(n, 1), "loss": loss[i].item() / max(n, 1)}
            if top1 > best_acc:
                best, best_acc = name, top1
        return {"best_classifier": {"name": best, "accuracy": best_acc}, "classifiers": results, "samples": n}

    # ------------------------------------------------------------------------------------------ checkpoints
    def state_dict(self):
        sd = OrderedDict()
        for name in self.names:
            sd[f"{STATE_PREFIX}{name}.linear.weight"] = self.weights[name].detach().clone()
            sd[f"{STATE_PREFIX}{name}.linear.bias"] = self.biases[name].detach().clone()
        return sd

    def load_state_dict(self, sd):
        sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
        want = set(self.state_dict_keys())
        if set(sd) != want:
            raise KeyError(f"LinearProbe.load_state_dict: missing {sorted(want - set(sd))[:3]}, unexpected {sorted(set(sd) - want)[:3]}")
        for name in self.names:
            self.weights[name].copy_(sd[f"{STATE_PREFIX}{name}.linear.weight"])
            self.biases[name].copy_(sd[f"{STATE_PREFIX}{name}.linear.bias"])

    def state_dict_keys(self):
        return [f"{STATE_PREFIX}{name}.linear.{p}" for name in self.names for p in ("weight", "bias")]


class ProbeSGD(torch.optim.Optimizer):
    """torch.optim.SGD(momentum, weight_decay=0) for a LinearProbe, as the fused gradient + update kernel.  One parameter group
    per classifier (``"lr"``, ``"name"``), so ``torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, max_iter, eta_min=0)``
    drives it unchanged.  ``step()`` uploads the groups' rates when they changed - the host's float64 rate rounded once to f32,
    through a pinned slot and a stream-ordered copy, never while the stream is capturing (a captured step reads the rates when
    it is replayed; ``CapturedProbeStep`` uploads in front of every replay) - and launches the kernel on the gradient of the
    probe's last cross entropy."""

    def __init__(self, probe, momentum=0.9):
        self.probe = probe
        groups = [{"params": [probe.weights[n], probe.biases[n]], "lr": probe.heads[n]["lr"], "name": n} for n in probe.names]
        super().__init__(groups, dict(lr=0.0, momentum=momentum))
        self._key, self._ring, self._ring_i = None, None, 0
        probe.optimizer = self

    def push_lr(self):
        key = tuple(float(g["lr"]) for g in self.param_groups)
        if key == self._key or torch.cuda.is_current_stream_capturing():
            return False
        if self._ring is None:
            self._ring = [[torch.empty(len(key), dtype=torch.float32).pin_memory(), None] for _ in range(4)]
        slot = self._ring[self._ring_i]
        self._ring_i = (self._ring_i + 1) % len(self._ring)
        if slot[1] is not None:
            slot[1].synchronize()
        slot[0].copy_(torch.tensor(key, dtype=torch.float64))
        self.probe.lr.copy_(slot[0], non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record()
        self._key = key
        return True

    @torch.no_grad()
    def step(self, closure=None):
        from . import ops
        p = self.probe
        p._need_gpu()
        if closure is not None:
            raise NotImplementedError("ProbeSGD.step: closures")
        if not p._have_grad:
            raise RuntimeError("ProbeSGD.step: no gradient - run LinearProbe.step / loss_and_grad first")
        momenta = {float(g["momentum"]) for g in self.param_groups}
        if len(momenta) != 1:
            raise ValueError("ProbeSGD: one momentum for all classifiers")
        self.push_lr()
        ops.probe_sgd(p._table, len(p.names), p.total_ktiles, p._grad_F, p._dlogits, p._grad_B, p.num_classes, p.lr,
                      momenta.pop(), p.sum_k)
        if not torch.cuda.is_current_stream_capturing():
            p._have_grad = False

    def zero_grad(self, set_to_none=True):
        self.probe._have_grad = False

    def state_dict(self):
        return {"momentum_buffer": self.probe.momentum.detach().clone(),
                "param_groups": [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups]}

    def load_state_dict(self, sd):
        if [g["name"] for g in sd["param_groups"]] != self.probe.names:
            raise KeyError("ProbeSGD.load_state_dict: the classifier names differ")
        self.probe.momentum.copy_(sd["momentum_buffer"])
        for g, s in zip(self.param_groups, sd["param_groups"]):
            g.update(s)
        self._key = None


class CapturedProbeStep:
    """``LinearProbe.step`` as one hipGraph replay (static shapes), the training-side sibling of ``serve.GraphedForward``:
    images and labels are copied into the graph's inputs, the learning rates into the device buffer the update kernel reads.
    Refuses other shapes, a backbone whose parameters changed since the capture (the graph reads frozen compute-dtype copies
    of them) and a backbone switched to training mode."""

    def __init__(self, probe, images, labels, warmup=2):
        if not images.is_cuda or probe.optimizer is None:
            raise RuntimeError("CapturedProbeStep: CUDA example inputs and a ProbeSGD are required")
        self.probe = probe
        self.images = images.detach().clone()
        self.labels = labels.detach().clone()
        dev = images.device
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(max(1, warmup)):       # fills the backbone's weight caches; the classifiers are not touched
                probe.extract(self.images)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        probe.optimizer.push_lr()
        gc.collect()                              # (as serve.GraphedForward: no collection of dead graphs inside the capture)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.loss = probe.step(self.images, self.labels)
        probe._have_grad = False
        self._stamp = self._param_stamp()

    def _param_stamp(self):
        return tuple((p.data_ptr(), p._version) for p in self.probe.model.parameters())

    def __call__(self, images, labels):
        if images.shape != self.images.shape or images.dtype != self.images.dtype or labels.shape != self.labels.shape:
            raise ValueError(f"CapturedProbeStep: input {tuple(images.shape)} {images.dtype} / labels {tuple(labels.shape)} differ "
                             f"from the captured {tuple(self.images.shape)} {self.images.dtype} / {tuple(self.labels.shape)}")
        if self._param_stamp() != self._stamp:
            raise RuntimeError("CapturedProbeStep: the backbone's parameters changed since the capture - capture again")
        if self.probe.model.training:
            raise RuntimeError("CapturedProbeStep: the backbone was switched to training mode")
        self.images.copy_(images, non_blocking=True)
        self.labels.copy_(labels, non_blocking=True)
        self.probe.optimizer.push_lr()
        self.graph.replay()
        return self.loss

    replay = __call__
