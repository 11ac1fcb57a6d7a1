"""The accuracies of the reference's evaluations (dinov2/eval/metrics.py) from device counters, on the kernels of
csrc/topk_metric.hip: mean (micro) accuracy, mean-per-class and per-class accuracy, ImageNet-ReaL (multi-label targets padded
with -1) and the class mapping of ``linear.py``'s ``LinearPostprocessor`` (``preds[:, class_mapping]``: ImageNet-A / -R score a
200-class subset of the 1000 logits).  ``LinearProbe.evaluate`` and ``knn.eval_knn*`` report MEAN_ACCURACY on the training label
space only; the entry points here stand beside them and take every metric type, every averaging and a mapping.

``TopkAccuracy`` is the metric: ``update(scores, targets)`` ranks every target among its row's candidates (``ops.topk_rank``, one
wave per row, all groups - classifiers, or values of k - in one launch) and adds the hits to int64 counters on the device
(``ops.topk_count``); nothing is read back until ``compute()``, which forms every ratio on the host in float64 from the integers.

What is ours, not the reference's: the order of EQUAL scores, which ``torch.topk`` (under torchmetrics' ``select_topk``) leaves
open.  ``tie="strict"`` counts the scores strictly greater than the target's, so a tied target is a hit (``octic_probe_ce``'s
rule, what ``LinearProbe.evaluate`` reports); ``tie="index"`` puts the lower class index first (``octic_knn_vote``'s rule; most
k-NN probas are exact zeros).  On rows of pairwise distinct scores both agree with the reference.  A NaN score counts as -inf.

``zero_support``: whether a class without a single sample is left out of the mean per class (``"exclude"``, the default) or
enters it as 0 (``"zero"``).  torchmetrics has done both across its versions, it is not a dependency of this package and the
reference pins no version; the two rules agree whenever every class has a sample, which holds for every set the reference
evaluates.  The per-class vector itself is hits / support with 0 where the support is 0 (torchmetrics' ``_safe_divide``) under
both.  A ratio whose denominator is 0 (nothing accumulated, or ReaL rows without any defined target only) is 0.0."""
from collections import OrderedDict
from enum import Enum

import torch

from . import knn as _knn


class MetricType(Enum):
    MEAN_ACCURACY = "mean_accuracy"
    MEAN_PER_CLASS_ACCURACY = "mean_per_class_accuracy"
    PER_CLASS_ACCURACY = "per_class_accuracy"
    IMAGENET_REAL_ACCURACY = "imagenet_real_accuracy"

    @property
    def accuracy_averaging(self):
        return getattr(AccuracyAveraging, self.name, None)

    def __str__(self):
        return self.value


class AccuracyAveraging(Enum):
    MEAN_ACCURACY = "micro"
    MEAN_PER_CLASS_ACCURACY = "macro"
    PER_CLASS_ACCURACY = "none"

    def __str__(self):
        return self.value


MAX_KS = 8                    # the counters of one launch: octic_topk_count's nk
MAX_TARGETS = 32              # ops.TOPK_MAX_TARGETS
_TIES = {"strict": 0, "index": 1}            # ops.TOPK_ORDER_STRICT / TOPK_ORDER_INDEX


def as_metric_type(metric_type):
    """MetricType from the enum, its value ("mean_accuracy") or its name ("MEAN_ACCURACY")."""
    if isinstance(metric_type, MetricType):
        return metric_type
    key = str(getattr(metric_type, "value", metric_type))
    for m in MetricType:
        if key in (m.value, m.name):
            return m
    raise ValueError(f"octic_vits_amd.metrics: unknown metric type {metric_type!r}")


def as_accuracy_averaging(averaging):
    """AccuracyAveraging from the enum, a name ("mean_per_class_accuracy", any case; a MetricType that has one) or a value
    ("macro")."""
    if isinstance(averaging, AccuracyAveraging):
        return averaging
    if isinstance(averaging, MetricType):
        if averaging.accuracy_averaging is None:
            raise ValueError(f"octic_vits_amd.metrics: {averaging} has no accuracy averaging")
        return averaging.accuracy_averaging
    key = str(getattr(averaging, "value", averaging))
    for a in AccuracyAveraging:
        if key == a.value or key.upper() == a.name:
            return a
    raise ValueError(f"octic_vits_amd.metrics: unknown accuracy averaging {averaging!r}")


def check_ks(ks):
    ks = tuple(int(k) for k in ks)
    if not ks or len(ks) > MAX_KS or ks[0] < 1 or any(b <= a for a, b in zip(ks, ks[1:])):
        raise ValueError(f"octic_vits_amd.metrics: ks must be 1 .. {MAX_KS} strictly ascending values >= 1, got {ks}")
    return ks


def check_class_mapping(class_mapping, num_columns=None):
    """The mapping as a CPU int32 [Cm] tensor; ValueError unless it is a non-empty 1-d list of integers in [0, num_columns)
    (num_columns None: only >= 0 is checked - the width of the scores is known at the first update)."""
    m = torch.as_tensor(class_mapping).detach().cpu()
    if m.dim() != 1 or not m.numel() or m.dtype.is_floating_point or m.dtype.is_complex or m.dtype == torch.bool:
        raise ValueError("octic_vits_amd.metrics: class_mapping must be a non-empty 1-d sequence of integers")
    m = m.long()
    hi = int(m.max())
    if int(m.min()) < 0 or (num_columns is not None and hi >= num_columns) or hi >= 2 ** 31:
        raise ValueError(f"octic_vits_amd.metrics: class_mapping entries must lie in [0, {num_columns if num_columns is not None else '2^31'}), "
                         f"got {int(m.min())} .. {hi}")
    return m.int().contiguous()


def _safe_divide(num, den):
    """num / den in float64 with 0 where den == 0 (torchmetrics' _safe_divide)."""
    num, den = num.double(), den.double()
    return torch.where(den == 0, torch.zeros_like(num), num / torch.where(den == 0, torch.ones_like(den), den))


def accuracies_from_counters(metric_type, counters, ks, zero_support="exclude"):
    """The values of ``TopkAccuracy.compute`` from the integer counters of ONE group: int64 [1 + len(ks)] (rows with a defined
    target, hits per k) for MEAN_ACCURACY / IMAGENET_REAL_ACCURACY, int64 [Cm, 1 + len(ks)] (support, hits per k of every class)
    for the per-class types.  Returns {"top-k": float}, or {"top-k": float64 [Cm] tensor} for PER_CLASS_ACCURACY."""
    metric_type, ks = as_metric_type(metric_type), check_ks(ks)
    if zero_support not in ("exclude", "zero"):
        raise ValueError('octic_vits_amd.metrics: zero_support is "exclude" or "zero"')
    c = torch.as_tensor(counters).cpu().long()
    per_class = metric_type in (MetricType.MEAN_PER_CLASS_ACCURACY, MetricType.PER_CLASS_ACCURACY)
    if c.dim() != (2 if per_class else 1) or c.shape[-1] != 1 + len(ks):
        raise ValueError(f"octic_vits_amd.metrics: counters of {metric_type} must be "
                         f"{'[classes, 1 + len(ks)]' if per_class else '[1 + len(ks)]'}, got {list(c.shape)}")
    out = OrderedDict()
    for i, k in enumerate(ks):
        if not per_class:
            rows, hits = int(c[0]), int(c[1 + i])
            out[f"top-{k}"] = hits / rows if rows else 0.0
            continue
        support = c[:, 0]
        acc = _safe_divide(c[:, 1 + i], support)
        if metric_type == MetricType.PER_CLASS_ACCURACY:
            out[f"top-{k}"] = acc
        else:
            classes = int((support > 0).sum()) if zero_support == "exclude" else int(support.numel())
            out[f"top-{k}"] = float(acc.sum()) / classes if classes else 0.0
    return out


class TopkAccuracy:
    """Top-k accuracies of ``groups`` score tensors that share their targets (the classifiers of a probe, the values of k of a
    k-NN module), accumulated on the device.

    ``num_classes`` is the metric's label space: the length of ``class_mapping`` where one is given, else the width of the
    scores.  ``update(scores, targets)``: scores f32 ``[n, C]`` (one group) or ``[groups, n, C]`` with unit column stride (any
    row / group stride - views are not copied); targets integer ``[n]`` or ``[n, A]`` (A <= 32; only IMAGENET_REAL_ACCURACY
    takes A > 1), a value outside ``[0, num_classes)`` - the reference pads with -1 - being an undefined target.  ``rank`` holds
    the int32 ``[groups, n, A]`` ranks of the last update, ``counters`` the int64 device counters."""

    def __init__(self, metric_type, num_classes, ks=(1, 5), groups=1, class_mapping=None, tie="strict", zero_support="exclude",
                 device=None):
        self.metric_type = as_metric_type(metric_type)
        self.num_classes, self.groups = int(num_classes), int(groups)
        self.ks = check_ks(ks)
        if self.num_classes < 1 or self.groups < 1:
            raise ValueError("TopkAccuracy: num_classes and groups must be positive")
        if tie not in _TIES:
            raise ValueError('TopkAccuracy: tie is "strict" or "index"')
        if zero_support not in ("exclude", "zero"):
            raise ValueError('TopkAccuracy: zero_support is "exclude" or "zero"')
        self.tie, self.zero_support = tie, zero_support
        self.class_mapping = None if class_mapping is None else check_class_mapping(class_mapping)
        if self.class_mapping is not None and self.class_mapping.numel() != self.num_classes:
            raise ValueError(f"TopkAccuracy: num_classes {self.num_classes} differs from the {self.class_mapping.numel()} mapped classes")
        self.per_class = self.metric_type in (MetricType.MEAN_PER_CLASS_ACCURACY, MetricType.PER_CLASS_ACCURACY)
        self.device = None
        self.counters = self.rank = self._map = None
        self._map_columns = None
        if device is not None:
            self._bind(torch.device(device))

    def _bind(self, device):
        if device.type != "cuda":
            raise RuntimeError("octic_vits_amd.metrics.TopkAccuracy runs on the GPU only (no CPU fallback)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self.device is not None and device != self.device:
            raise ValueError(f"TopkAccuracy: scores on {device}, counters on {self.device}")
        if self.device is None:
            self.device = device
            shape = (self.groups, self.num_classes, 1 + len(self.ks)) if self.per_class else (self.groups, 1 + len(self.ks))
            self.counters = torch.zeros(shape, dtype=torch.int64, device=device)
            if self.class_mapping is not None:
                self._map = self.class_mapping.to(device)

    def check(self, scores, targets):
        """(G, n, C, A) of an update, ValueError for what the metric does not take.  Looks at shapes and the host copy of the
        mapping only."""
        from . import ops
        G, n, C, A = ops.topk_shapes(scores, targets)
        if G != self.groups:
            raise ValueError(f"TopkAccuracy: scores of {G} groups for a metric of {self.groups}")
        if A > 1 and self.metric_type != MetricType.IMAGENET_REAL_ACCURACY:
            raise ValueError(f"TopkAccuracy: {self.metric_type} takes one target per row, got {A} (only imagenet_real_accuracy takes more)")
        if self.class_mapping is None:
            if C != self.num_classes:
                raise ValueError(f"TopkAccuracy: scores of {C} columns for num_classes = {self.num_classes} without a class mapping")
        elif self._map_columns != C:
            check_class_mapping(self.class_mapping, C)
            self._map_columns = C
        if targets.dtype.is_floating_point or targets.dtype.is_complex or targets.dtype == torch.bool:
            raise ValueError("TopkAccuracy: targets must be integers")
        return G, n, C, A

    def update(self, scores, targets):
        from . import ops
        G, n, C, A = self.check(scores, targets)
        if not scores.is_cuda:
            raise RuntimeError("octic_vits_amd.metrics.TopkAccuracy runs on the GPU only (no CPU fallback); got CPU scores")
        self._bind(scores.device)
        if not n:
            return
        if scores.dtype != torch.float32:
            raise ValueError("TopkAccuracy: scores must be float32")
        if scores.stride(-1) != 1:
            scores = scores.contiguous()
        targets = targets.to(self.device, non_blocking=True).long().reshape(n, A).contiguous()
        self.rank = ops.topk_rank(scores.unsqueeze(0) if scores.dim() == 2 else scores, targets, class_map=self._map,
                                  order=_TIES[self.tie])
        ops.topk_count(self.rank, self.counters, self.ks, mode=ops.TOPK_CLASS if self.per_class else ops.TOPK_ANY,
                       num_classes=self.num_classes, targets=targets.view(n) if self.per_class else None)

    def compute(self):
        """Per group {"top-k": value} (a list of ``groups`` dictionaries): the one read-back."""
        if self.counters is None:
            shape = (self.groups, self.num_classes, 1 + len(self.ks)) if self.per_class else (self.groups, 1 + len(self.ks))
            host = torch.zeros(shape, dtype=torch.int64)
        else:
            host = self.counters.cpu()
        return [accuracies_from_counters(self.metric_type, host[g], self.ks, self.zero_support) for g in range(self.groups)]

    def reset(self):
        if self.counters is not None:
            self.counters.zero_()
        self.rank = None


def build_metric(metric_type, *, num_classes, ks=None, **kw):
    """The reference's build_metric: a ``TopkAccuracy`` of that type with ks = (1, 5) unless given; further keywords (groups,
    class_mapping, tie, zero_support, device) go to its constructor."""
    return TopkAccuracy(as_metric_type(metric_type), num_classes, ks=(1, 5) if ks is None else ks, **kw)


# ---------------------------------------------------------------------------------------------- linear probe (linear.py)
def evaluate_linear_classifiers(probe, batches, metric_type="mean_accuracy", class_mapping=None, best_classifier_on_val=None,
                                on_features=False):
    """evaluate_linear_classifiers (linear.py:262-312) on a ``LinearProbe`` for every metric type and an optional class mapping:
    one metric group per classifier in the probe's order, ``tie="strict"``, num_classes = len(class_mapping) where one is given.
    Returns ``LinearProbe.evaluate``'s dictionary without "loss" (the reference's evaluation has no criterion, and under a
    mapping or ReaL targets a loss is not defined).  The best classifier is the first strict maximum of top-1 in dictionary order
    starting from 0, or ``best_classifier_on_val`` where given; with per_class_accuracy (where the reference's ``.item()``
    raises) "best_classifier" is None.  batches: iterable of (images, targets), or of (feature rows, targets) with on_features."""
    metric_type = as_metric_type(metric_type)
    num_classes = len(class_mapping) if class_mapping is not None else probe.num_classes
    metric = TopkAccuracy(metric_type, num_classes, ks=(1, 5), groups=len(probe.names), class_mapping=class_mapping, tie="strict")
    if best_classifier_on_val is not None and best_classifier_on_val not in probe.names:
        raise KeyError(f"evaluate_linear_classifiers: no classifier named {best_classifier_on_val!r}")
    probe._need_gpu()
    n = 0
    for x, targets in batches:
        F = x if on_features else probe.extract(x)
        metric.update(probe.forward_features(F), torch.as_tensor(targets))
        n += F.shape[0]
    values = metric.compute()
    results = OrderedDict((name, dict(values[i])) for i, name in enumerate(probe.names))
    if metric_type == MetricType.PER_CLASS_ACCURACY:
        return {"best_classifier": None, "classifiers": results, "samples": n}
    best, best_acc = "", 0
    for name in probe.names:
        top1 = results[name]["top-1"]
        if (best_classifier_on_val is None and top1 > best_acc) or name == best_classifier_on_val:
            best, best_acc = name, top1
    return {"best_classifier": {"name": best, "accuracy": best_acc}, "classifiers": results, "samples": n}


def test_on_datasets(probe, test_sets, best_classifier_on_val, on_features=False):
    """test_on_datasets (linear.py:431-462): ``{f"{name}_accuracy": 100 * accuracy}`` of the classifier chosen on the validation
    set, per test set.  test_sets: iterable of (name, batches, metric_type, class_mapping)."""
    results = OrderedDict()
    for name, batches, metric_type, class_mapping in test_sets:
        if as_metric_type(metric_type) == MetricType.PER_CLASS_ACCURACY:
            raise ValueError("test_on_datasets: per_class_accuracy has no scalar accuracy (the reference raises here too)")
        r = evaluate_linear_classifiers(probe, batches, metric_type=metric_type, class_mapping=class_mapping,
                                        best_classifier_on_val=best_classifier_on_val, on_features=on_features)
        results[f"{name}_accuracy"] = 100.0 * r["best_classifier"]["accuracy"]
    return results


test_on_datasets.__test__ = False        # a driver named as the reference names it, not a test


# ---------------------------------------------------------------------------------------------- k-NN (knn.py)
def _probas_of_all_k(module, features):
    """(ks ascending, the [len(ks), B, C] probas whose slices KnnModule.forward hands out per k): one tensor, no copy."""
    return sorted(set(module.nb_knn)), module._vote(features)


def eval_knn_features(train_features, train_labels, val_batches_of_features, nb_knn=_knn.DEFAULT_NB_KNN, temperature=0.07,
                      n_per_class_list=(-1,), n_tries=1, accuracy_averaging=AccuracyAveraging.MEAN_ACCURACY, gather_on_cpu=False,
                      zero_support="exclude"):
    """``knn.eval_knn_features`` for every accuracy averaging (the enum, a name such as "mean_per_class_accuracy" or a value such
    as "macro"): ``{(n_per_class, k): {"top-1": ..., "top-5": ...}}`` averaged over the tries (per-class vectors elementwise), with
    num_classes = train_labels.max() + 1.  The modules are ``knn.create_module_dict``'s; the probas of all k of a module go through
    one ``TopkAccuracy(groups=len(ks), tie="index")``."""
    averaging = as_accuracy_averaging(accuracy_averaging)
    if gather_on_cpu:
        raise NotImplementedError("octic_vits_amd.metrics: gather_on_cpu (the training features stay on the device)")
    _knn._single_rank()
    if not train_features.is_cuda:
        raise RuntimeError("octic_vits_amd.metrics.eval_knn_features runs on the GPU only (no CPU fallback)")
    metric_type = MetricType[averaging.name]
    train_labels = train_labels.to(train_features.device).long()
    num_classes = int(train_labels.max()) + 1

    def module(train_features, train_labels, nb_knn):
        return _knn.KnnModule(train_features, train_labels, nb_knn, temperature, num_classes=num_classes)

    modules = _knn.create_module_dict(module=module, n_per_class_list=list(n_per_class_list), n_tries=n_tries, nb_knn=list(nb_knn),
                                      train_features=train_features, train_labels=train_labels)
    metrics = {}
    for feats, targets in val_batches_of_features:
        for name, tries in modules.items():
            for t, m in tries.items():
                ks, probas = _probas_of_all_k(m, feats)
                if (name, t) not in metrics:
                    metrics[(name, t)] = TopkAccuracy(metric_type, num_classes, ks=(1, 5), groups=len(ks), tie="index",
                                                      zero_support=zero_support)
                metrics[(name, t)].update(probas, torch.as_tensor(targets))
    results = {}
    for name, tries in modules.items():
        per_try = []
        for t, m in tries.items():
            if (name, t) not in metrics:
                raise RuntimeError("octic_vits_amd.metrics.eval_knn_features: nothing accumulated")
            values, ks = metrics[(name, t)].compute(), sorted(set(m.nb_knn))
            per_try.append({k: values[ks.index(k)] for k in m.nb_knn})
        for k in next(iter(tries.values())).nb_knn:
            results[(name, k)] = {key: sum(a[k][key] for a in per_try) / len(per_try) for key in ("top-1", "top-5")}
    return results


def eval_knn(model, train_batches, val_batches, nb_knn=_knn.DEFAULT_NB_KNN, temperature=0.07, n_per_class_list=(-1,), n_tries=1,
             accuracy_averaging=AccuracyAveraging.MEAN_ACCURACY, gather_on_cpu=False, zero_support="exclude"):
    """``knn.eval_knn`` for every accuracy averaging: the features of the training set, then every validation batch through
    every module.  train_batches / val_batches: iterables of (images, labels)."""
    as_accuracy_averaging(accuracy_averaging)
    if gather_on_cpu:
        raise NotImplementedError("octic_vits_amd.metrics: gather_on_cpu (the training features stay on the device)")
    _knn._single_rank()
    train_features, train_labels = _knn.extract_features(model, train_batches)

    def val_features():
        for images, y in val_batches:
            yield _knn.extract_features(model, [(images, y)])

    return eval_knn_features(train_features, train_labels, val_features(), nb_knn=nb_knn, temperature=temperature,
                             n_per_class_list=n_per_class_list, n_tries=n_tries, accuracy_averaging=accuracy_averaging,
                             zero_support=zero_support)
