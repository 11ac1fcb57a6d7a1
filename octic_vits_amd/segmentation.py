"""Segmentation evaluation of a frozen DINOv2 backbone: the logreg and k-NN classifiers of the reference's ``eval_model``
(dinov2/eval/segmentation/eval_segmentation.py:346-470) on ONE GPU with the patch features resident in device memory.

The reference gathers ~20 GB of patch features to the host, fits cuML's L-BFGS logistic regression and scores with
sklearn.  Here the feature matrix X [N, D] (f32) is written once by ``patch_features`` and never leaves the device or is
copied: standardisation is in place, a held-out validation tenth is a row range, ignored patches are rows whose target
is -1, a sub-sampled fit is a row stride.  The per-evaluation work (cross entropy + ``softmax - onehot``, then
``dlogits^T X``) runs on csrc/segeval.hip; the L-BFGS iteration itself is ~0.8 MB of float64 state and runs on the host
(``lbfgs``), which is also how it is tested without a GPU.

Objective (sklearn's and cuML's default, penalty="l2", intercept unpenalised, start at zero):

    J(W, b) = C * sum_n CE(x_n W^T + b, y_n) + 1/2 |W|^2

Stopping rule of ``lbfgs`` (cuML's own rule is not reproducible here and not claimed): stop when
``max|g| <= tol * max(1, max|x|)``, after ``max_iter`` iterations, or when a line search finds no point with a lower
objective in ``linesearch_max_iter`` trials - then the best iterate seen is returned.  An f32 objective always ends on
that last rule: near the optimum the decrease along the search direction falls below the rounding noise of the sum.

k-NN (``KNNClassifier``, csrc/segknn.hip): the reference materialises ``cdist`` and runs ``topk`` once per grid point; here
ONE fused pass gives the 32 nearest training patches under both distances (both need only the dot product and the row norms,
and the lists for fewer neighbours are prefixes), and a vote kernel reads the neighbours' pixel labels from the resident label
matrix.  Neighbours are ordered by (distance, row index) - ``torch.topk`` leaves ties unspecified.  ``eval_model`` still refuses
"knn" (its refusal is pinned by earlier tests); the reference's default ``("logreg", "knn")`` runs through ``extract_splits`` +
``eval_features``, which share one backbone pass.  The final refit is on train + val with the validation rows FIRST in the
resident matrix (the reference concatenates train then val): row order matters to k-NN only through exact distance ties.
``KNNClassifier(dtype="bfloat16")`` - what the reference's eval_config.yaml sets - rounds keys and queries to bf16 ONCE and
computes everything after that cast in float32 (norms, bf16-MFMA dots with f32 accumulation, ordering keys, the same total
order): one deterministic member of the reference's set of valid bf16 answers; the class docstring has the rule.

Not here: the L1 / Linf / inner_product distances and more than 32 neighbours, RobustScaler / PCA standardisation, datasets
and transforms, multi-rank grid splitting.
CPU tensors raise "GPU only" wherever a kernel is involved; ``lbfgs``, ``patch_labels``, ``upscale``, the metric formulas
on a confusion matrix, the hyper-parameter names and the label <-> class-index tables are plain host code.
"""
import itertools
from typing import Any, Callable, Dict, Iterable, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops

__all__ = ["patch_features", "patch_labels", "Standardizer", "LogregClassifier", "lbfgs", "mIoU", "accuracy",
           "confusion_matrix", "miou_from_confusion", "accuracy_from_confusion", "class_tables", "hparam_name", "eval_model", "KNNClassifier", "SegSplits", "extract_splits",
           "eval_features"]


# ------------------------------------------------------------------------------------------------ features and labels
def _patch_size(model) -> int:
    ps = getattr(model, "patch_size", None)
    if ps is None:
        ps = model.patch_embed.patch_size
    return int(ps[0] if isinstance(ps, (tuple, list)) else ps)


@torch.no_grad()
def patch_features(model, images: torch.Tensor, out: Optional[torch.Tensor] = None, row0: int = 0) -> torch.Tensor:
    """The [B, ih, iw, D] f32 feature map of the reference's ``custom_fwd`` (segmentation/dinov2_loader.py:13-29): the normed
    patch tokens of the last block, class and register tokens dropped, computed under bf16 autocast (eval_segmentation.py:400).
    With ``out`` (the resident f32 [N, D] matrix) the rows ``row0 .. row0 + B ih iw`` are written in place and returned as a
    view: no cat, no host gather."""
    ops._require_cuda(images)
    ps = _patch_size(model)
    B, _, H, W = images.shape
    ih, iw = H // ps, W // ps
    with torch.autocast("cuda", dtype=torch.bfloat16):
        tokens = model.get_intermediate_layers(images, n=1, norm=True)[0]
    D = tokens.shape[-1]
    if tuple(tokens.shape[:2]) != (B, ih * iw):
        raise ValueError(f"patch_features: expected {ih * iw} patch tokens per image, got {tuple(tokens.shape)}")
    if out is None:
        return tokens.float().reshape(B, ih, iw, D).contiguous()
    if out.dim() != 2 or out.dtype != torch.float32 or out.shape[1] != D or not out.is_contiguous():
        raise ValueError("patch_features: out must be a contiguous f32 [N, D] matrix")
    if row0 < 0 or row0 + B * ih * iw > out.shape[0]:
        raise ValueError("patch_features: the batch does not fit into out at row0")
    rows = out[row0:row0 + B * ih * iw]
    rows.copy_(tokens.reshape(B * ih * iw, D))
    return rows.view(B, ih, iw, D)


def patch_labels(labels: torch.Tensor, patch_size: int) -> torch.Tensor:
    """[B, H, W] pixel labels -> [B ih iw, ps^2]: the ``bs (ih ph) (iw pw) -> (bs ih iw) (ph pw)`` rearrangement of
    ``extract_features`` (segmentation/utils.py:493-500)."""
    if labels.dim() != 3:
        raise ValueError("patch_labels: labels must be [B, H, W]")
    B, H, W = labels.shape
    ps = int(patch_size)
    if H % ps or W % ps:
        raise ValueError("patch_labels: H and W must be multiples of the patch size")
    ih, iw = H // ps, W // ps
    return labels.reshape(B, ih, ps, iw, ps).permute(0, 1, 3, 2, 4).reshape(B * ih * iw, ps * ps)


# ------------------------------------------------------------------------------------------------ standardisation
class Standardizer:
    """``standardizations[kind]()`` of segmentation/utils.py:566-573 for kind in "StandardScaler", "center", "center_div":
    column statistics in f64 on the device, ``transform`` in place on the resident matrix.
    ``mean_`` / ``scale_`` are f64 [D] device tensors (``scale_`` is a broadcast scalar for "center_div", ones for "center")."""

    KINDS = ("StandardScaler", "center", "center_div")

    def __init__(self, kind: str = "StandardScaler"):
        if kind in ("RobustScaler", "pca", "pca_whiten"):
            raise NotImplementedError(f"standardization {kind!r} is not implemented on the HIP engine")
        if kind not in self.KINDS:
            raise ValueError(f"unknown standardization {kind!r}")
        self.kind = kind

    def fit(self, X: torch.Tensor) -> "Standardizer":
        mean, var = ops.seg_colstats(X)
        n = X.shape[0]
        self.mean_, self.var_, self.n_samples_seen_ = mean, var, n
        if self.kind == "StandardScaler":
            # sklearn's _is_constant_feature / _handle_zeros_in_scale: a column whose variance is rounding noise keeps scale 1
            eps = float(np.finfo(np.float64).eps)
            constant = var <= n * eps * var + (n * mean * eps) ** 2
            self.scale_ = torch.where(constant, torch.ones_like(var), var.sqrt())
        elif self.kind == "center":
            self.scale_ = torch.ones_like(var)
        else:   # one global std over all elements: E[var_d + (mean_d - m)^2]
            m = mean.mean()
            std = (var + (mean - m) ** 2).mean().sqrt()
            self.scale_ = torch.full_like(var, float(std) + 1e-8)
        return self

    def transform(self, X: torch.Tensor) -> torch.Tensor:
        return ops.seg_standardize_(X, self.mean_, self.scale_)

    def fit_transform(self, X: torch.Tensor) -> torch.Tensor:
        return self.fit(X).transform(X)


# ------------------------------------------------------------------------------------------------ L-BFGS (host, float64)
def lbfgs(fun: Callable[[np.ndarray], Tuple[float, np.ndarray]], x0, memory: int = 5, max_iter: int = 1000,
          tol: float = 1e-12, linesearch_max_iter: int = 50):
    """Minimise ``fun(x) -> (f, g)`` from ``x0`` with L-BFGS: two-loop recursion over the last ``memory`` (s, y) pairs, and a
    line search for the strong Wolfe conditions (c1 = 1e-4, c2 = 0.9; bracketing by doubling, then safeguarded cubic
    interpolation) that spends at most ``linesearch_max_iter`` evaluations.  A search that ends without a Wolfe point takes
    its best trial if that lowers f.  Stops on ``max|g| <= tol * max(1, max|x|)``, on ``max_iter``, or when a search finds
    no lower point - and then returns the best iterate seen.  Returns ``(x, f, info)``; everything in numpy float64."""
    x = np.array(x0, dtype=np.float64).ravel().copy()
    f, g = fun(x)
    f, g = float(f), np.asarray(g, dtype=np.float64).ravel()
    n_eval = 1
    S, Y, RHO = [], [], []
    status = "max_iter"
    it = 0
    c1, c2 = 1e-4, 0.9

    def converged(x, g):
        return float(np.max(np.abs(g))) <= tol * max(1.0, float(np.max(np.abs(x))))

    if converged(x, g):
        return x, f, {"n_iter": 0, "n_eval": n_eval, "status": "converged"}
    while it < max_iter:
        # two-loop recursion
        q = g.copy()
        alphas = []
        for s, y, rho in zip(reversed(S), reversed(Y), reversed(RHO)):
            a = rho * float(s @ q)
            alphas.append(a)
            q -= a * y
        if S:
            q *= float(S[-1] @ Y[-1]) / float(Y[-1] @ Y[-1])
        for (s, y, rho), a in zip(zip(S, Y, RHO), reversed(alphas)):
            q += (a - rho * float(y @ q)) * s
        d = -q
        dg0 = float(g @ d)
        if not dg0 < 0.0:            # not a descent direction (numerical breakdown of the pairs): steepest descent
            S, Y, RHO = [], [], []
            d = -g
            dg0 = float(g @ d)
        step = 1.0 if S else min(1.0, 1.0 / float(np.sqrt(g @ g)))

        # ---- line search: phi(a) = f(x + a d)
        best = None                   # (f, a, g) of the lowest trial
        evals = [0]

        def phi(a):
            fa, ga = fun(x + a * d)
            evals[0] += 1
            fa = float(fa)
            ga = np.asarray(ga, dtype=np.float64).ravel()
            if not np.isfinite(fa):
                return np.inf, ga, np.inf
            return fa, ga, float(ga @ d)

        def note(a, fa, ga):
            nonlocal best
            if np.isfinite(fa) and (best is None or fa < best[0]):
                best = (fa, a, ga)

        def interpolate(a_lo, f_lo, dg_lo, a_hi, f_hi, dg_hi):
            """Minimiser of the cubic through both points (values and slopes), kept inside the middle 80 % of the bracket."""
            lo, hi = min(a_lo, a_hi), max(a_lo, a_hi)
            mid = 0.5 * (lo + hi)
            if not (np.isfinite(f_hi) and np.isfinite(dg_hi)):
                return mid
            d1 = dg_lo + dg_hi - 3.0 * (f_lo - f_hi) / (a_lo - a_hi)
            rad = d1 * d1 - dg_lo * dg_hi
            if rad < 0.0:
                return mid
            d2 = np.sqrt(rad) * (1.0 if a_hi > a_lo else -1.0)
            den = dg_hi - dg_lo + 2.0 * d2
            if den == 0.0:
                return mid
            a = a_hi - (a_hi - a_lo) * (dg_hi + d2 - d1) / den
            if not np.isfinite(a):
                return mid
            width = hi - lo
            return min(max(a, lo + 0.1 * width), hi - 0.1 * width)

        accepted = None
        a_prev, f_prev, dg_prev = 0.0, f, dg0
        a = step
        bracket = None
        while evals[0] < linesearch_max_iter:
            fa, ga, dga = phi(a)
            note(a, fa, ga)
            if fa > f + c1 * a * dg0 or (a_prev > 0.0 and fa >= f_prev):
                bracket = (a_prev, f_prev, dg_prev, a, fa, dga)
                break
            if abs(dga) <= -c2 * dg0:
                accepted = (fa, a, ga)
                break
            if dga >= 0.0:
                bracket = (a, fa, dga, a_prev, f_prev, dg_prev)
                break
            a_prev, f_prev, dg_prev = a, fa, dga
            a *= 2.0
        if accepted is None and bracket is not None:
            a_lo, f_lo, dg_lo, a_hi, f_hi, dg_hi = bracket
            while evals[0] < linesearch_max_iter and abs(a_hi - a_lo) > 1e-16 * max(abs(a_lo), abs(a_hi)):
                a = interpolate(a_lo, f_lo, dg_lo, a_hi, f_hi, dg_hi)
                fa, ga, dga = phi(a)
                note(a, fa, ga)
                if fa > f + c1 * a * dg0 or fa >= f_lo:
                    a_hi, f_hi, dg_hi = a, fa, dga
                else:
                    if abs(dga) <= -c2 * dg0:
                        accepted = (fa, a, ga)
                        break
                    if dga * (a_hi - a_lo) >= 0.0:
                        a_hi, f_hi, dg_hi = a_lo, f_lo, dg_lo
                    a_lo, f_lo, dg_lo = a, fa, dga
        n_eval += evals[0]
        if accepted is None and best is not None and best[0] < f:
            accepted = best
        if accepted is None:
            status = "linesearch"     # no lower point: x is the best iterate (f only ever decreases along the run)
            break
        f_new, a, g_new = accepted
        s = a * d
        y = g_new - g
        sy = float(s @ y)
        if sy > 1e-10 * float(y @ y):
            S.append(s)
            Y.append(y)
            RHO.append(1.0 / sy)
            if len(S) > memory:
                S.pop(0), Y.pop(0), RHO.pop(0)
        x, f, g = x + s, f_new, g_new
        it += 1
        if converged(x, g):
            status = "converged"
            break
    return x, f, {"n_iter": it, "n_eval": n_eval, "status": status}


# ------------------------------------------------------------------------------------------------ metrics
def confusion_matrix(y_true: torch.Tensor, y_pred: torch.Tensor, ignore_labels: Sequence[int]) -> torch.Tensor:
    """int64 [256, 256] device counts of (pixel label, predicted label) over the pixels whose label is not ignored.
    ``y_true`` is [n, L]; ``y_pred`` is [n] patch labels or their up-scaled [n, L] form (``Classifier.upscale``)."""
    ops._require_cuda(y_true)
    ops._require_cuda(y_pred)
    if y_true.dim() == 1:
        y_true = y_true[:, None]
    if y_pred.dim() == 2:
        if y_pred.shape != y_true.shape:
            raise ValueError("confusion_matrix: y_pred must be [n] or match y_true")
        if y_pred.stride(1) == 0 or y_pred.shape[1] == 1:
            y_pred = y_pred[:, 0]                      # the expanded view upscale() returns
        else:                                          # arbitrary per-pixel predictions: one pixel per row
            y_true, y_pred = y_true.reshape(-1, 1), y_pred.reshape(-1)
    ignore = torch.zeros(256, dtype=torch.uint8)
    for v in ignore_labels:
        ignore[int(v) & 255] = 1
    counts = torch.zeros(256, 256, dtype=torch.int64, device=y_true.device)
    return ops.seg_confusion(y_true.contiguous(), y_pred.to(torch.int32).contiguous(), ignore.to(y_true.device), counts)


def _np_conf(conf) -> np.ndarray:
    return conf.detach().cpu().numpy() if isinstance(conf, torch.Tensor) else np.asarray(conf)


def accuracy_from_confusion(conf) -> float:
    """Pixel accuracy over the counted pixels (``accuracy``, eval_segmentation.py:50-54)."""
    c = _np_conf(conf).astype(np.float64)
    return float(np.trace(c) / c.sum())


def miou_from_confusion(conf) -> float:
    """``sklearn.metrics.jaccard_score(gt[mask], pred[mask], average="macro")`` (eval_segmentation.py:57-61): the mean of
    tp / (tp + fp + fn) over the labels present in the masked truth OR the masked prediction."""
    c = _np_conf(conf).astype(np.float64)
    tp = np.diag(c)
    rows, cols = c.sum(1), c.sum(0)
    present = (rows + cols) > 0
    return float(np.mean(tp[present] / (rows + cols - tp)[present]))


def accuracy(y_true, y_pred, ignore_labels: Sequence[int]) -> float:
    return accuracy_from_confusion(confusion_matrix(y_true, y_pred, ignore_labels))


def mIoU(y_true, y_pred, ignore_labels: Sequence[int]) -> float:
    return miou_from_confusion(confusion_matrix(y_true, y_pred, ignore_labels))


metrics_dict = {"mIoU": mIoU, "acc": accuracy}


# ------------------------------------------------------------------------------------------------ classifier
def class_tables(modes: torch.Tensor, ignore_labels: Sequence[int]):
    """(classes, lut): the sorted label values that occur among the non-ignored patch labels (sklearn's ``classes_``) and the
    int32 [256] table label value -> class index, -1 for ignored or absent values."""
    present = torch.zeros(256, dtype=torch.bool, device=modes.device)
    present[modes.long()] = True
    for v in ignore_labels:
        if 0 <= int(v) < 256:
            present[int(v)] = False
    classes = torch.nonzero(present).flatten()
    lut = torch.full((256,), -1, dtype=torch.int32, device=modes.device)
    lut[classes] = torch.arange(classes.numel(), dtype=torch.int32, device=modes.device)
    return classes, lut


def hparam_name(metric_name: str, names: Sequence[str], values: Sequence[Any]) -> str:
    """The key ``select_hparams`` reports a grid point under (eval_segmentation.py:136-138)."""
    return f"{metric_name}_" + "_".join(f"{k}={v}" for k, v in zip(names, values))


class LogregClassifier:
    """``LogregClassifier`` of eval_segmentation.py:281-337 with the reference's grids as defaults.  ``fit`` keeps the
    feature matrix where it is: sub-sampling is a row stride, patches whose label is ignored get target -1 (the kernels
    skip them), label values are mapped to class indices and back in ``predict``."""

    def __init__(self, ignore_labels: Sequence[int], train_set_subsampling: int = 1, inference_bs: int = 1024,
                 C: Iterable[float] = tuple(10 ** np.linspace(-6, 5, 8)), max_iter: Iterable[int] = (1000,),
                 tol: Iterable[float] = (1e-12,), linesearch_max_iter: Iterable[int] = (50,),
                 lbfgs_hessian_rank: Iterable[int] = (5,)):
        self.train_set_subsampling = train_set_subsampling
        self.inference_bs = inference_bs            # kept for the signature: prediction is one launch over all rows
        self.ignore_labels = ignore_labels
        self.hparam_grids = {"C": C, "max_iter": max_iter, "tol": tol, "linesearch_max_iter": linesearch_max_iter,
                             "lbfgs_hessian_rank": lbfgs_hessian_rank}
        for k, grid in self.hparam_grids.items():   # a fit without select_hparams uses the first grid point
            setattr(self, k, next(iter(grid)))

    # ---- host pieces
    def upscale(self, labels: torch.Tensor) -> torch.Tensor:
        """Patch level -> pixel level (a broadcast view)."""
        return labels[:, None].expand(-1, self.n_pixels_per_sample)

    def targets_from_modes(self, modes: torch.Tensor):
        """(classes, y): class table and int32 targets of the (already sub-sampled) patch labels, -1 where ignored."""
        classes, lut = class_tables(modes, self.ignore_labels)
        return classes, lut[modes.long()]

    def unfit(self) -> None:
        for k in ("coef_", "intercept_", "classes_"):
            if hasattr(self, k):
                delattr(self, k)

    # ---- device pieces
    def fit(self, features: torch.Tensor, labels: torch.Tensor) -> None:
        self.unfit()
        ops._require_cuda(features)
        ops._require_cuda(labels)
        if self.train_set_subsampling > 1:
            labels = labels[:: self.train_set_subsampling]
            features = features[:: self.train_set_subsampling]
        self.n_pixels_per_sample = labels.shape[-1]
        self.label_dtype = labels.dtype
        modes = ops.seg_patch_mode(labels.contiguous())
        classes, y = self.targets_from_modes(modes)
        del modes
        if classes.numel() < 2:
            raise ValueError("LogregClassifier.fit needs at least 2 classes among the non-ignored patches")
        self.n_fit_rows_ = int(features.shape[0])
        self._fit(features, y, classes)

    def _fit(self, X: torch.Tensor, y: torch.Tensor, classes: torch.Tensor) -> None:
        N, D = X.shape
        nc = int(classes.numel())
        dev = X.device
        dlogits = torch.empty(N, ops.seg_ldd(nc), dtype=torch.float32, device=dev)
        ws = ops.seg_workspace(N, D, nc, dev)
        W, b = torch.empty(nc, D, dtype=torch.float32, device=dev), torch.empty(nc, dtype=torch.float32, device=dev)
        dW, db = torch.empty_like(W), torch.empty_like(b)
        value = torch.empty(1, dtype=torch.float64, device=dev)
        Creg = float(self.C)

        def fun(x):
            w64 = x[:nc * D]
            W.copy_(torch.from_numpy(w64.astype(np.float32)).view(nc, D))
            b.copy_(torch.from_numpy(x[nc * D:].astype(np.float32)))
            ops.seg_value_dlogits(X, W, b, y, dlogits, value, ws)
            ops.seg_wgrad(X, dlogits, W, Creg, 1.0, dW, db, ws)
            g = np.concatenate([dW.flatten().cpu().numpy(), db.cpu().numpy()]).astype(np.float64)
            return Creg * float(value.item()) + 0.5 * float(w64 @ w64), g

        x, f, info = lbfgs(fun, np.zeros(nc * D + nc), memory=int(self.lbfgs_hessian_rank), max_iter=int(self.max_iter),
                           tol=float(self.tol), linesearch_max_iter=int(self.linesearch_max_iter))
        self.coef_ = torch.from_numpy(x[:nc * D].astype(np.float32)).view(nc, D).to(dev)
        self.intercept_ = torch.from_numpy(x[nc * D:].astype(np.float32)).to(dev)
        self.classes_ = classes
        self.objective_, self.solver_info_ = f, info

    @torch.no_grad()
    def predict_patches(self, features: torch.Tensor) -> torch.Tensor:
        """[n] predicted label VALUES (label dtype), one per patch row."""
        idx = torch.empty(features.shape[0], dtype=torch.int32, device=features.device)
        ops.seg_predict(features, self.coef_, self.intercept_, idx)
        return self.classes_[idx.long()].to(self.label_dtype)

    @torch.no_grad()
    def predict(self, features: torch.Tensor) -> torch.Tensor:
        """[n, L] pixel-level predictions on the device (the reference returns them on the host)."""
        return self.upscale(self.predict_patches(features))

    def select_hparams(self, features_train, labels_train, features_val, labels_val, metric_name: str = "mIoU") -> Dict[str, float]:
        names, grids = zip(*self.hparam_grids.items())
        grid = list(itertools.product(*grids))
        metrics: Dict[str, float] = {}
        best = grid[0]
        if len(grid) > 1:
            scores = []
            for point in grid:
                for k, v in zip(names, point):
                    setattr(self, k, v)
                self.fit(features_train, labels_train)
                score = metrics_dict[metric_name](labels_val, self.predict(features_val), self.ignore_labels)
                scores.append(score)
                metrics[hparam_name(metric_name, names, point)] = score
                self.unfit()
            best = grid[int(np.argmax(scores))]         # the first maximum, as max() over the reference's ordered results
        for k, v in zip(names, best):
            setattr(self, k, v)
        return metrics


class KNNClassifier:
    """``KNNClassifier`` of eval_segmentation.py:172-278 with the reference's signature and grids.  ``inference_bs``,
    ``train_set_chunk_size`` and ``device`` are kept for the signature and not used: the keys are the resident matrix, streamed
    by one kernel.  ``fit`` keeps views (sub-sampling is a row stride), marks the patches whose mode label is ignored as skipped
    keys (``Classifier.fit``, :83) and computes the key norms.  The vote is over the neighbours' raw pixel labels, so an ignored
    value can win a pixel, as in the reference.  Distances "cosine" and "L2"; at most 32 neighbours.

    ``dtype="bfloat16"`` is the reference's shipped configuration (``classifiers_kwargs: {knn: {dtype: bfloat16}}``,
    eval_config.yaml).  The reference casts keys and queries to bf16, forms bf16 distances and calls ``torch.topk`` on them;
    those carry 8 significant bits and tie in bulk, ``topk`` leaves ties open, so its lists are not reproducible.  Here:
    1. operands are rounded ONCE, with ``tensor.to(torch.bfloat16)`` (the reference's own cast): the keys in ``fit`` after
       sub-sampling, each query batch in ``predict_grid``.  The bf16 copy of the keys is what stays resident; the caller's f32
       matrix is not kept.
    2. everything after the cast is float32: the row norms of the rounded rows (a fixed-order f32 sum), the dot products (bf16
       MFMA, f32 accumulation), the ordering keys, the total order (distance, key row index), the NaN and skip rules.
    3. both distances come from one pass; there is no second, normalised-then-rounded copy of the keys for the cosine distance.
    Rounding is monotone, so the list ordered by the f32 distance of the rounded operands is one valid top-k of the
    reference's bf16 distances (for cosine: within one bf16 ulp, the price of rounding once instead of normalising in bf16),
    and a deterministic one.  Any other ``dtype`` than "float32" / "bfloat16" is a ValueError."""

    DISTANCES = {"L2": ops.KNN_L2, "cosine": ops.KNN_COSINE}
    DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16}
    # Queries go through the kernels in batches of at most this many rows: the neighbour lists and votes of a batch are a few
    # hundred bytes per row, and the workspace the library asks for (octic_seg_knn_workspace_bytes) holds partial lists only
    # while splits x query tiles stays near the CU count, so memory is bounded whatever the number of rows.
    QUERY_ROWS = 65536

    def __init__(self, ignore_labels: Sequence[int], inference_bs: int = 1024, train_set_chunk_size: Optional[int] = 262144,
                 train_set_subsampling: int = 1, device: str = "cuda", dtype: str = "float32",
                 num_neighbors: Sequence[int] = (1, 3, 10, 30), distance: Sequence[str] = ("cosine", "L2")):
        if dtype not in self.DTYPES:
            raise ValueError(f"KNNClassifier: the HIP engine computes k-NN distances from float32 or bfloat16 operands, not {dtype!r}")
        self.device, self.dtype = device, self.DTYPES[dtype]
        self.inference_bs, self.train_set_chunk_size = inference_bs, train_set_chunk_size
        self.train_set_subsampling = train_set_subsampling
        self.ignore_labels = ignore_labels
        self.hparam_grids = {"num_neighbors": tuple(num_neighbors), "distance": tuple(distance)}
        for k in self.hparam_grids["num_neighbors"]:
            self._check_k(k)
        for d in self.hparam_grids["distance"]:
            self._check_distance(d)
        for k, grid in self.hparam_grids.items():   # a fit without select_hparams uses the first grid point
            setattr(self, k, grid[0])

    # ---- host pieces
    @staticmethod
    def _check_k(k) -> int:
        if int(k) != k or not 1 <= int(k) <= ops.KNN_KMAX:
            raise ValueError(f"KNNClassifier: num_neighbors must be an integer in 1 .. {ops.KNN_KMAX}, got {k!r}")
        return int(k)

    @classmethod
    def _check_distance(cls, d) -> int:
        if d in ("L1", "Linf", "inner_product"):
            raise NotImplementedError(f"k-NN distance {d!r} is not implemented on the HIP engine")
        if d not in cls.DISTANCES:
            raise ValueError(f"unknown k-NN distance {d!r}")
        return cls.DISTANCES[d]

    def upscale(self, labels: torch.Tensor) -> torch.Tensor:
        return labels[:, None].expand(-1, self.n_pixels_per_sample)

    def unfit(self) -> None:
        for k in ("train_X", "train_y", "key_norms_", "skip_", "n_keys_"):
            if hasattr(self, k):
                delattr(self, k)

    # ---- device pieces
    def fit(self, features: torch.Tensor, labels: torch.Tensor) -> None:
        self.unfit()
        ops._require_cuda(features)
        ops._require_cuda(labels)
        if self.train_set_subsampling > 1:
            labels = labels[:: self.train_set_subsampling]
            features = features[:: self.train_set_subsampling]
        self.n_pixels_per_sample = labels.shape[-1]
        self.label_dtype = labels.dtype
        labels = labels.contiguous()                 # a copy only when sub-sampled
        modes = ops.seg_patch_mode(labels)
        ignore = torch.zeros(256, dtype=torch.bool, device=labels.device)
        for v in self.ignore_labels:
            ignore[int(v) & 255] = True
        self.skip_ = ignore[modes.long()].to(torch.uint8)
        self.n_keys_ = int(features.shape[0]) - int(self.skip_.sum())
        if self.dtype != torch.float32:
            features = features.to(self.dtype)       # rounded once; this copy, not the caller's matrix, stays resident
        self.train_X, self.train_y = features, labels
        self.key_norms_ = ops.seg_rownorms(features)

    @torch.no_grad()
    def predict_grid(self, features: torch.Tensor, ks: Sequence[int], distances: Sequence[str]) -> Dict[Tuple[int, str], torch.Tensor]:
        """{(k, distance): [n, L] pixel-level predictions on the device} for every pair, from ONE pass over the keys."""
        ops._require_cuda(features)
        if not hasattr(self, "train_X"):
            raise RuntimeError("KNNClassifier.predict before fit")
        ks = [self._check_k(k) for k in ks]
        metrics = 0
        for d in distances:
            metrics |= self._check_distance(d)
        kasc = sorted(set(ks))
        kmax = kasc[-1]
        if self.n_keys_ < kmax:
            raise ValueError(f"KNNClassifier: {kmax} neighbours asked for, but only {self.n_keys_} training patches are not ignored")
        n, L = features.shape[0], self.n_pixels_per_sample
        dev = features.device
        votes = {d: torch.empty(len(kasc), n, L, dtype=torch.uint8, device=dev) for d in dict.fromkeys(distances)}
        M, D = self.train_X.shape
        bs = min(n, self.QUERY_ROWS)
        ws = ops.seg_knn_workspace(bs, M, D, kmax, metrics, 0, dev) if n else None
        for i in range(0, n, bs):
            q = features[i:i + bs]
            if self.dtype != torch.float32:
                q = q.to(self.dtype)
            if q.shape[0] != bs:                     # the last batch: its own plan and workspace
                ws = ops.seg_knn_workspace(q.shape[0], M, D, kmax, metrics, 0, dev)
            idx_l2, _, idx_cos, _ = ops.seg_knn(q, self.train_X, ops.seg_rownorms(q), self.key_norms_, self.skip_, kmax, metrics,
                                                0, workspace=ws)
            for d, idx in (("L2", idx_l2), ("cosine", idx_cos)):
                if d in votes:
                    votes[d][:, i:i + bs] = ops.seg_knn_vote(idx, self.train_y, kasc)
        return {(k, d): votes[d][kasc.index(k)].to(self.label_dtype) for k in ks for d in distances}

    @torch.no_grad()
    def predict(self, features: torch.Tensor) -> torch.Tensor:
        """[n, L] pixel-level predictions on the device for the current (num_neighbors, distance)."""
        return self.predict_grid(features, (self.num_neighbors,), (self.distance,))[(int(self.num_neighbors), self.distance)]

    def select_hparams(self, features_train, labels_train, features_val, labels_val, metric_name: str = "mIoU") -> Dict[str, float]:
        names, grids = zip(*self.hparam_grids.items())
        grid = list(itertools.product(*grids))
        metrics: Dict[str, float] = {}
        best = grid[0]
        if len(grid) > 1:
            self.fit(features_train, labels_train)
            preds = self.predict_grid(features_val, self.hparam_grids["num_neighbors"], self.hparam_grids["distance"])
            scores = []
            for point in grid:
                score = metrics_dict[metric_name](labels_val, preds[(int(point[0]), point[1])], self.ignore_labels)
                scores.append(score)
                metrics[hparam_name(metric_name, names, point)] = score
            del preds
            self.unfit()
            best = grid[int(np.argmax(scores))]         # the first maximum
        for k, v in zip(names, best):
            setattr(self, k, v)
        return metrics


classifiers_dict = {"logreg": LogregClassifier, "knn": KNNClassifier}


# ------------------------------------------------------------------------------------------------ eval_model
def _count_images(batches) -> int:
    return sum(int(im.shape[0]) for im, _ in batches)


@torch.no_grad()
def _extract(model, batches, X, L, row0, ps, slots=None):
    """Write the features / patch labels of the batches into rows row0 .. of X / L; with ``slots`` image i of the split goes
    to image slot slots[i] (the seeded hold-out permutation) instead of slot i."""
    dev = X.device
    i0 = 0
    for images, labels in batches:
        images = images.to(dev, non_blocking=True)
        lab = patch_labels(labels.to(dev, non_blocking=True), ps).to(L.dtype)
        B = images.shape[0]
        P = (images.shape[2] // ps) * (images.shape[3] // ps)
        if slots is None:
            patch_features(model, images, out=X, row0=row0 + i0 * P)
            L[row0 + i0 * P: row0 + (i0 + B) * P] = lab
        else:
            fm = patch_features(model, images)
            idx = torch.as_tensor(slots[i0:i0 + B], device=dev, dtype=torch.long)
            n_slots = (X.shape[0] - row0) // P
            X[row0:row0 + n_slots * P].view(n_slots, P, -1).index_copy_(0, idx, fm.view(B, P, -1))
            L[row0:row0 + n_slots * P].view(n_slots, P, -1).index_copy_(0, idx, lab.view(B, P, -1))
        i0 += B


class SegSplits:
    """What ``extract_splits`` leaves on the device: X [n_fit P, D] f32 and L [n_fit P, ps^2] uint8 with the ``n_val`` validation
    images FIRST (so train, val and train + val are row ranges), the test rows Xt / Lt, and P patches per image."""
    __slots__ = ("X", "L", "Xt", "Lt", "n_val", "P")

    def __init__(self, X, L, Xt, Lt, n_val, P):
        self.X, self.L, self.Xt, self.Lt, self.n_val, self.P = X, L, Xt, Lt, n_val, P


def extract_splits(model, train, test, val=None, standardization: Optional[str] = "StandardScaler", val_seed: int = 0) -> SegSplits:
    """The feature half of ``eval_model`` (eval_segmentation.py:386-415).  ``train`` / ``test`` / ``val`` are iterables of
    ``(images [B, 3, H, W], labels [B, H, W])`` batches (one resolution; they are walked once, after being listed to count the
    images).  With ``val=None`` a tenth of the training images, drawn by ``numpy.random.RandomState(val_seed).permutation``,
    is held out (:392-398).  Train and validation features share ONE resident matrix, validation rows first; the
    standardisation is fitted on the training rows only and applied in place."""
    preproc = Standardizer(standardization) if standardization is not None else None
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError("octic_vits_amd.segmentation.eval_model runs on the GPU only (no CPU fallback)")
    ps = _patch_size(model)
    train, test = list(train), list(test)
    val = list(val) if val is not None else None
    im0 = train[0][0]
    P = (im0.shape[2] // ps) * (im0.shape[3] // ps)
    D = int(model.embed_dim)
    n_train_all = _count_images(train)
    if val is None:
        perm = np.random.RandomState(val_seed).permutation(n_train_all)
        n_val = n_train_all // 10
        slot_of = np.empty(n_train_all, dtype=np.int64)
        slot_of[perm] = np.arange(n_train_all)        # image perm[j] sits in slot j: slots 0 .. n_val-1 are the hold-out
        n_fit = n_train_all
    else:
        n_val = _count_images(val)
        n_fit = n_val + n_train_all
    label_dtype = torch.uint8                          # label values are 0 .. 255: one byte per pixel next to the features
    X = torch.empty(n_fit * P, D, dtype=torch.float32, device=dev)
    L = torch.empty(n_fit * P, ps * ps, dtype=label_dtype, device=dev)
    if val is None:
        _extract(model, train, X, L, 0, ps, slots=slot_of)
    else:
        _extract(model, val, X, L, 0, ps)
        _extract(model, train, X, L, n_val * P, ps)
    n_test = _count_images(test)
    Xt = torch.empty(n_test * P, D, dtype=torch.float32, device=dev)
    Lt = torch.empty(n_test * P, ps * ps, dtype=label_dtype, device=dev)
    _extract(model, test, Xt, Lt, 0, ps)
    if preproc is not None:
        preproc.fit(X[n_val * P:])                    # never on val / test
        preproc.transform(X)
        preproc.transform(Xt)
    return SegSplits(X, L, Xt, Lt, n_val, P)


def _check_classifiers(classifiers: Sequence[str]) -> None:
    for name in classifiers:
        if name not in classifiers_dict:
            raise ValueError(f"unknown classifier {name!r}")


def eval_features(feats: SegSplits, classifiers: Sequence[str] = ("logreg", "knn"), ignore_labels: Sequence[int] = (0, 255),
                  classifiers_kwargs: Optional[Dict[str, Dict[str, Any]]] = None) -> Dict[str, float]:
    """The classifier loop of ``eval_model`` (eval_segmentation.py:417-468) on extracted splits, with the reference's default
    classifiers: per classifier the hyper-parameter search on train against val (``hparam_fitting.<classifier>.<name>``), the
    refit on train + val (:441-444) and ``labels_<classifier>_mIoU`` / ``labels_<classifier>_acc`` on test.  The refit sees the
    validation rows first, the reference train first: for k-NN that changes outcomes only where distances tie exactly."""
    _check_classifiers(classifiers)
    X, L, Xt, Lt, nv = feats.X, feats.L, feats.Xt, feats.Lt, feats.n_val * feats.P
    Xv, Lv, Xtr, Ltr = X[:nv], L[:nv], X[nv:], L[nv:]
    results: Dict[str, float] = {}
    for name in classifiers:
        kw = (classifiers_kwargs or {}).get(name, {})
        clf = classifiers_dict[name](ignore_labels=ignore_labels, **kw)
        for k, v in clf.select_hparams(Xtr, Ltr, Xv, Lv).items():
            results[f"hparam_fitting.{name}.{k}"] = v
        clf.fit(X, L)                                 # train + val
        preds = clf.predict(Xt)
        for metric_name, metric in metrics_dict.items():
            results[f"labels_{name}_{metric_name}"] = float(metric(Lt, preds, ignore_labels))
        del clf
    return results


def eval_model(model, train, test, val=None, classifiers: Sequence[str] = ("logreg",),
               standardization: Optional[str] = "StandardScaler", ignore_labels: Sequence[int] = (0, 255), val_seed: int = 0,
               classifiers_kwargs: Optional[Dict[str, Dict[str, Any]]] = None) -> Dict[str, float]:
    """The logreg half of ``eval_model`` (eval_segmentation.py:346-470): ``extract_splits`` then ``eval_features``.  Train and
    validation features share ONE resident matrix, validation rows first, so the hyper-parameter fits and the final refit on
    train + val (:441-444) are row ranges of it.  Returns the reference's keys:
    ``hparam_fitting.logreg.mIoU_C=..._max_iter=..._tol=..._linesearch_max_iter=..._lbfgs_hessian_rank=...``,
    ``labels_logreg_mIoU``, ``labels_logreg_acc``.  "knn" is refused HERE (call ``extract_splits`` + ``eval_features`` for the
    reference's default pair of classifiers)."""
    for name in classifiers:
        if name == "knn":
            raise NotImplementedError("the k-NN classifier of the segmentation evaluation is not implemented on the HIP engine")
        if name not in classifiers_dict:
            raise ValueError(f"unknown classifier {name!r}")
    feats = extract_splits(model, train, test, val=val, standardization=standardization, val_seed=val_seed)
    return eval_features(feats, classifiers=classifiers, ignore_labels=ignore_labels, classifiers_kwargs=classifiers_kwargs)
