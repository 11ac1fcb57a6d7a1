"""k-NN classification of a frozen backbone (the reference's dinov2/eval/knn.py) on one GPU, on the fused kernels of
csrc/knn_cls.hip: ``ops.knn_topk`` lists the max_k training rows with the largest inner product per query without writing the
similarity matrix, ``ops.knn_vote`` turns each list into the class probas of every k and counts top-1 / top-5 hits on the device.

What follows the reference: L2-normalised f32 class tokens as features (``ModelWithNormalize``), ``KnnModule`` with its
attributes and its arithmetic (the softmax over all max_k similarities at temperature T, each k summing a prefix),
``create_class_indices_mapping`` / ``filter_train`` / ``create_module_dict`` with the ``"full"`` / ``"{npc} per class"`` x tries
layout and the ``k_list`` rule, results keyed ``(n_per_class, k)`` and averaged over the tries, and the result lines of
``eval_knn_with_model``.

What is ours: the order of equal similarities (lower training row first; ``torch.topk`` leaves it open) and of equal probas
(lower class first); hit counters that stay on the device until the end of the evaluation, as ``LinearProbe.evaluate``.

Refused loudly: accuracy averaging other than MEAN_ACCURACY (``octic_vits_amd.metrics.eval_knn`` takes the others), ``gather_on_cpu``, a process group of more than one rank (the
reference shards the training features over ranks; this is a one-GPU evaluation), max(nb_knn) above the kernel's limit or above
the number of training rows, a feature width that is no multiple of 64, CPU tensors ("GPU only": there is no CPU fallback).
"""
import torch
import torch.nn.functional as F

KMAX = 256                     # ops.KNN_CLS_KMAX, the list length of knn_topk_kernel
DEFAULT_NB_KNN = (10, 20, 100, 200)


def _single_rank():
    if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
        raise NotImplementedError("octic_vits_amd.knn: a process group of more than one rank (the training features are not "
                                  "sharded here: this is a one-GPU evaluation)")


def _check_options(accuracy_averaging, gather_on_cpu):
    if str(getattr(accuracy_averaging, "value", accuracy_averaging)) != "mean_accuracy":
        raise NotImplementedError(f"octic_vits_amd.knn: accuracy averaging {accuracy_averaging!r} (only mean_accuracy; every "
                                  "other averaging is octic_vits_amd.metrics.eval_knn / eval_knn_features)")
    if gather_on_cpu:
        raise NotImplementedError("octic_vits_amd.knn: gather_on_cpu (the training features stay on the device)")
    _single_rank()


def extract_features(model, batches):
    """(features f32 [N, D] on the device, labels int64 [N]): a row is ``F.normalize(model(images).float(), dim=1, p=2)``, the
    rows in batch order.  ``model`` is anything whose eval forward returns the class token; it runs under the caller's autocast."""
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError("octic_vits_amd.knn.extract_features runs on the GPU only (no CPU fallback)")
    model.eval()
    feats, labels = [], []
    with torch.no_grad():
        for images, y in batches:
            out = model(images.to(dev, non_blocking=True))
            feats.append(F.normalize(out.float(), dim=1, p=2))
            labels.append(torch.as_tensor(y).to(dev, non_blocking=True).long().reshape(-1))
    if not feats:
        raise ValueError("octic_vits_amd.knn.extract_features: no batches")
    return torch.cat(feats).contiguous(), torch.cat(labels).contiguous()


class KnnModule(torch.nn.Module):
    """The reference's KnnModule on one device: ``forward(features)`` returns ``{k: probas [B, num_classes]}``."""

    def __init__(self, train_features, train_labels, nb_knn, T, num_classes=1000):
        super().__init__()
        _single_rank()
        self.nb_knn = [int(k) for k in nb_knn]
        self.max_k = max(self.nb_knn)
        self.T = float(T)
        self.num_classes = int(num_classes)
        self._ks = sorted(set(self.nb_knn))
        if train_features.dim() != 2 or train_labels.dim() != 1 or train_labels.shape[0] != train_features.shape[0]:
            raise ValueError("KnnModule: train_features [M, D] and train_labels [M]")
        M, D = train_features.shape
        if D % 64:
            raise ValueError(f"KnnModule: the feature width {D} must be a multiple of 64")
        if min(self.nb_knn) < 1 or self.max_k > KMAX:
            raise ValueError(f"KnnModule: nb_knn must lie in 1 .. {KMAX} (the kernel's list length), got {self.nb_knn}")
        if self.max_k > M:
            raise ValueError(f"KnnModule: max(nb_knn) = {self.max_k} exceeds the {M} training rows")
        if len(self._ks) > 8:
            raise ValueError("KnnModule: at most 8 distinct values of k")
        if self.num_classes < 5:
            raise ValueError("KnnModule: top-5 needs at least 5 classes")
        if not self.T > 0:
            raise ValueError("KnnModule: the temperature must be positive")
        self.train_features = train_features.float().contiguous()
        self.candidates = train_labels.long().contiguous()
        self.counters = None
        self.seen = 0

    def _need_gpu(self, features):
        if not (self.train_features.is_cuda and features.is_cuda):
            raise RuntimeError("octic_vits_amd.knn.KnnModule runs on the GPU only (no CPU fallback)")

    def _lists(self, features):
        from . import ops
        self._need_gpu(features)
        return ops.knn_topk(features.float().contiguous(), self.train_features, self.max_k)

    def compute_neighbors(self, features):
        """(topk_sims f32 [B, max_k], neighbors_labels int64 [B, max_k]), sorted by (similarity descending, row ascending)."""
        idx, sim = self._lists(features)
        return sim, self.candidates[idx.long()]

    def _vote(self, features, targets=None):
        from . import ops
        idx, sim = self._lists(features)
        if targets is not None:
            if self.counters is None:
                self.counters = torch.zeros(len(self._ks), 2, dtype=torch.int64, device=sim.device)
            targets = targets.to(sim.device).long().contiguous()
            self.seen += int(sim.shape[0])
        return ops.knn_vote(sim, idx, self.candidates, self.num_classes, 1.0 / self.T, self._ks, targets=targets,
                            counters=self.counters if targets is not None else None)

    def forward(self, features):
        probas = self._vote(features)
        return {k: probas[self._ks.index(k)] for k in self.nb_knn}

    def accumulate(self, features, targets):
        """forward + the top-1 / top-5 hits of this batch added to the device counters; nothing is read back."""
        probas = self._vote(features, targets)
        return {k: probas[self._ks.index(k)] for k in self.nb_knn}

    def accuracies(self):
        """{k: {"top-1": ..., "top-5": ...}} over everything accumulated so far (the one read-back)."""
        if not self.seen:
            raise RuntimeError("KnnModule.accuracies: nothing accumulated")
        hits = self.counters.cpu().tolist()
        return {k: {"top-1": hits[self._ks.index(k)][0] / self.seen, "top-5": hits[self._ks.index(k)][1] / self.seen}
                for k in self.nb_knn}


def create_class_indices_mapping(labels):
    """{class: the [count, 1] row indices of that class}, classes ascending (the reference's mapping with int keys)."""
    unique_labels, inverse = torch.unique(labels, return_inverse=True)
    return {int(unique_labels[i]): (inverse == i).nonzero() for i in range(len(unique_labels))}


def filter_train(mapping, n_per_class, seed):
    """The reference's draw: per class, in the mapping's order, the first n_per_class of a ``randperm``.  The reference seeds
    the global generator; a local CPU generator seeded the same way yields the same stream and leaves the global state alone."""
    g = torch.Generator().manual_seed(int(seed))
    final_indices = []
    for k in mapping.keys():
        index = torch.randperm(len(mapping[k]), generator=g)[:n_per_class]
        final_indices.append(mapping[k][index.to(mapping[k].device)])
    return torch.cat(final_indices).squeeze()


def k_list_for(nb_knn, npc):
    """The values of k a few-shot module votes with: the reference's sorted(k for k in set(nb_knn + [npc]) if k <= npc)."""
    return sorted(k for k in set(list(nb_knn) + [npc]) if k <= npc)


def create_module_dict(*, module, n_per_class_list, n_tries, nb_knn, train_features, train_labels):
    """{"full": {"1": module}, "{npc} per class": {"0": module, ...}} as the reference builds it; ``module`` is called with
    train_features / train_labels / nb_knn."""
    modules = {}
    mapping = create_class_indices_mapping(train_labels)
    for npc in n_per_class_list:
        if npc < 0:                       # only one try is needed with the full data
            modules["full"] = {"1": module(train_features=train_features, train_labels=train_labels, nb_knn=list(nb_knn))}
            continue
        tries = {}
        for t in range(n_tries):
            rows = filter_train(mapping, npc, seed=t).to(train_features.device)
            tries[str(t)] = module(train_features=train_features[rows], train_labels=train_labels[rows],
                                   nb_knn=k_list_for(nb_knn, npc))
        modules[f"{npc} per class"] = tries
    return modules


def eval_knn_features(train_features, train_labels, val_batches_of_features, nb_knn=DEFAULT_NB_KNN, temperature=0.07,
                      n_per_class_list=(-1,), n_tries=1, accuracy_averaging="mean_accuracy", gather_on_cpu=False):
    """The reference's eval_knn behind the feature extraction: ``{(n_per_class, k): {"top-1": ..., "top-5": ...}}``, averaged
    over the tries, with num_classes = train_labels.max() + 1.  val_batches_of_features: iterable of (features [B, D], labels)."""
    _check_options(accuracy_averaging, gather_on_cpu)
    if not train_features.is_cuda:
        raise RuntimeError("octic_vits_amd.knn.eval_knn_features runs on the GPU only (no CPU fallback)")
    train_labels = train_labels.to(train_features.device).long()
    num_classes = int(train_labels.max()) + 1

    def module(train_features, train_labels, nb_knn):
        return KnnModule(train_features, train_labels, nb_knn, temperature, num_classes=num_classes)

    modules = create_module_dict(module=module, n_per_class_list=list(n_per_class_list), n_tries=n_tries, nb_knn=list(nb_knn),
                                 train_features=train_features, train_labels=train_labels)
    for feats, targets in val_batches_of_features:
        for tries in modules.values():
            for m in tries.values():
                m.accumulate(feats, targets)
    results = {}
    for name, tries in modules.items():
        per_try = [m.accuracies() for m in tries.values()]
        for k in next(iter(tries.values())).nb_knn:
            results[(name, k)] = {key: sum(a[k][key] for a in per_try) / len(per_try) for key in ("top-1", "top-5")}
    return results


def eval_knn(model, train_batches, val_batches, nb_knn=DEFAULT_NB_KNN, temperature=0.07, n_per_class_list=(-1,), n_tries=1,
             accuracy_averaging="mean_accuracy", gather_on_cpu=False):
    """The reference's eval_knn on one GPU: features of the training set, then every validation batch through every module.
    train_batches / val_batches: iterables of (images, labels)."""
    _check_options(accuracy_averaging, gather_on_cpu)
    train_features, train_labels = extract_features(model, train_batches)

    def val_features():
        for images, y in val_batches:
            yield extract_features(model, [(images, y)])

    return eval_knn_features(train_features, train_labels, val_features(), nb_knn=nb_knn, temperature=temperature,
                             n_per_class_list=n_per_class_list, n_tries=n_tries)


def results_lines(results):
    """The entries the reference writes to results_eval_knn.json: ``"('full', 10) Top 1": 100 * accuracy``, Top 1 then Top 5."""
    out = {}
    for key, acc in results.items():
        out[f"{key} Top 1"] = float(acc["top-1"]) * 100.0
        out[f"{key} Top 5"] = float(acc["top-5"]) * 100.0
    return out
