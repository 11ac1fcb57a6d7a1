"""Generate tests/golden/knn_cls.npz by RUNNING THE REAL REFERENCE on the CPU: ``KnnModule``, ``create_class_indices_mapping``,
``filter_train`` and ``create_module_dict`` of dinov2/eval/knn.py, on a one-rank gloo group.  knn.py is imported by file path; the
packages it imports at module level that are absent here or not needed (constants, dinov2.data, dinov2.distributed,
dinov2.eval.metrics / setup / utils) are in-memory stand-ins, as in make_probe_golden.py.  torchmetrics is absent: micro top-1 /
top-5 come from the reference's probas with ``torch.topk``, as ``MulticlassAccuracy(top_k=k)`` takes them.  Nothing of the
reference is copied: the file holds labels, the rows' clusters, a checksum, probas, hit flags, accuracies, drawn indices and keys.

The problem (knn_cls_cases.py): 400 keys, 64 queries, D = 64, 16 Gaussian clusters with centre scale 0.6, rows L2-normalised,
50 % of the labels redrawn uniformly; nb_knn = (10, 20, 100, 200), T = 0.07; plus a few-shot case, n_per_class_list = [5] with
n_tries = 2 (the reference's k_list rule leaves k = 5).

Seed search.  (a) at every query the similarity gap across each boundary k of nb_knn (and across k = 5 of both few-shot tries)
exceeds twice the f32 bar of an inner product of unit rows, 2 x 1e-5; (b) the top-1 class leads by more than 2e-5 at every
(query, k).  Top-5 cannot be made tie-free at small k: a target with zero votes ties with every other zero class and torch.topk
leaves that order open.  So a (query, k) is marked AMBIGUOUS when its top-5 hit depends on the order inside the group of probas
within 2e-5 of the target's, and the tests compare hit flags with the reference only on the others.  Asserted here: the ambiguous
share is at most 15 % at k = 10, 5 % at k = 20 and zero at k = 100 and 200.

    python tests/golden/make_knn_cls_golden.py
"""
import argparse
import enum
import importlib.util
import os
import sys
from functools import partial

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import knn_cls_cases as KC  # noqa: E402
from _ref_import import REFERENCE_ROOT  # noqa: E402
from make_probe_golden import _module  # noqa: E402

BASE_SEED = 20261019


def load_knn():
    def absent(*a, **k):
        raise RuntimeError("stand-in: not available in the golden maker")

    class AccuracyAveraging(enum.Enum):
        MEAN_ACCURACY = "micro"

    _module("constants", IMAGENET_PATH="")
    for pkg in ("dinov2", "dinov2.eval"):
        _module(pkg).__path__ = []
    _module("dinov2.data", SamplerType=None, make_data_loader=absent, make_dataset=absent)
    _module("dinov2.data.transforms", make_classification_eval_transform=absent)
    sys.modules["dinov2"].distributed = _module(
        "dinov2.distributed", get_global_size=lambda: 1, get_global_rank=lambda: 0, is_enabled=lambda: False,
        is_main_process=lambda: True)
    _module("dinov2.eval.metrics", AccuracyAveraging=AccuracyAveraging, build_topk_accuracy_metric=absent)
    _module("dinov2.eval.setup", get_args_parser=lambda parents=None, add_help=True: argparse.ArgumentParser(add_help=False),
            setup_and_build_model=absent)
    _module("dinov2.eval.utils", ModelWithNormalize=absent, evaluate=absent, extract_features=absent)
    spec = importlib.util.spec_from_file_location("reference_knn", os.path.join(REFERENCE_ROOT, "dinov2", "eval", "knn.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.distributed.init_process_group("gloo", store=torch.distributed.HashStore(), rank=0, world_size=1)
    return mod


def draw(seed):
    rng = np.random.RandomState(seed)
    n = KC.N_KEYS + KC.N_QUERIES
    centers = rng.standard_normal((KC.N_CLASSES, KC.D)) * KC.CENTER_SCALE
    cls = rng.randint(0, KC.N_CLASSES, size=n)
    labels = cls.copy()
    flip = rng.rand(n) < KC.LABEL_NOISE
    labels[flip] = rng.randint(0, KC.N_CLASSES, size=int(flip.sum()))
    return cls.astype(np.int64), centers, labels.astype(np.int64)


def flags(probas, targets, top):
    """[n] bool from the reference's probas with torch.topk, as MulticlassAccuracy(top_k=top, average='micro') counts them."""
    return (probas.topk(top, dim=1).indices == targets[:, None]).any(1).numpy()


def record(out, prefix, p32, p64, targets, ks):
    """probas, hit flags, ambiguity and accuracies of one module; returns False where condition (b) fails."""
    t = targets.numpy()
    out[f"{prefix}_probas"] = np.stack([p32[k].numpy() for k in ks])
    out[f"{prefix}_top1"] = np.stack([flags(p32[k], targets, 1) for k in ks])
    out[f"{prefix}_top5"] = np.stack([flags(p32[k], targets, 5) for k in ks])
    out[f"{prefix}_ambiguous5"] = np.stack([KC.ambiguous(p64[k].numpy(), t, 5) for k in ks])
    out[f"{prefix}_acc1"] = out[f"{prefix}_top1"].mean(1)
    out[f"{prefix}_acc5"] = out[f"{prefix}_top5"].mean(1)
    for k in ks:
        top2 = p64[k].topk(2, dim=1).values
        if float((top2[:, 0] - top2[:, 1]).min()) <= KC.PROBA_BAR:
            return False
    return True


def main():
    E = load_knn()
    nb_knn = list(KC.NB_KNN)
    tried = 0
    for off in range(100000):
        seed = BASE_SEED + off
        cls, centers, labels = draw(seed)
        X = KC.features(cls, centers, seed)
        keys, queries = X[:KC.N_KEYS], X[KC.N_KEYS:]
        if KC.boundary_gaps(queries, keys, nb_knn).min() <= 2 * KC.BAR:
            continue
        train_labels = torch.from_numpy(labels[:KC.N_KEYS])
        targets = torch.from_numpy(labels[KC.N_KEYS:])
        mapping = E.create_class_indices_mapping(train_labels)
        drawn = [E.filter_train(mapping, KC.FEWSHOT_NPC, seed=t) for t in range(KC.FEWSHOT_TRIES)]
        if min(len(v) for v in mapping.values()) < KC.FEWSHOT_NPC:
            continue
        if any(KC.boundary_gaps(queries, keys[d.numpy()], [KC.FEWSHOT_NPC]).min() <= 2 * KC.BAR for d in drawn):
            continue
        tried += 1
        print(f"seed offset {off}: every boundary gap exceeds twice the f32 bar; running the reference")
        out, ok = {}, True
        res = {}
        for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
            module = partial(E.KnnModule, T=KC.T, device="cpu", num_classes=KC.N_CLASSES)
            md = E.create_module_dict(module=module, n_per_class_list=[-1, KC.FEWSHOT_NPC], n_tries=KC.FEWSHOT_TRIES, nb_knn=nb_knn,
                                      train_features=torch.from_numpy(keys).to(dt), train_labels=train_labels)
            with torch.no_grad():
                res[name] = md(torch.from_numpy(queries).to(dt))
            if name == "f32":
                out["module_keys"] = np.asarray(list(md.keys()))
                out["try_keys"] = np.asarray(list(md[f"{KC.FEWSHOT_NPC} per class"].keys()))
                out["fewshot_k_list"] = np.asarray(md[f"{KC.FEWSHOT_NPC} per class"]["0"].nb_knn, dtype=np.int64)
                sims, nl = md["full"]["1"].compute_neighbors(torch.from_numpy(queries))
                out["full_neighbor_labels"] = nl.numpy()
        ok &= record(out, "full", res["f32"]["full"]["1"], res["f64"]["full"]["1"], targets, nb_knn)
        spread = max(float((res["f32"]["full"]["1"][k].double() - res["f64"]["full"]["1"][k]).abs().max()) for k in nb_knn)
        fk = [int(k) for k in out["fewshot_k_list"]]
        for t in range(KC.FEWSHOT_TRIES):
            a, b = res["f32"][f"{KC.FEWSHOT_NPC} per class"][str(t)], res["f64"][f"{KC.FEWSHOT_NPC} per class"][str(t)]
            ok &= record(out, f"fewshot{t}", a, b, targets, fk)
            spread = max(spread, max(float((a[k].double() - b[k]).abs().max()) for k in fk))
            out[f"fewshot{t}_rows"] = drawn[t].numpy()
        if not ok:
            print("  the top-1 class leads by 2e-5 or less somewhere: next seed")
            if tried >= 40:
                raise SystemExit("no seed met the maker's conditions")
            continue
        share = out["full_ambiguous5"].mean(1)
        print("  ambiguous top-5 share per k:", dict(zip(nb_knn, share.round(4))),
              "few-shot:", [float(out[f"fewshot{t}_ambiguous5"].mean()) for t in range(KC.FEWSHOT_TRIES)])
        assert all(s <= lim for s, lim in zip(share, KC.AMBIGUOUS_SHARE)), share
        break
    else:
        raise SystemExit("no seed met the maker's conditions")
    # the keys of the reference's results_dict after the averaging over tries (eval_knn), and of results_eval_knn.json
    keys = [("full", k) for k in nb_knn] + [(f"{KC.FEWSHOT_NPC} per class", k) for k in fk]
    out["result_keys"] = np.asarray([repr(k) for k in keys])
    out["result_line_keys"] = np.asarray([f"{k} Top {t}" for k in keys for t in (1, 5)])
    out["fewshot_acc1"] = np.mean([out[f"fewshot{t}_acc1"] for t in range(KC.FEWSHOT_TRIES)], 0)
    out["fewshot_acc5"] = np.mean([out[f"fewshot{t}_acc5"] for t in range(KC.FEWSHOT_TRIES)], 0)
    out.update(cls=cls, centers=centers, labels=labels, feature_seed=np.asarray(seed), seed_offset=np.asarray(off),
               checksum=KC.checksum(X), ref_f32_f64_spread=np.asarray(spread), nb_knn=np.asarray(nb_knn), temperature=np.asarray(KC.T))
    path = os.path.join(HERE, "knn_cls.npz")
    np.savez_compressed(path, **out)
    print("knn_cls.npz", os.path.getsize(path), "bytes; seed offset", off, "; f32-vs-f64 spread of the reference's probas", spread)
    print("accuracies:", out["full_acc1"], out["full_acc5"], out["fewshot_acc1"], out["fewshot_acc5"])
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
