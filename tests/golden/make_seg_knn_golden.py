"""Generate tests/golden/seg_knn.npz by RUNNING THE REAL REFERENCE on the CPU: ``KNNClassifier`` (fit, predict, select_hparams)
and ``eval_model(classifiers=("knn",))`` of dinov2/eval/segmentation/eval_segmentation.py, imported through
make_seg_golden.load_reference (the same in-memory stand-ins).  ``torch.compile`` is replaced by the identity before the
reference is imported (its ``_find_closest_chunk`` is decorated with it); ``device="cpu"`` is passed to the classifier.
Nothing of the reference is copied: the file holds names, scores, the chosen grid point and uint8 predictions.

The problem (seg_knn_cases.py): 400 keys and 160 queries in 6 overlapping Gaussian clusters, D = 64, a per-row scale in
[0.5, 2] (so the cosine and L2 orders differ), L = 16 pixels per patch with a second label value on some pixels, label noise,
and patches whose mode label is ignored (0 / 255).

Seed search.  Equality of predictions is the right comparison only where rounding cannot reorder neighbours.  A relative gap
of 1e-4 at EVERY (query, k, distance) cannot be had on a problem of this size: with a few hundred keys the relative spacing of
neighbouring distances is near 1e-2, so about one boundary gap in a hundred lies below 1e-4 and each seed has dozens of them
among its 3360 (34 at the first seed; the maker prints the count).  The condition used instead is the one the GPU test applies to its float64 oracle: every
boundary gap d[k] - d[k-1], k in (1, 3, 10, 30), must exceed TWICE the f32 error bar of the distance - 2e-5 absolute for the
cosine distance, 2e-5 (|a|^2 + |b|^2) for the squared L2 distance - for the queries against all keys, against every third key,
and for the validation rows against the training rows.  Any implementation within the bar then returns the same neighbour sets.
The two best select_hparams scores must also differ by >= 0.01 in each of the three searches.

    python tests/golden/make_seg_knn_golden.py
"""
import logging
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
torch.compile = lambda *a, **k: (a[0] if a and callable(a[0]) else (lambda f: f))   # before the reference is imported

import seg_knn_cases as KC  # noqa: E402
from make_seg_golden import DATASETS, IndexModel, TensorPairs, index_images, load_reference  # noqa: E402

BASE_SEED = 20261018


def draw(seed):
    """cls, scale, centers, pixel labels of keys then queries."""
    rng = np.random.RandomState(seed)
    n = KC.N_KEYS + KC.N_QUERIES
    centers = rng.standard_normal((KC.K, KC.D)) * 0.6
    cls = rng.randint(0, KC.K, size=n)
    scale = rng.uniform(0.5, 2.0, size=n)
    shown = cls.copy()
    flip = rng.rand(n) < 0.2                                   # label noise: the patch shows another class
    shown[flip] = rng.randint(0, KC.K, size=int(flip.sum()))
    second_values = np.concatenate([KC.LABEL_VALUES, np.asarray([0, 255], dtype=np.uint8)])
    labels = np.empty((n, KC.L), dtype=np.uint8)
    for i in range(n):
        n_a = rng.randint(9, KC.L + 1)
        px = np.asarray([KC.LABEL_VALUES[shown[i]]] * n_a + [rng.choice(second_values)] * (KC.L - n_a), dtype=np.uint8)
        labels[i] = rng.permutation(px)
    ignored = rng.rand(n) < 0.08                               # patches whose mode is an ignored value
    labels[ignored] = np.where(rng.rand(int(ignored.sum()), 1) < 0.5, 0, 255).astype(np.uint8)
    return cls, scale, centers, labels


def kept(labels):
    modes = torch.from_numpy(labels).mode(dim=-1).values.numpy()
    return ~np.isin(modes, KC.IGNORE)


def gaps(X, labels, rel=None):
    keys, queries = X[:KC.N_KEYS], X[KC.N_KEYS:]
    keep = kept(labels[:KC.N_KEYS])
    bad = 0
    for sub in KC.SUBSAMPLINGS:
        rows = np.arange(KC.N_KEYS)[::sub]
        bad += KC.close_gaps(queries, keys, rows[keep[::sub]], rel)
    train_rows = np.arange(KC.N_VAL, KC.N_KEYS)
    bad += KC.close_gaps(keys[:KC.N_VAL], keys, train_rows[keep[KC.N_VAL:]], rel)
    return bad


def separated(metrics):
    s = sorted(metrics.values())
    return s[-1] - s[-2] >= 0.01


def run_reference(E, X, labels):
    keys, queries = torch.from_numpy(X[:KC.N_KEYS]), torch.from_numpy(X[KC.N_KEYS:])
    kl, ql = torch.from_numpy(labels[:KC.N_KEYS]), torch.from_numpy(labels[KC.N_KEYS:])
    out = {}
    for sub in KC.SUBSAMPLINGS:
        clf = E.KNNClassifier(ignore_labels=KC.IGNORE, train_set_subsampling=sub, device="cpu")
        assert tuple(clf.hparam_grids["num_neighbors"]) == KC.KS and tuple(clf.hparam_grids["distance"]) == KC.DISTANCES
        clf.fit(keys, kl)
        preds = []
        for k, d in KC.grid():
            clf.num_neighbors, clf.distance = k, d
            p = clf.predict(queries)
            assert p.dtype == torch.uint8 and tuple(p.shape) == (KC.N_QUERIES, KC.L)
            preds.append(p.numpy().copy())
        out[f"pred_sub{sub}"] = np.stack(preds)
        sel = E.KNNClassifier(ignore_labels=KC.IGNORE, train_set_subsampling=sub, device="cpu")
        metrics = sel.select_hparams(keys, kl, queries, ql)
        print(f"sub {sub}:", {k: round(v, 4) for k, v in metrics.items()}, "->", sel.num_neighbors, sel.distance)
        if not separated(metrics):
            return None
        out[f"select_names_sub{sub}"] = np.asarray(list(metrics.keys()))
        out[f"select_scores_sub{sub}"] = np.asarray(list(metrics.values()))
        out[f"best_k_sub{sub}"], out[f"best_distance_sub{sub}"] = np.asarray(sel.num_neighbors), np.asarray(sel.distance)

    # ---- eval_model: one 4 x 4 image per patch; train = keys[N_VAL:], val = keys[:N_VAL], test = the queries
    ps = 4
    order = np.concatenate([np.arange(KC.N_VAL, KC.N_KEYS), np.arange(KC.N_VAL), np.arange(KC.N_KEYS, KC.N_KEYS + KC.N_QUERIES)])
    table = torch.from_numpy(X[order])                                      # IndexModel: image i is patch row i
    lab = torch.from_numpy(labels[order]).reshape(-1, ps, ps)
    n_tr = KC.N_KEYS - KC.N_VAL
    images = index_images(len(order), ps)
    DATASETS["knn_train"] = TensorPairs(images[:n_tr], lab[:n_tr])
    DATASETS["knn_val"] = TensorPairs(images[n_tr:KC.N_KEYS], lab[n_tr:KC.N_KEYS])
    DATASETS["knn_test"] = TensorPairs(images[KC.N_KEYS:], lab[KC.N_KEYS:])
    model = IndexModel(ps, KC.D, table)
    spy = {}
    orig = E.KNNClassifier.select_hparams

    def select(self, *a, **k):
        m = orig(self, *a, **k)
        spy["metrics"] = m
        return m

    E.KNNClassifier.select_hparams = select
    try:
        res = E.eval_model(model, train_dataset_name="knn_train", test_dataset_name="knn_test", val_dataset_name="knn_val",
                           classifiers=("knn",), standardization=None, classifiers_kwargs={"knn": {"device": "cpu"}},
                           ignore_labels=KC.IGNORE, batch_size=64, num_workers=0)
    finally:
        E.KNNClassifier.select_hparams = orig
    print("eval_model:", {k: round(v, 4) for k, v in res.items()})
    if not separated(spy["metrics"]):
        return None
    out["eval_model_keys"] = np.asarray(sorted(res.keys()))
    out["eval_labels_knn_mIoU"], out["eval_labels_knn_acc"] = np.asarray(res["labels_knn_mIoU"]), np.asarray(res["labels_knn_acc"])
    out["eval_select_scores"] = np.asarray(list(spy["metrics"].values()))
    out["eval_n_val_rows"] = np.asarray(KC.N_VAL)
    return out


def main():
    logging.disable(logging.CRITICAL)
    U, E = load_reference()
    tried = 0
    for off in range(200000):
        seed = BASE_SEED + off
        cls, scale, centers, labels = draw(seed)
        X = KC.features(cls, scale, centers, seed)
        if off == 0:
            print("boundary gaps below 1e-4 relative at the first seed:", gaps(X, labels, rel=1e-4))
        if gaps(X, labels):
            continue
        tried += 1
        print(f"seed offset {off}: no boundary gap within twice the f32 bar; running the reference")
        out = run_reference(E, X, labels)
        if out is not None:
            break
        if tried >= 40:
            raise SystemExit("no seed met the maker's conditions")
    else:
        raise SystemExit("no seed met the maker's conditions")
    out.update(cls=cls.astype(np.int64), scale=scale, centers=centers, feature_seed=np.asarray(seed), seed_offset=np.asarray(off),
               key_labels=labels[:KC.N_KEYS], query_labels=labels[KC.N_KEYS:], checksum=KC.checksum(X))
    path = os.path.join(HERE, "seg_knn.npz")
    np.savez_compressed(path, **out)
    print("seg_knn.npz", os.path.getsize(path), "bytes; seed offset", off)
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
