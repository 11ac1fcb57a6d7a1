"""Generate tests/golden/seg_knn_bf16.npz by RUNNING THE REAL REFERENCE on the CPU at ``dtype="bfloat16"`` - the value its
eval_config.yaml ships for both datasets: ``KNNClassifier(dtype="bfloat16", device="cpu")`` of
dinov2/eval/segmentation/eval_segmentation.py, imported through make_seg_golden.load_reference with ``torch.compile`` replaced
by the identity, as make_seg_knn_golden.py does.  Nothing of the reference is copied: the file holds uint16 bit patterns of
distances, uint8 predictions, names, scores and the numbers that regenerate the features.

Stored, on the seg_knn_cases.py problem (drawn by make_seg_knn_golden.draw from this file's own seed):
  ref_<distance>_sub<s>   the reference's ``_cdist`` of the bf16 queries against the bf16 keys[::s], ALL of them (the tests mask
                          the ignored ones), as bf16 bit patterns; distances "L2" (the root, as the reference ranks it) and "cosine"
  pred_sub<s>             its predictions at the 8 grid points;  select_* / best_*: its select_hparams
  slack_<distance>        the bf16 steps by which the float64 ordering of the rounded operands (seg_knn_bf16_cases.f64_lists)
                          exceeds the reference's k-th distance, max over queries, k and both sub-samplings
  clear_sub<s>            the number of clear boundaries per (distance, k) cell, in the order of seg_knn_cases.grid()

A seed is accepted only if (seg_knn_bf16_cases.py has the definitions)
  (a) at least 40 % of the (query, k, distance) boundaries against all keys are clear and every (distance, k) cell has at
      least 8 clear queries - so the set and prediction comparisons of the tests bite;
  (b) the float64 ordering of the bf16-rounded operands is a valid top-k of the reference's distances within MAX_SLACK steps
      (L2: 0, cosine: 1), for both sub-samplings.

    python tests/golden/make_seg_knn_bf16_golden.py
"""
import logging
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
torch.compile = lambda *a, **k: (a[0] if a and callable(a[0]) else (lambda f: f))   # before the reference is imported

import seg_knn_bf16_cases as BC  # noqa: E402
import seg_knn_cases as KC  # noqa: E402
from make_seg_golden import load_reference  # noqa: E402
from make_seg_knn_golden import BASE_SEED, draw  # noqa: E402


def bits(t):
    assert t.dtype == torch.bfloat16
    return t.contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def run_reference(E, X, labels):
    keys, queries = torch.from_numpy(X[:KC.N_KEYS]), torch.from_numpy(X[KC.N_KEYS:])
    kl, ql = torch.from_numpy(labels[:KC.N_KEYS]), torch.from_numpy(labels[KC.N_KEYS:])
    keep_all = BC.kept(labels[:KC.N_KEYS])
    assert np.array_equal(keep_all, ~np.isin(kl.mode(dim=-1).values.numpy(), KC.IGNORE))
    out, slack = {}, {d: -10 ** 9 for d in KC.DISTANCES}
    for sub in KC.SUBSAMPLINGS:
        clf = E.KNNClassifier(ignore_labels=KC.IGNORE, train_set_subsampling=sub, device="cpu", dtype="bfloat16")
        assert clf.dtype == torch.bfloat16
        clf.fit(keys, kl)
        assert clf.train_X.dtype == torch.bfloat16
        keep = keep_all[::sub]
        ref = {}
        for d in KC.DISTANCES:
            clf.distance = d
            dist = clf._cdist(queries.to(torch.bfloat16), keys[::sub].to(torch.bfloat16))
            ref[d] = out[f"ref_{d}_sub{sub}"] = bits(dist)
        counts = BC.clear_counts(ref, keep)
        total = sum(counts.values())
        print(f"sub {sub}: clear boundaries {total} of {KC.N_QUERIES * len(counts)} "
              f"({100.0 * total / (KC.N_QUERIES * len(counts)):.1f} %), smallest cell {min(counts.values())}")
        if sub == 1 and not BC.condition_a(counts, KC.N_QUERIES):
            return None
        out[f"clear_sub{sub}"] = np.asarray([counts[(d, k)] for k, d in KC.grid()])
        lists = BC.f64_lists(X[KC.N_KEYS:], X[:KC.N_KEYS][::sub], keep, KC.KS[-1])
        for d in KC.DISTANCES:
            s = BC.slack_steps(ref[d], keep, lists[d])
            print(f"sub {sub} {d}: the f64 ordering of the rounded operands exceeds the reference's k-th distance by {s} bf16 steps")
            slack[d] = max(slack[d], s)
        preds = []
        for k, d in KC.grid():
            clf.num_neighbors, clf.distance = k, d
            p = clf.predict(queries)
            assert p.dtype == torch.uint8 and tuple(p.shape) == (KC.N_QUERIES, KC.L)
            preds.append(p.numpy().copy())
        out[f"pred_sub{sub}"] = np.stack(preds)
        sel = E.KNNClassifier(ignore_labels=KC.IGNORE, train_set_subsampling=sub, device="cpu", dtype="bfloat16")
        metrics = sel.select_hparams(keys, kl, queries, ql)
        print(f"sub {sub}:", {k: round(v, 4) for k, v in metrics.items()}, "->", sel.num_neighbors, sel.distance)
        out[f"select_names_sub{sub}"] = np.asarray(list(metrics.keys()))
        out[f"select_scores_sub{sub}"] = np.asarray(list(metrics.values()))
        out[f"best_k_sub{sub}"], out[f"best_distance_sub{sub}"] = np.asarray(sel.num_neighbors), np.asarray(sel.distance)
    if any(slack[d] > BC.MAX_SLACK[d] for d in KC.DISTANCES):
        return None
    for d in KC.DISTANCES:
        out[f"slack_{d}"] = np.asarray(max(slack[d], 0))
    return out


def main():
    logging.disable(logging.CRITICAL)
    _, E = load_reference()
    for off in range(40):
        seed = BASE_SEED + off
        cls, scale, centers, labels = draw(seed)
        X = KC.features(cls, scale, centers, seed)
        print(f"seed offset {off}")
        out = run_reference(E, X, labels)
        if out is not None:
            break
    else:
        raise SystemExit("no seed met the maker's conditions")
    out.update(cls=cls.astype(np.int64), scale=scale, centers=centers, feature_seed=np.asarray(seed), seed_offset=np.asarray(off),
               key_labels=labels[:KC.N_KEYS], query_labels=labels[KC.N_KEYS:], checksum=KC.checksum(X))
    path = os.path.join(HERE, "seg_knn_bf16.npz")
    np.savez_compressed(path, **out)
    print("seg_knn_bf16.npz", os.path.getsize(path), "bytes; seed offset", off)
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
