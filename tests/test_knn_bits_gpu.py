"""The two k-NN searches (csrc/segknn.hip, csrc/knn_cls.hip) return the BITS that the commit before their shared stream core
(csrc/knn_common.hpp) returned.

The other GPU tests of these kernels would not notice a changed accumulation order: integer features are exact in any order and
the float64-oracle tests allow a bar.  Here the inputs are real-valued (Gaussian rows times a per-row scale in [0.25, 4], from
numpy seeds below) and tests/golden/knn_parent_bits.npz holds what the library of the commit named in its ``parent_commit``
returned for them on an MI355X: ``idx`` as int32, ``dist`` / ``sim`` as the int32 view of the f32 bits.  Every run - every split
count, and for the segmentation side the two single-metric kernels next to KNN_BOTH - must equal that one answer exactly.
The shapes are the smallest that cross every edge of the shared core: a query-tile edge (130 rows; 67 and 3 for a partly filled
tile), a key-tile tail (389 = 3 x 128 + 5), 2 and 6 channel chunks, a merge (3 requested splits become 2 of 389 keys, 3 of 1000),
one quad per lane of the classification insert (kmax = 37) and all four (256).

    python tests/test_knn_bits_gpu.py --record OUT.npz --commit HASH
records the fixture; it is run ONCE, against a library built from the parent commit, never against the code under test."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "knn_parent_bits.npz")
SPLITS = (0, 1, 3)
# (name, D, n, M, kmax, skipped share of the keys, all-zero query row or None, seed)
SEG_CASES = [("seg_D64", 64, 130, 389, 30, 0.1, 77, 6401), ("seg_D192", 192, 67, 1000, 32, 0.0, None, 19201)]
CLS_CASES = [("cls_D64", 64, 130, 389, 37, 6402), ("cls_D192", 192, 3, 1000, 256, 19202)]


def _rows(rng, n, D):
    return (rng.standard_normal((n, D)) * rng.uniform(0.25, 4, size=(n, 1))).astype(np.float32)


def _inputs(D, n, M, seed, skip_frac=0.0, zero_row=None):
    rng = np.random.RandomState(seed)
    q, k = _rows(rng, n, D), _rows(rng, M, D)
    skip = rng.rand(M) < skip_frac
    if zero_row is not None:
        q[zero_row] = 0.0
    skip = torch.from_numpy(skip.astype(np.uint8)).to(DEV) if skip_frac else None
    return torch.from_numpy(q).to(DEV), torch.from_numpy(k).to(DEV), skip


def _bits(t):
    return t.view(torch.int32).cpu().numpy()


def _seg_runs(case):
    """Yields (what, {fixture key: int32 array}) for every (metrics, splits) of one segmentation case."""
    from octic_vits_amd import ops
    from test_seg_knn_gpu import run_knn
    name, D, n, M, kmax, frac, zero_row, seed = case
    Q, K, skip = _inputs(D, n, M, seed, frac, zero_row)
    for metrics in (ops.KNN_BOTH, ops.KNN_L2, ops.KNN_COSINE):
        for splits in SPLITS:
            res = run_knn(Q, K, skip, kmax, metrics, splits)
            got = {f"{name}_{key}": _bits(r) for key, r in zip(("idx_l2", "dist_l2", "idx_cos", "dist_cos"), res) if r is not None}
            yield f"{name} metrics={metrics} splits={splits}", got


def _cls_runs(case):
    from test_knn_cls_gpu import run_topk
    name, D, n, M, kmax, seed = case
    Q, K, _ = _inputs(D, n, M, seed)
    for splits in SPLITS:
        idx, sim = run_topk(Q, K, kmax, splits)
        yield f"{name} splits={splits}", {f"{name}_idx": _bits(idx), f"{name}_sim": _bits(sim)}


@pytest.fixture(scope="module")
def parent():
    return np.load(FIXTURE)


def _check(runs, parent):
    for what, got in runs:
        for key, v in got.items():
            assert parent[key].dtype == np.int32 and np.array_equal(v, parent[key]), f"{what}: {key} differs from the parent's bits"


@pytest.mark.parametrize("case", SEG_CASES, ids=lambda c: c[0])
def test_segmentation_lists_equal_the_parent_commits_bits(case, parent):
    _check(_seg_runs(case), parent)


@pytest.mark.parametrize("case", CLS_CASES, ids=lambda c: c[0])
def test_classification_lists_equal_the_parent_commits_bits(case, parent):
    _check(_cls_runs(case), parent)


def _record(path, commit):
    """The first run of every key is stored; the later runs of the same library must already agree with it."""
    stored = {"parent_commit": np.asarray(commit)}
    for case in SEG_CASES:
        for what, got in _seg_runs(case):
            for key, v in got.items():
                assert np.array_equal(stored.setdefault(key, v), v), f"{what}: {key} is not one answer"
    for case in CLS_CASES:
        for what, got in _cls_runs(case):
            for key, v in got.items():
                assert np.array_equal(stored.setdefault(key, v), v), f"{what}: {key} is not one answer"
    np.savez_compressed(path, **stored)
    print(f"recorded {len(stored) - 1} arrays from {commit} into {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "tests", "golden")]
    _record(sys.argv[sys.argv.index("--record") + 1], sys.argv[sys.argv.index("--commit") + 1])
