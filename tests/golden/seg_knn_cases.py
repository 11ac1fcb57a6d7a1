"""The clustered problem of the k-NN segmentation golden (tests/golden/seg_knn.npz), shared by the maker and the tests.

As in seg_cases.py the f32 features are REGENERATED from a seed (numpy's legacy ``RandomState`` stream is frozen, every later
step is an elementwise IEEE operation in f64 and one cast to f32); the golden stores the class and scale of every row, the
class centres, the pixel labels and a checksum.  Pure numpy: nothing here touches the reference or the GPU."""
import itertools

import numpy as np

N_KEYS, N_QUERIES, D, L, K = 400, 160, 64, 16, 6
LABEL_VALUES = np.asarray([3, 7, 12, 40, 41, 100], dtype=np.uint8)
IGNORE = (0, 255)
KS = (1, 3, 10, 30)
DISTANCES = ("cosine", "L2")
SUBSAMPLINGS = (1, 3)
N_VAL = 40                      # eval_model fixture: keys [0, N_VAL) are the validation rows, the rest the training rows
# The distance bars of tests/test_seg_knn_gpu.py: an f32 implementation stays within BAR of the exact cosine distance and within
# BAR (|a|^2 + |b|^2) of the exact squared L2 distance, so a neighbour gap above twice that cannot reorder.
BAR = 1e-5


def grid():
    return list(itertools.product(KS, DISTANCES))


def features(cls, scale, centers, seed):
    z = np.random.RandomState(int(seed)).standard_normal((cls.shape[0], centers.shape[1]))
    return ((z + centers[cls]) * scale[:, None]).astype(np.float32)


def checksum(X):
    X64 = X.astype(np.float64)
    return np.asarray([X64.sum(), (X64 ** 2).sum(), float(X[17, 5]), float(X[-1, -1])])


def problem(g):
    """keys [N_KEYS, D], key_labels [N_KEYS, L], queries [N_QUERIES, D], query_labels of golden ``g``, checksum verified."""
    X = features(g["cls"], g["scale"], g["centers"], g["feature_seed"])
    assert np.array_equal(checksum(X), g["checksum"]), "the regenerated features differ from the maker's"
    return {"keys": X[:N_KEYS], "queries": X[N_KEYS:], "key_labels": g["key_labels"], "query_labels": g["query_labels"]}


def oracle_distances(q, k):
    """float64 (squared L2, cosine) distance matrices and their gap thresholds 2 BAR (|a|^2 + |b|^2) / 2 BAR."""
    q, k = q.astype(np.float64), k.astype(np.float64)
    qn, kn = (q ** 2).sum(1), (k ** 2).sum(1)
    dot = q @ k.T
    return {"L2": (qn[:, None] + kn[None, :] - 2 * dot, 2 * BAR * (qn[:, None] + kn[None, :])),
            "cosine": (1.0 - dot / np.sqrt(qn[:, None] * kn[None, :]), np.full(dot.shape, 2 * BAR))}


def close_gaps(q, k, keep, rel=None):
    """Number of (query, k in KS, distance) whose neighbour gap d[k] - d[k-1] over the kept keys is not above the threshold:
    twice the f32 bar by default, ``rel`` x d[k] when given."""
    bad = 0
    for name, (d, thr) in oracle_distances(q, k[keep]).items():
        if name == "L2" and rel is not None:
            d = np.sqrt(np.maximum(d, 0.0))           # the reference orders by the root
        order = np.argsort(d, axis=1)
        ds = np.take_along_axis(d, order, 1)
        ts = np.take_along_axis(thr, order, 1)
        for kk in KS:
            if kk >= ds.shape[1]:
                continue
            gap = ds[:, kk] - ds[:, kk - 1]
            limit = rel * np.abs(ds[:, kk]) if rel is not None else np.maximum(ts[:, kk], ts[:, kk - 1])
            bad += int((gap <= limit).sum())
    return bad
