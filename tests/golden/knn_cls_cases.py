"""The clustered problem of the k-NN classification golden (tests/golden/knn_cls.npz), shared by the maker and the tests, and
the float64 restatement of the vote that the tests use as their oracle.

As in seg_knn_cases.py the f32 features are REGENERATED from a seed (numpy's legacy ``RandomState`` stream is frozen, every later
step is an elementwise IEEE operation or a row sum in f64 and one cast to f32); the golden stores the cluster of every row, the
centres, the labels and a checksum.  Pure numpy: nothing here touches the reference or the GPU."""
import numpy as np

N_KEYS, N_QUERIES, D, N_CLASSES = 400, 64, 64, 16
CENTER_SCALE, LABEL_NOISE = 0.6, 0.5
NB_KNN = (10, 20, 100, 200)
T = 0.07
FEWSHOT_NPC, FEWSHOT_TRIES = 5, 2
# An f32 inner product of unit-norm rows stays within BAR of the exact one (seg_knn_cases.BAR), so a similarity gap above twice
# that cannot reorder.  PROBA_BAR: two probas closer than this may be ordered either way by an f32 implementation.
BAR = 1e-5
PROBA_BAR = 2e-5
# the share of (query, k) whose top-5 hit may depend on the order of tied probas, per k of NB_KNN (asserted by the maker)
AMBIGUOUS_SHARE = (0.15, 0.05, 0.0, 0.0)


def features(cls, centers, seed):
    z = np.random.RandomState(int(seed)).standard_normal((cls.shape[0], centers.shape[1])) + centers[cls]
    return (z / np.sqrt((z * z).sum(1, keepdims=True))).astype(np.float32)


def checksum(X):
    X64 = X.astype(np.float64)
    return np.asarray([X64.sum(), (X64 ** 2).sum(), float(X[17, 5]), float(X[-1, -1])])


def problem(g):
    """keys [N_KEYS, D], key_labels, queries [N_QUERIES, D], query_labels of golden ``g``, checksum verified."""
    X = features(g["cls"], g["centers"], g["feature_seed"])
    assert np.array_equal(checksum(X), g["checksum"]), "the regenerated features differ from the maker's"
    return {"keys": X[:N_KEYS], "queries": X[N_KEYS:], "key_labels": g["labels"][:N_KEYS], "query_labels": g["labels"][N_KEYS:]}


def boundary_gaps(q, k, ks):
    """[n, len(ks)] float64: s[k-1] - s[k] of every query's descending similarities (inf where there is no k-th key)."""
    s = -np.sort(-(q.astype(np.float64) @ k.astype(np.float64).T), axis=1)
    return np.stack([s[:, kk - 1] - s[:, kk] if kk < s.shape[1] else np.full(s.shape[0], np.inf) for kk in ks], 1)


def oracle_probas(sim, idx, labels, C, inv_T, ks):
    """float64 [len(ks), n, C]: the reference's formula (softmax over all kmax similarities, each k a prefix sum) on the lists
    (sim, idx).  An index outside [0, len(labels)) or a label outside [0, C) casts no vote."""
    sim = np.asarray(sim, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    n, kmax = sim.shape
    z = np.where(np.isnan(sim), -np.inf, sim) * float(inv_T)
    m = z.max(1, keepdims=True)
    with np.errstate(invalid="ignore"):
        e = np.where(z == m, 1.0, np.exp(z - m))
    e = np.where(np.isneginf(m), 0.0, e)
    total = e.sum(1, keepdims=True)
    w = np.divide(e, total, out=np.zeros_like(e), where=total > 0)
    ok = (idx >= 0) & (idx < len(labels))
    lab = np.where(ok, np.asarray(labels, dtype=np.int64)[np.clip(idx, 0, len(labels) - 1)], -1)
    lab = np.where((lab >= 0) & (lab < C), lab, -1)
    out = np.zeros((len(ks), n, C))
    rows = np.arange(n)
    for i, k in enumerate(ks):
        for j in range(k):
            v = lab[:, j] >= 0
            np.add.at(out[i], (rows[v], lab[v, j]), w[v, j])
    return out


def rank_of_target(probas, targets):
    """[n] the number of classes ahead of the target under (proba descending, class index ascending); C for no valid target."""
    n, C = probas.shape
    t = np.asarray(targets, dtype=np.int64)
    ok = (t >= 0) & (t < C)
    pt = probas[np.arange(n), np.clip(t, 0, C - 1)][:, None]
    c = np.arange(C)[None, :]
    ahead = ((probas > pt) | ((probas == pt) & (c < t[:, None]))).sum(1)
    return np.where(ok, ahead, C)


def ambiguous(probas, targets, top, tol=PROBA_BAR):
    """[n] bool: whether 'the target is among the first ``top``' depends on the order inside the group of probas within tol of
    the target's (float64 probas)."""
    n, C = probas.shape
    pt = probas[np.arange(n), targets][:, None]
    above = (probas > pt + tol).sum(1)
    near = (np.abs(probas - pt) <= tol).sum(1) - 1            # without the target itself
    return (above < top) & (above + near >= top)
