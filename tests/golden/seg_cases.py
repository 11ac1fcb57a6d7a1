"""The synthetic problems of the segmentation-evaluation goldens (tests/golden/seg_*.npz), shared by the maker and the tests.

The logreg fixture is ~6000 x 64 f32 - too large to commit - so the features are REGENERATED from a seed: numpy's legacy
``RandomState`` stream is frozen, and every step after it is an elementwise IEEE operation (f64 add, subtract, divide, one
cast to f32), so maker and tests hold bit-identical matrices; the golden stores the small inputs (class of each row, class
centres, the standardisation vectors) and a checksum.  Pure numpy: nothing here touches the reference or the GPU."""
import numpy as np

SEED = 20251017
N_TRAIN, N_HELD, D, K = 5000, 1000, 64, 7
LABEL_VALUES = np.asarray([3, 7, 12, 40, 41, 100, 200], dtype=np.uint8)     # non-contiguous label values of the 7 classes
IGNORE = (0, 255)
CS = (1e-3, 1.0, 100.0)
# the hyper-parameter selection fixture: a small, noisy training subset, so the three C values separate on validation
N_SELECT = 400
PIXELS = 4


def raw_features(cls, centers, seed=SEED):
    z = np.random.RandomState(seed).standard_normal((cls.shape[0], centers.shape[1]))
    return (z + centers[cls]).astype(np.float32)


def standardised(raw, mean, std):
    return ((raw.astype(np.float64) - mean) / std).astype(np.float32)


def logreg_features(g):
    """(X_train, X_held): the standardised f32 features of golden ``g`` (seg_logreg.npz), checked against its checksum."""
    X = standardised(raw_features(g["cls"], g["centers"]), g["mean"], g["std"])
    chk = np.asarray([X.astype(np.float64).sum(), (X.astype(np.float64) ** 2).sum(), float(X[17, 5]), float(X[-1, -1])])
    assert np.array_equal(chk, g["checksum"]), "the regenerated features differ from the maker's"
    return X[:N_TRAIN], X[N_TRAIN:]


def objective(X, y, C, dtype=np.float64):
    """fun(x) -> (J, g) of J = C sum CE(X W^T + b, y) + 1/2 |W|^2 with x = [W.ravel(), b]; the data term in ``dtype``."""
    Xd = X.astype(dtype)
    n, d = Xd.shape
    k = int(y.max()) + 1
    rows = np.arange(n)

    def fun(x):
        w64 = x[:k * d]
        W, b = w64.reshape(k, d).astype(dtype), x[k * d:].astype(dtype)
        z = Xd @ W.T + b
        m = z.max(1, keepdims=True)
        e = np.exp(z - m)
        s = e.sum(1, keepdims=True)
        loss = (np.log(s) + m)[:, 0] - z[rows, y]
        p = e / s
        p[rows, y] -= 1
        gW = dtype(C) * (p.T @ Xd) + W
        gb = dtype(C) * p.sum(0)
        J = C * float(loss.sum(dtype=np.float64)) + 0.5 * float(w64 @ w64)
        return J, np.concatenate([gW.ravel(), gb]).astype(np.float64)

    return fun


def pack(coef, intercept):
    return np.concatenate([np.asarray(coef, dtype=np.float64).ravel(), np.asarray(intercept, dtype=np.float64).ravel()])


def numpy_confusion(y_true, y_pred, ignore):
    """[256, 256] counts of (pixel label, predicted label) over the pixels whose label is not ignored."""
    t, p = np.asarray(y_true).reshape(-1).astype(np.int64), np.asarray(y_pred).reshape(-1).astype(np.int64)
    keep = ~np.isin(t, ignore)
    return np.bincount(t[keep] * 256 + p[keep], minlength=65536).reshape(256, 256)
