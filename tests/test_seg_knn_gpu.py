"""csrc/segknn.hip and octic_vits_amd.segmentation.KNNClassifier on the GPU.

Exact tests: features are small integers, so every dot product and norm is exact in f32 in any summation order and the
expected neighbours are ``np.lexsort((index, distance))`` in int64 - compared with ``==``.  Integer data is full of exact
distance ties, which is what checks the (distance, index) rule across tile and split boundaries.
Real-valued tests: a float64 numpy oracle; the bar is the f32-MFMA error (about 1.5e-7 sum|a_i b_i| at K <= 1024, 3.5e-7 at
K = 4096) with about 10x margin: 1e-5 absolute on a cosine distance (sum|a_i b_i| <= |a||b|), 1e-5 (|a|^2 + |b|^2) on a
squared L2 distance.  No test here reads the reference or imports sklearn; tests/golden/seg_knn.npz holds what the reference's
own KNNClassifier and eval_model computed on the CPU (tests/golden/make_seg_knn_golden.py)."""
import os

import numpy as np
import pytest
import torch

import seg_knn_cases as KC

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IDX_GUARD, DIST_GUARD, GUARD_COLS = -7, -7.0, 3


def run_knn(Q, K, skip, kmax, metrics, splits):
    """seg_knn into sentinel-filled outputs GUARD_COLS wider than kmax; asserts the guard columns, returns the four [n, kmax]."""
    from octic_vits_amd import ops
    n = Q.shape[0]
    out = []
    for bit in (ops.KNN_L2, ops.KNN_COSINE):
        if metrics & bit:
            out += [torch.full((n, kmax + GUARD_COLS), IDX_GUARD, dtype=torch.int32, device=DEV),
                    torch.full((n, kmax + GUARD_COLS), DIST_GUARD, dtype=torch.float32, device=DEV)]
        else:
            out += [None, None]
    ops.seg_knn(Q, K, ops.seg_rownorms(Q), ops.seg_rownorms(K), skip, kmax, metrics, splits, out=out)
    res = []
    for o, guard in zip(out, (IDX_GUARD, DIST_GUARD) * 2):
        if o is None:
            res.append(None)
            continue
        assert bool((o[:, kmax:] == guard).all()), "a guard column was written"
        res.append(o[:, :kmax].contiguous())
    return res


def integer_case(D, n, M, skip_frac, stride, seed, pm1=False):
    rng = np.random.RandomState(seed)
    draw = (lambda shape: rng.randint(0, 2, size=shape) * 2 - 1) if pm1 else (lambda shape: rng.randint(-8, 9, size=shape))
    q = draw((n, D)).astype(np.int64)
    k = draw((M, D)).astype(np.int64)
    skip = (rng.rand(M) < skip_frac)
    Q = torch.from_numpy(q.astype(np.float32)).to(DEV)
    if stride == 1:
        K = torch.from_numpy(k.astype(np.float32)).to(DEV)
    else:                                             # the keys are every stride-th row of a larger matrix of other values
        big = torch.full((M * stride, D), 5.0, device=DEV)
        big[::stride] = torch.from_numpy(k.astype(np.float32)).to(DEV)
        K = big[::stride]
    return q, k, skip, Q, K


def expected_order(dist, skip, kmax):
    """[n, kmax] indices by (distance, index) over the keys that are not skipped; ``dist`` is int64 [n, M]."""
    keep = np.nonzero(~skip)[0]
    out = np.empty((dist.shape[0], kmax), dtype=np.int64)
    for i in range(dist.shape[0]):
        order = np.lexsort((keep, dist[i, keep]))
        out[i] = keep[order[:kmax]]
    return out


# (D, n, M, fraction of skipped keys, kmax, key stride); M = None: exactly kmax keys are not skipped
EXACT_CASES = [
    (64, 1, None, 0.5, 1, 1),
    (64, 127, 129, 0.0, 3, 1),
    (64, 129, 1000, 0.2, 30, 3),
    (64, 300, 2500, 0.0, 32, 1),
    (192, 1, 2500, 0.0, 30, 3),
    (192, 127, None, 0.5, 32, 1),
    (192, 129, 129, 0.0, 1, 3),
    (192, 300, 1000, 0.2, 3, 1),
    (64, 300, None, 0.3, 30, 3),
    (192, 300, 2500, 0.2, 32, 3),
]


def _exact_keys(D, n, M, frac, kmax, stride, seed, pm1):
    if M is None:                                     # exactly kmax listable keys among 150
        q, k, skip, Q, K = integer_case(D, n, 150, 0.0, stride, seed, pm1)
        skip[:] = True
        skip[np.random.RandomState(seed + 1).choice(150, kmax, replace=False)] = False
    else:
        q, k, skip, Q, K = integer_case(D, n, M, frac, stride, seed, pm1)
    skip_t = torch.from_numpy(skip.astype(np.uint8)).to(DEV) if skip.any() else None
    return q, k, skip, Q, K, skip_t


@pytest.mark.parametrize("case", EXACT_CASES, ids=lambda c: "D{}-n{}-M{}-skip{}-k{}-stride{}".format(*c))
def test_exact_neighbours_on_integer_features(case):
    """Squared L2 on integers in [-8, 8]: indices AND distances equal the int64 oracle for splits 0 (the plan's), 1 and 3;
    bitwise equal across the split counts, under a permutation of the query rows, and for the 'both' kernel against the two
    single-metric kernels."""
    from octic_vits_amd import ops
    D, n, M, frac, kmax, stride = case
    q, k, skip, Q, K, skip_t = _exact_keys(D, n, M, frac, kmax, stride, 100 + D + n + kmax, False)
    d2 = (q ** 2).sum(1)[:, None] + (k ** 2).sum(1)[None, :] - 2 * (q @ k.T)
    want = expected_order(d2, skip, kmax)
    want_d = np.take_along_axis(d2, want, 1).astype(np.float32)
    first = None
    for splits in (0, 1, 3):
        idx, dist, _, _ = run_knn(Q, K, skip_t, kmax, ops.KNN_L2, splits)
        assert np.array_equal(idx.cpu().numpy(), want), f"splits={splits}"
        assert np.array_equal(dist.cpu().numpy(), want_d), f"splits={splits}"
        first = first or (idx, dist)
        assert torch.equal(idx, first[0]) and torch.equal(dist, first[1])
    perm = torch.from_numpy(np.random.RandomState(7).permutation(n)).to(DEV)
    idx_p, dist_p, _, _ = run_knn(Q[perm].contiguous(), K, skip_t, kmax, ops.KNN_L2, 0)
    assert torch.equal(idx_p, first[0][perm]) and torch.equal(dist_p, first[1][perm])
    for splits in (1, 3):
        _, _, idx_c, dist_c = run_knn(Q, K, skip_t, kmax, ops.KNN_COSINE, splits)
        b = run_knn(Q, K, skip_t, kmax, ops.KNN_BOTH, splits)
        assert torch.equal(b[0], first[0]) and torch.equal(b[1], first[1])
        assert torch.equal(b[2], idx_c) and torch.equal(b[3].view(torch.int32), dist_c.view(torch.int32))


@pytest.mark.parametrize("case", EXACT_CASES[2:6] + EXACT_CASES[8:], ids=lambda c: "D{}-n{}-M{}-skip{}-k{}-stride{}".format(*c))
def test_exact_cosine_neighbours_on_sign_features(case):
    """+-1 features: every norm is sqrt(D), so the cosine order is the order of -dot; indices equal lexsort((index, -dot))."""
    from octic_vits_amd import ops
    D, n, M, frac, kmax, stride = case
    q, k, skip, Q, K, skip_t = _exact_keys(D, n, M, frac, kmax, stride, 200 + D + n + kmax, True)
    want = expected_order(-(q @ k.T), skip, kmax)
    first = None
    for splits in (0, 1, 3):
        _, _, idx, dist = run_knn(Q, K, skip_t, kmax, ops.KNN_COSINE, splits)
        assert np.array_equal(idx.cpu().numpy(), want), f"splits={splits}"
        first = first or (idx, dist)
        assert torch.equal(idx, first[0]) and torch.equal(dist.view(torch.int32), first[1].view(torch.int32))
    dot = np.take_along_axis(q @ k.T, want, 1)
    assert np.abs(first[1].cpu().numpy().astype(np.float64) - (1.0 - dot / D)).max() <= 1e-6


# (D, kmax, seed): the seeds were chosen on the CPU, from the float64 oracle alone, so that at most 2 % of the queries have a
# boundary gap within twice the bar (3 / 2 of 300 for L2 / cosine at D = 64, 3 / 2 at D = 1280).  kmax is 10 at D = 1280: the cosine
# distances of Gaussian rows concentrate there (std 1 / sqrt(D) = 0.028), the spacing of neighbours at rank 30 of 1800 is
# 3.5e-4 and 5 - 6 % of the queries lie within 2e-5 of a swap at ANY seed; at rank 10 the spacing is 1e-3.
REAL_CASES = [(64, 30, 97), (1280, 10, 1329)]


@pytest.mark.parametrize("D,kmax,seed", REAL_CASES, ids=lambda v: str(v))
def test_real_valued_neighbours_against_a_float64_oracle(D, kmax, seed):
    """Gaussian rows times a per-row scale in [0.25, 4], n = 300, M = 2000, 10 % of the keys skipped, both metrics in one pass
    with 3 splits.  Returned indices are distinct and not skipped, the returned distances are sorted and within the bar of
    their pair's f64 distance; the f64 distances of the returned indices, sorted, match the oracle's kmax
    smallest within the bar; the index SETS are equal on every query whose oracle gap d[kmax] - d[kmax-1] exceeds twice the
    bar, and at most 2 % of the queries may lie inside that gap (the seed is fixed on the CPU, so the oracle alone decides)."""
    from octic_vits_amd import ops
    n, M = 300, 2000
    rng = np.random.RandomState(seed)
    q = (rng.standard_normal((n, D)) * rng.uniform(0.25, 4, size=(n, 1))).astype(np.float32)
    k = (rng.standard_normal((M, D)) * rng.uniform(0.25, 4, size=(M, 1))).astype(np.float32)
    skip = rng.rand(M) < 0.1
    q64, k64 = q.astype(np.float64), k.astype(np.float64)
    qn, kn = (q64 ** 2).sum(1), (k64 ** 2).sum(1)
    dot = q64 @ k64.T
    oracle = {"L2": qn[:, None] + kn[None, :] - 2 * dot, "cosine": 1.0 - dot / np.sqrt(qn[:, None] * kn[None, :])}
    bar = {"L2": 1e-5 * (qn[:, None] + kn[None, :]), "cosine": np.full((n, M), 1e-5)}
    res = run_knn(torch.from_numpy(q).to(DEV), torch.from_numpy(k).to(DEV), torch.from_numpy(skip.astype(np.uint8)).to(DEV),
                  kmax, ops.KNN_BOTH, 3)
    for name, idx, dist in (("L2", res[0], res[1]), ("cosine", res[2], res[3])):
        idx = idx.cpu().numpy().astype(np.int64)
        dist = dist.cpu().numpy().astype(np.float64)
        d = np.where(skip[None, :], np.inf, oracle[name])
        order = np.argsort(d, axis=1, kind="stable")
        top = order[:, :kmax]
        assert idx.min() >= 0 and idx.max() < M and not skip[idx].any()
        assert all(len(set(row)) == kmax for row in idx.tolist())
        got_d = np.take_along_axis(oracle[name], idx, 1)
        own = np.abs(dist - got_d) / np.take_along_axis(bar[name], idx, 1)
        print(f"D={D} {name}: max |returned distance - f64 distance of the returned pair| / bar = {own.max():.3e}")
        assert own.max() <= 1.0 and np.all(np.diff(dist, axis=1) >= 0)          # the returned values: within the bar, sorted
        got_order = np.argsort(got_d, axis=1, kind="stable")
        got_sorted = np.take_along_axis(got_d, got_order, 1)
        got_bar = np.take_along_axis(np.take_along_axis(bar[name], idx, 1), got_order, 1)
        want_sorted = np.take_along_axis(d, top, 1)
        want_bar = np.take_along_axis(bar[name], top, 1)
        err = np.abs(got_sorted - want_sorted)
        print(f"D={D} {name}: max |distance - oracle| / bar = {(err / np.maximum(got_bar, want_bar)).max():.3e}")
        assert np.all(err <= np.maximum(got_bar, want_bar))
        gap = np.take_along_axis(d, order[:, kmax:kmax + 1], 1)[:, 0] - want_sorted[:, -1]
        edge = np.maximum(np.take_along_axis(bar[name], order[:, kmax - 1:kmax], 1), np.take_along_axis(bar[name], order[:, kmax:kmax + 1], 1))[:, 0]
        clear = gap > 2 * edge
        print(f"D={D} {name}: {int((~clear).sum())} of {n} queries inside the gap")
        assert (~clear).mean() <= 0.02
        same = np.asarray([set(a) == set(b) for a, b in zip(idx.tolist(), top.tolist())])
        assert same[clear].all()


@pytest.mark.parametrize("L", [16, 196, 256])
def test_vote_equals_torch_mode(L):
    """Random uint8 labels from 9 values and random neighbour lists, ks = (1, 3, 10, 30), against torch.mode on the CPU; rows
    0 .. 2 carry a constructed 2-way tie, a 3-way tie and a tie won by the ignored value 0."""
    from octic_vits_amd import ops
    g = torch.Generator().manual_seed(L)
    values = torch.tensor([0, 255, 3, 7, 12, 40, 41, 100, 200], dtype=torch.uint8)
    R, n, ks = 700, 333, (1, 3, 10, 30)
    labels = values[torch.randint(0, 9, (R, L), generator=g)]
    idx = torch.randint(0, R, (n, 32), generator=g, dtype=torch.int32)
    idx[0, :10] = torch.arange(10, dtype=torch.int32)
    labels[:10] = torch.tensor([41, 12, 41, 12, 12, 41, 41, 12, 12, 41], dtype=torch.uint8)[:, None]     # 5 : 5 at k = 10 -> 12
    idx[1, :3] = torch.arange(10, 13, dtype=torch.int32)
    labels[10:13] = torch.tensor([200, 7, 40], dtype=torch.uint8)[:, None]                            # 1 : 1 : 1 at k = 3 -> 7
    idx[2, :10] = torch.arange(13, 23, dtype=torch.int32)
    labels[13:23] = torch.tensor([3, 0, 3, 0, 0, 3, 3, 0, 0, 3], dtype=torch.uint8)[:, None]            # 5 : 5 with 0 -> 0
    got = ops.seg_knn_vote(idx.to(DEV), labels.to(DEV), ks)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (4, n, L)
    for i, k in enumerate(ks):
        want = labels[idx[:, :k].long()].mode(dim=1).values
        assert torch.equal(got[i].cpu(), want), k
    assert int(got[2, 0, 0]) == 12 and int(got[1, 1, 0]) == 7 and int(got[2, 2, 0]) == 0
    # a strided neighbour list and int64 labels give the same votes
    wide = torch.full((n, 40), -1, dtype=torch.int32)
    wide[:, :32] = idx
    assert torch.equal(ops.seg_knn_vote(wide.to(DEV)[:, :32], labels.long().to(DEV), ks), got)


# ------------------------------------------------------------------------------------------------ against the reference
def _golden():
    g = np.load(os.path.join(GOLDEN, "seg_knn.npz"))
    return g, KC.problem(g)


@pytest.mark.parametrize("sub", [1, 3])
def test_classifier_equals_the_reference_on_every_grid_point(sub):
    """predict_grid, predict and select_hparams against the reference's KNNClassifier (CPU, float32 torch) on the clustered
    problem of the golden: identical [n, L] predictions at all 8 grid points, the same keys in the same order, scores equal to
    1e-12 (ratios of integer counts) and the same chosen point.  The maker kept a seed at which no query has an f64 neighbour
    gap below 1e-4 relative at any k of the grid, so equality is the right comparison."""
    from octic_vits_amd import segmentation as S
    g, p = _golden()
    Xk, Lk, Xq, Lq = (torch.from_numpy(p[k]).to(DEV) for k in ("keys", "key_labels", "queries", "query_labels"))
    clf = S.KNNClassifier(ignore_labels=KC.IGNORE, train_set_subsampling=sub)
    clf.fit(Xk, Lk)
    assert int(clf.skip_.sum()) > 0                              # ignored patches are in the fixture
    grid = clf.predict_grid(Xq, KC.KS, KC.DISTANCES)
    for i, (k, d) in enumerate(KC.grid()):
        assert np.array_equal(grid[(k, d)].cpu().numpy(), g[f"pred_sub{sub}"][i]), (k, d)
        clf.num_neighbors, clf.distance = k, d
        assert torch.equal(clf.predict(Xq), grid[(k, d)])
    sel = S.KNNClassifier(ignore_labels=KC.IGNORE, train_set_subsampling=sub)
    metrics = sel.select_hparams(Xk, Lk, Xq, Lq)
    assert list(metrics) == list(g[f"select_names_sub{sub}"])
    assert np.abs(np.asarray(list(metrics.values())) - g[f"select_scores_sub{sub}"]).max() <= 1e-12
    assert (sel.num_neighbors, sel.distance) == (int(g[f"best_k_sub{sub}"]), str(g[f"best_distance_sub{sub}"]))
    one = S.KNNClassifier(ignore_labels=KC.IGNORE, num_neighbors=(3,), distance=("L2",))
    assert one.select_hparams(Xk, Lk, Xq, Lq) == {} and (one.num_neighbors, one.distance) == (3, "L2")
    with pytest.raises(ValueError):                              # more neighbours than listable keys
        few = S.KNNClassifier(ignore_labels=KC.IGNORE, num_neighbors=(30,))
        few.fit(Xk[:20], Lk[:20])
        few.predict(Xq)


def test_eval_features_keys_equal_the_reference():
    """eval_features on splits built from the golden's rows: the reference's eval_model(classifiers=("knn",)) key list, and the
    test metrics it recorded (the refit sees val first instead of train first: no distance ties at this seed)."""
    from octic_vits_amd import segmentation as S
    g, p = _golden()
    n_val = int(g["eval_n_val_rows"])
    X = torch.from_numpy(p["keys"]).to(DEV)                      # the validation rows are the first n_val keys
    L = torch.from_numpy(p["key_labels"]).to(DEV)
    feats = S.SegSplits(X, L, torch.from_numpy(p["queries"]).to(DEV), torch.from_numpy(p["query_labels"]).to(DEV), n_val, 1)
    res = S.eval_features(feats, classifiers=("knn",), ignore_labels=KC.IGNORE)
    assert sorted(res) == list(g["eval_model_keys"])
    assert list(res)[:8] == ["hparam_fitting.knn." + s for s in g["select_names_sub1"]]
    assert list(res)[8:] == ["labels_knn_mIoU", "labels_knn_acc"]
    assert np.abs(np.asarray(list(res.values())[:8]) - g["eval_select_scores"]).max() <= 1e-12
    for key in ("labels_knn_mIoU", "labels_knn_acc"):
        assert abs(res[key] - float(g["eval_" + key])) <= 1e-12, key


def test_extract_splits_and_eval_features_share_the_backbone_pass():
    """extract_splits + eval_features(("logreg", "knn")) on the tiny hybrid model of test_seg_gpu.py: the logreg entries equal
    eval_model's bitwise, the knn entries follow with the reference's names."""
    from octic_vits_amd import dinov2_models
    from octic_vits_amd import segmentation as S
    torch.manual_seed(4)
    model = dinov2_models._dinov2(4, 256, 10, 4, False, 2, dict(img_size=32)).to(DEV).eval()
    g = torch.Generator().manual_seed(21)

    def batches(n_img, bs):
        out = []
        for i in range(0, n_img, bs):
            b = min(bs, n_img - i)
            lab = torch.tensor([0, 255, 3, 7, 12], dtype=torch.uint8)[torch.randint(0, 5, (b, 8, 8), generator=g)]
            out.append((torch.randn(b, 3, 32, 32, generator=g), lab.repeat_interleave(4, 1).repeat_interleave(4, 2)))
        return out

    train, test = batches(20, 8), batches(4, 4)
    kw = {"logreg": {"C": (0.01, 1.0), "max_iter": (5,)}, "knn": {"num_neighbors": (1, 10), "distance": ("cosine", "L2")}}
    ref = S.eval_model(model, train, test, classifiers=("logreg",), classifiers_kwargs=kw, val_seed=3)
    feats = S.extract_splits(model, train, test, val_seed=3)
    assert feats.n_val == 2 and feats.P == 64 and tuple(feats.X.shape) == (20 * 64, 256) and tuple(feats.L.shape) == (20 * 64, 16)
    res = S.eval_features(feats, classifiers_kwargs=kw)
    assert list(res)[:len(ref)] == list(ref) and all(res[k] == ref[k] for k in ref)
    assert list(res)[len(ref):] == ["hparam_fitting.knn.mIoU_num_neighbors=1_distance=cosine",
                                    "hparam_fitting.knn.mIoU_num_neighbors=1_distance=L2",
                                    "hparam_fitting.knn.mIoU_num_neighbors=10_distance=cosine",
                                    "hparam_fitting.knn.mIoU_num_neighbors=10_distance=L2", "labels_knn_mIoU", "labels_knn_acc"]
    assert all(isinstance(v, float) and 0.0 <= v <= 1.0 for v in res.values())
    with pytest.raises(NotImplementedError):
        S.eval_model(model, train, test, classifiers=("knn",))
