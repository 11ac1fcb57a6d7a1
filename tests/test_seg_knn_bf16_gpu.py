"""csrc/segknn.hip on rows of bf16 (octic_seg_rownorms_bf16, octic_seg_knn_bf16) and KNNClassifier(dtype="bfloat16") on the GPU.

The rule under test (include/octic_hip.h): operands are rounded to bf16 once, everything after that cast is f32 - so every
oracle here works on the ROUNDED operands.
Exact tests: integers in -8 .. 8 are bf16 values, their products and sums are exact in f32 in any order, so the expected
neighbours are ``np.lexsort((index, distance))`` in int64, compared with ``==`` - across tile edges, split counts, row strides.
Real-valued tests: a float64 oracle on the rounded operands with the bars of seg_knn_cases.BAR.  They hold for this path:
products of two bf16 values are exact in f32, and a dot is one f32 accumulator chain of D / 32 MFMA steps, so its error is at
most a few 2^-24 sum|a_i b_i| per step - 40 steps at D = 1280, 2.4e-6 sum|a_i b_i| against the bar of 1e-5 |a||b|.
Against the reference: tests/golden/seg_knn_bf16.npz holds the bf16 distances the reference's own KNNClassifier computed on
the CPU; our lists must be valid top-k answers of THOSE (tests/golden/seg_knn_bf16_cases.py has the definitions)."""
import os

import numpy as np
import pytest
import torch

import seg_knn_bf16_cases as BC
import seg_knn_cases as KC

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IDX_GUARD, DIST_GUARD, GUARD_COLS, GUARD_ROWS = -7, -7.0, 3, 2
BF16 = torch.bfloat16


def run16(Q, K, skip, kmax, metrics, splits):
    """seg_knn on bf16 rows into sentinel-filled outputs with GUARD_COLS more columns and GUARD_ROWS more rows than asked for;
    asserts that the guards are untouched and returns the four [n, kmax] (None for a metric not asked for)."""
    from octic_vits_amd import ops
    assert Q.dtype == BF16 and K.dtype == BF16
    n = Q.shape[0]
    bufs, out = [], []
    for bit in (ops.KNN_L2, ops.KNN_COSINE):
        for guard, dt in ((IDX_GUARD, torch.int32), (DIST_GUARD, torch.float32)):
            b = torch.full((n + GUARD_ROWS, kmax + GUARD_COLS), guard, dtype=dt, device=DEV) if metrics & bit else None
            bufs.append(b)
            out.append(b[:n] if b is not None else None)
    ops.seg_knn(Q, K, ops.seg_rownorms(Q), ops.seg_rownorms(K), skip, kmax, metrics, splits, out=out)
    res = []
    for b, guard in zip(bufs, (IDX_GUARD, DIST_GUARD) * 2):
        if b is None:
            res.append(None)
            continue
        assert bool((b[:, kmax:] == guard).all()) and bool((b[n:] == guard).all()), "a guard column or row was written"
        res.append(b[:n, :kmax].contiguous())
    return res


def wide_rows(x, pad, fill):
    """The bf16 rows of the numpy matrix x as a view with row stride D + pad of a wider matrix filled with ``fill``."""
    w = torch.full((x.shape[0], x.shape[1] + pad), fill, dtype=BF16, device=DEV)
    w[:, :x.shape[1]] = torch.from_numpy(x.astype(np.float32)).to(DEV)
    return w[:, :x.shape[1]]


def strided_rows(x, stride, fill):
    """The bf16 rows of x as every stride-th row of a larger matrix of other values."""
    if stride == 1:
        return torch.from_numpy(x.astype(np.float32)).to(DEV).to(BF16)
    big = torch.full((x.shape[0] * stride, x.shape[1]), fill, dtype=BF16, device=DEV)
    big[::stride] = torch.from_numpy(x.astype(np.float32)).to(DEV).to(BF16)
    return big[::stride]


def lex_order(dist, keep, kmax):
    rows = np.nonzero(keep)[0]
    return np.stack([rows[np.lexsort((rows, dist[i, rows]))[:kmax]] for i in range(dist.shape[0])])


# (D, n, M, kmax, key row stride): every D in (64, 128, 192), n in (1, 127, 128, 129), M in (kmax, 127, 128, 129, 3 * 128 + 5),
# kmax in (1, 31, 32).  n = 1, 127 and 129 leave query rows past n in the last tile.
EXACT_CASES = [
    (64, 1, 1, 1, 1),
    (64, 127, 127, 31, 2),
    (64, 128, 32, 32, 1),
    (128, 128, 128, 32, 1),
    (128, 129, 129, 31, 3),
    (128, 127, 389, 31, 1),
    (192, 129, 389, 32, 1),
    (192, 1, 389, 1, 2),
    (192, 128, 31, 31, 3),
]
SPLITS = (1, 2, 3, 64)


@pytest.mark.parametrize("case", EXACT_CASES, ids=lambda c: "D{}-n{}-M{}-k{}-stride{}".format(*c))
def test_exact_neighbours_on_integer_features(case):
    """Integers in [-8, 8].  Squared L2: indices AND distances equal the int64 oracle under (distance, index) for the forced
    splits 1, 2, 3 and 64.  Cosine: against the float64 oracle - returned distances within BAR of their pair's, sorted under
    the total order, and the index SET equal on every query whose boundary gap exceeds 2 BAR (the rule of the f32 test);
    bitwise equal across the split counts.  Both at once: bitwise the two single-metric launches.  Keys 126 .. 128, the two
    sides of a tile edge, are skipped where enough keys remain, with a random fifth of the others at M = 389; queries and keys
    have row strides above D; outputs have guard rows and columns."""
    from octic_vits_amd import ops
    D, n, M, kmax, stride = case
    rng = np.random.RandomState(1000 + D + 7 * n + 13 * M + kmax)
    q = rng.randint(-8, 9, size=(n, D)).astype(np.int64)
    k = rng.randint(-8, 9, size=(M, D)).astype(np.int64)
    skip = np.zeros(M, dtype=bool)
    if M - 3 >= kmax and M > 128:
        skip[126:129] = True
    if M == 389:
        skip |= rng.rand(M) < 0.2
        skip[388] = False                                  # the last key, alone with 4 others in the last tile, stays listable
    assert (~skip).sum() >= kmax
    Q, K = wide_rows(q, 8, 3.0), strided_rows(k, stride, 5.0)
    assert Q.stride(0) == D + 8 and K.stride(0) == stride * D
    skip_t = torch.from_numpy(skip.astype(np.uint8)).to(DEV) if skip.any() else None
    qn, kn, dot = (q ** 2).sum(1), (k ** 2).sum(1), q @ k.T
    d2 = qn[:, None] + kn[None, :] - 2 * dot
    want = lex_order(d2, ~skip, kmax)
    want_d = np.take_along_axis(d2, want, 1).astype(np.float32)
    cos = 1.0 - dot / np.sqrt((qn[:, None] * kn[None, :]).astype(np.float64))
    cos_kept = np.where(skip[None, :], np.inf, cos)
    cos_sorted = np.sort(cos_kept, axis=1)
    kth = cos_sorted[:, kmax - 1]
    clear = (cos_sorted[:, kmax] - kth > 2 * KC.BAR) if M > kmax else np.ones(n, dtype=bool)
    first = None
    for splits in SPLITS:
        il, dl, ic, dc = run16(Q, K, skip_t, kmax, ops.KNN_BOTH, splits)
        assert np.array_equal(il.cpu().numpy(), want), f"splits={splits}"
        assert np.array_equal(dl.cpu().numpy(), want_d), f"splits={splits}"
        first = first or (ic, dc)
        assert torch.equal(ic, first[0]) and torch.equal(dc.view(torch.int32), first[1].view(torch.int32)), f"splits={splits}"
    ic, dc = first[0].cpu().numpy().astype(np.int64), first[1].cpu().numpy().astype(np.float64)
    assert ic.min() >= 0 and ic.max() < M and not skip[ic].any() and all(len(set(r)) == kmax for r in ic.tolist())
    pair = np.take_along_axis(cos, ic, 1)
    print(f"cosine: max |returned - f64| = {np.abs(dc - pair).max():.3e}; {int((~clear).sum())} of {n} queries inside the gap")
    assert np.abs(dc - pair).max() <= KC.BAR and (pair <= kth[:, None] + KC.BAR).all()
    step = np.diff(dc, axis=1)
    assert (step >= 0).all() and (np.diff(ic, axis=1)[step == 0] > 0).all()      # the total order on the returned values
    top = np.argsort(cos_kept, axis=1, kind="stable")[:, :kmax]
    assert all(set(a) == set(b) for a, b, c in zip(ic.tolist(), top.tolist(), clear) if c)
    one_l2 = run16(Q, K, skip_t, kmax, ops.KNN_L2, 0)
    one_cos = run16(Q, K, skip_t, kmax, ops.KNN_COSINE, 0)
    assert one_l2[2] is None and one_cos[0] is None
    assert np.array_equal(one_l2[0].cpu().numpy(), want) and np.array_equal(one_l2[1].cpu().numpy(), want_d)
    assert torch.equal(one_cos[2], first[0]) and torch.equal(one_cos[3].view(torch.int32), first[1].view(torch.int32))


def _random_rows(rng, rows, D):
    x = (rng.standard_normal((rows, D)) * rng.uniform(0.25, 4, size=(rows, 1))).astype(np.float32)
    return BC.round_bf16(x)                                # f32 values that ARE bf16 values


def test_bitwise_invariance_under_splits_query_order_and_batching(monkeypatch):
    """Random bf16 rows, n = 300, M = 2000, D = 128, kmax = 30, a tenth of the keys skipped: indices and distances of both
    metrics are bitwise equal for the split counts 0 (the plan's), 1, 2, 3 and 64, under a permutation of the queries and
    for the queries searched in two parts; predict_grid gives the same predictions in batches of 100 rows as in one."""
    from octic_vits_amd import ops
    from octic_vits_amd import segmentation as S
    rng = np.random.RandomState(5)
    n, M, D, kmax = 300, 2000, 128, 30
    q, k = _random_rows(rng, n, D), _random_rows(rng, M, D)
    skip = torch.from_numpy((rng.rand(M) < 0.1).astype(np.uint8)).to(DEV)
    Q, K = torch.from_numpy(q).to(DEV).to(BF16), torch.from_numpy(k).to(DEV).to(BF16)

    def same(a, b, rows=slice(None)):
        return all(torch.equal(x.view(torch.int32), y.view(torch.int32)[rows]) for x, y in zip(a, b))

    base = run16(Q, K, skip, kmax, ops.KNN_BOTH, 1)
    assert int(base[0].min()) >= 0 and bool(torch.isfinite(base[1]).all()) and bool(torch.isfinite(base[3]).all())
    for splits in (0, 2, 3, 64):
        assert same(run16(Q, K, skip, kmax, ops.KNN_BOTH, splits), base), splits
    perm = torch.from_numpy(rng.permutation(n)).to(DEV)
    assert same(run16(Q[perm].contiguous(), K, skip, kmax, ops.KNN_BOTH, 0), base, perm)
    assert same(run16(Q[:150], K, skip, kmax, ops.KNN_BOTH, 0), base, slice(0, 150))
    assert same(run16(Q[150:], K, skip, kmax, ops.KNN_BOTH, 0), base, slice(150, n))
    labels = torch.from_numpy(KC.LABEL_VALUES[rng.randint(0, 6, size=(M, 16))]).to(DEV)
    clf = S.KNNClassifier(ignore_labels=KC.IGNORE, dtype="bfloat16")
    clf.fit(torch.from_numpy(k).to(DEV), labels)
    assert clf.train_X.dtype == BF16 and clf.key_norms_.dtype == torch.float32
    whole = clf.predict_grid(torch.from_numpy(q).to(DEV), KC.KS, KC.DISTANCES)
    monkeypatch.setattr(S.KNNClassifier, "QUERY_ROWS", 100)
    parts = clf.predict_grid(torch.from_numpy(q).to(DEV), KC.KS, KC.DISTANCES)
    assert all(torch.equal(whole[p], parts[p]) for p in whole)


@pytest.mark.parametrize("D,kmax", [(64, 30), (1280, 10)], ids=lambda v: str(v))
def test_random_rows_against_the_float64_oracle_of_the_rounded_operands(D, kmax):
    """n = 300, M = 2000, a tenth of the keys skipped, 3 splits, both metrics.  Returned indices are distinct and not skipped;
    returned distances are sorted and within the bar of their pair's f64 distance; EVERY listed neighbour's f64 distance is
    within the bar of the true k-th distance.  Bars: seg_knn_cases.BAR (1e-5 on a cosine distance, 1e-5 (|a|^2 + |b|^2) on a
    squared L2 distance)."""
    from octic_vits_amd import ops
    rng = np.random.RandomState(300 + D)
    n, M = 300, 2000
    q, k = _random_rows(rng, n, D), _random_rows(rng, M, D)
    skip = rng.rand(M) < 0.1
    res = run16(torch.from_numpy(q).to(DEV).to(BF16), torch.from_numpy(k).to(DEV).to(BF16),
                torch.from_numpy(skip.astype(np.uint8)).to(DEV), kmax, ops.KNN_BOTH, 3)
    oracle = KC.oracle_distances(q, k)                     # q, k are already the rounded values
    for name, idx, dist in (("L2", res[0], res[1]), ("cosine", res[2], res[3])):
        d, thr = oracle[name]
        bar = thr / 2
        idx, dist = idx.cpu().numpy().astype(np.int64), dist.cpu().numpy().astype(np.float64)
        assert idx.min() >= 0 and idx.max() < M and not skip[idx].any() and all(len(set(r)) == kmax for r in idx.tolist())
        pair, pair_bar = np.take_along_axis(d, idx, 1), np.take_along_axis(bar, idx, 1)
        print(f"D={D} {name}: max |returned - f64 of the pair| / bar = {(np.abs(dist - pair) / pair_bar).max():.3e}")
        assert (np.abs(dist - pair) <= pair_bar).all() and (np.diff(dist, axis=1) >= 0).all()
        kept = np.where(skip[None, :], np.inf, d)
        order = np.argsort(kept, axis=1, kind="stable")
        kth = np.take_along_axis(kept, order[:, kmax - 1:kmax], 1)
        kth_bar = np.take_along_axis(bar, order[:, kmax - 1:kmax], 1)
        excess = (pair - kth) / np.maximum(pair_bar, kth_bar)
        print(f"D={D} {name}: max (f64 distance of a listed neighbour - true k-th) / bar = {excess.max():.3e}")
        assert excess.max() <= 1.0


@pytest.mark.parametrize("D", [64, 1280])
def test_row_norms_of_bf16_rows_against_float64(D):
    """37 rows (the last workgroup has one live wave) with a row stride above D.  Squares of bf16 values are exact in f32 and
    all terms are positive, so the f32 sum is within (number of additions on the longest path) 2^-24 of the exact one,
    relatively: 8 ceil(D / 512) per lane, 6 butterfly steps."""
    from octic_vits_amd import ops
    x = _random_rows(np.random.RandomState(D), 37, D)
    got = ops.seg_rownorms(wide_rows(x, 8, 9.0))
    assert got.dtype == torch.float32 and tuple(got.shape) == (37,)
    want = (x.astype(np.float64) ** 2).sum(1)
    rel = np.abs(got.cpu().numpy().astype(np.float64) - want) / want
    bound = (8 * -(-D // 512) + 6) * 2.0 ** -24
    print(f"D={D}: max relative error {rel.max():.3e}, bound {bound:.3e}")
    assert rel.max() <= bound


def test_zero_rows_and_nan_keys_are_never_listed():
    """A zero key has no cosine distance (0 / 0): never in a cosine list, but at its L2 distance in the L2 list.  A key with
    a NaN is in neither.  A zero query lists nothing under cosine: (+inf, -1) entries."""
    from octic_vits_amd import ops
    rng = np.random.RandomState(11)
    n, M, D, kmax = 40, 300, 64, 8
    q, k = _random_rows(rng, n, D), _random_rows(rng, M, D)
    k[3] = 0.0
    k[130] = 0.0
    k[7, 5] = np.nan
    k[128, 63] = np.nan
    q[0] = 0.0
    q[1:] *= 0.01                                          # small queries: the zero keys are their L2-nearest
    for splits in (1, 3):
        il, dl, ic, dc = [t.cpu().numpy() for t in run16(torch.from_numpy(q).to(DEV).to(BF16), torch.from_numpy(k).to(DEV).to(BF16),
                                                         None, kmax, ops.KNN_BOTH, splits)]
        assert not np.isin(ic, (3, 130, 7, 128)).any() and not np.isin(il, (7, 128)).any()
        assert (il[:, 0] == 3).all() and (il[:, 1] == 130).all()          # equal distances: the lower index first
        assert (il >= 0).all() and np.isfinite(dl).all()
        assert (ic[0] == -1).all() and np.isinf(dc[0]).all() and (ic[1:] >= 0).all() and np.isfinite(dc[1:]).all()


# ------------------------------------------------------------------------------------------------ against the reference
def _golden():
    g = np.load(os.path.join(GOLDEN, "seg_knn_bf16.npz"))
    return g, KC.problem(g)


@pytest.mark.parametrize("sub", KC.SUBSAMPLINGS)
def test_lists_are_valid_topk_answers_of_the_reference_bf16_distances(sub):
    """The golden's problem, keys[::sub], ignored patches skipped.  (1) Every list of ours is a valid top-k of the distances
    the reference computed in bf16: the worst reference distance among our k neighbours exceeds the reference's k-th smallest
    by at most the slack the maker measured for the f64 ordering plus one bf16 step.  (2) On the clear boundaries our
    neighbour set is the reference's.  (3) On the queries whose boundary is clear KNNClassifier(dtype="bfloat16") predicts
    every pixel as the reference did.  Condition (a) of the maker is asserted here, so none of this passes by default."""
    from octic_vits_amd import ops
    from octic_vits_amd import segmentation as S
    g, p = _golden()
    keep = BC.kept(p["key_labels"])[::sub]
    ref = {d: g[f"ref_{d}_sub{sub}"] for d in KC.DISTANCES}
    counts = BC.clear_counts(ref, keep)
    if sub == 1:
        assert BC.condition_a(counts, KC.N_QUERIES)
    assert min(counts.values()) >= BC.MIN_CLEAR_PER_CELL
    Xk, Xq = torch.from_numpy(p["keys"]).to(DEV), torch.from_numpy(p["queries"]).to(DEV)
    skip = torch.from_numpy((~keep).astype(np.uint8)).to(DEV)
    res = run16(Xq.to(BF16), Xk[::sub].to(BF16), skip, KC.KS[-1], ops.KNN_BOTH, 0)
    ours = {"L2": res[0].cpu().numpy().astype(np.int64), "cosine": res[2].cpu().numpy().astype(np.int64)}
    clf = S.KNNClassifier(ignore_labels=KC.IGNORE, train_set_subsampling=sub, dtype="bfloat16")
    clf.fit(Xk, torch.from_numpy(p["key_labels"]).to(DEV))
    assert torch.equal(clf.skip_, skip) and clf.train_X.dtype == BF16
    grid = clf.predict_grid(Xq, KC.KS, KC.DISTANCES)
    for d in KC.DISTANCES:
        slack = BC.slack_steps(ref[d], keep, ours[d])
        print(f"sub {sub} {d}: our lists exceed the reference's k-th distance by {slack} bf16 steps (the f64 ordering: {int(g['slack_' + d])})")
        assert slack <= int(g[f"slack_{d}"]) + 1
        o = BC.ordinal(ref[d])
        for k in KC.KS:
            kth, clear = BC.boundaries(ref[d], keep)[k]
            ref_set = keep[None, :] & (o <= kth[:, None])
            got_set = np.zeros_like(ref_set)
            np.put_along_axis(got_set, ours[d][:, :k], True, 1)
            assert ref_set[clear].sum(1).tolist() == [k] * int(clear.sum())
            assert np.array_equal(got_set[clear], ref_set[clear]), (d, k)
            pred = grid[(k, d)].cpu().numpy()
            assert pred.dtype == np.uint8 and np.array_equal(pred[clear], g[f"pred_sub{sub}"][KC.grid().index((k, d))][clear]), (d, k)
    sel = S.KNNClassifier(ignore_labels=KC.IGNORE, train_set_subsampling=sub, dtype="bfloat16")
    metrics = sel.select_hparams(Xk, torch.from_numpy(p["key_labels"]).to(DEV), Xq, torch.from_numpy(p["query_labels"]).to(DEV))
    assert list(metrics) == list(g[f"select_names_sub{sub}"]) and all(0.0 <= v <= 1.0 for v in metrics.values())


def test_bfloat16_classifier_equals_the_float32_classifier_on_bf16_representable_features():
    """Integers in [-8, 8] are bf16 values and every dot and norm is exact in f32 on both paths, so fit / predict at every grid
    point and select_hparams give identical results at both dtypes."""
    from octic_vits_amd import segmentation as S
    rng = np.random.RandomState(23)
    n, M, D, L = 200, 500, 64, 16
    Xk = torch.from_numpy(rng.randint(-8, 9, size=(M, D)).astype(np.float32)).to(DEV)
    Xq = torch.from_numpy(rng.randint(-8, 9, size=(n, D)).astype(np.float32)).to(DEV)
    values = np.concatenate([KC.LABEL_VALUES, np.asarray([0, 255], dtype=np.uint8)])
    Lk = torch.from_numpy(values[rng.randint(0, 8, size=(M, 1))].repeat(L, 1)).to(DEV)
    Lk[torch.from_numpy(rng.rand(M, L) < 0.2).to(DEV)] = 7
    Lq = torch.from_numpy(KC.LABEL_VALUES[rng.randint(0, 6, size=(n, L))]).to(DEV)
    a = S.KNNClassifier(ignore_labels=KC.IGNORE, dtype="float32", train_set_subsampling=3)
    b = S.KNNClassifier(ignore_labels=KC.IGNORE, dtype="bfloat16", train_set_subsampling=3)
    a.fit(Xk, Lk)
    b.fit(Xk, Lk)
    assert a.train_X.dtype == torch.float32 and b.train_X.dtype == BF16 and int(b.skip_.sum()) > 0
    assert torch.equal(a.key_norms_, b.key_norms_) and torch.equal(a.skip_, b.skip_)
    for k, d in KC.grid():
        a.num_neighbors = b.num_neighbors = k
        a.distance = b.distance = d
        assert torch.equal(a.predict(Xq), b.predict(Xq)), (k, d)
    ma, mb = (S.KNNClassifier(ignore_labels=KC.IGNORE, dtype=t).select_hparams(Xk, Lk, Xq, Lq) for t in ("float32", "bfloat16"))
    assert ma == mb and len(ma) == 8


def test_eval_features_runs_the_reference_configuration():
    """eval_features with the reference's ``classifiers_kwargs: {knn: {dtype: bfloat16}}`` returns the key names of the
    reference's eval_model(classifiers=("knn",)) (recorded in tests/golden/seg_knn.npz), in its order."""
    from octic_vits_amd import segmentation as S
    g, p = _golden()
    names = np.load(os.path.join(GOLDEN, "seg_knn.npz"))["eval_model_keys"]
    feats = S.SegSplits(torch.from_numpy(p["keys"]).to(DEV), torch.from_numpy(p["key_labels"]).to(DEV),
                        torch.from_numpy(p["queries"]).to(DEV), torch.from_numpy(p["query_labels"]).to(DEV), KC.N_VAL, 1)
    res = S.eval_features(feats, classifiers=("knn",), ignore_labels=KC.IGNORE, classifiers_kwargs={"knn": {"dtype": "bfloat16"}})
    assert sorted(res) == list(names)
    assert list(res)[:8] == ["hparam_fitting.knn." + s for s in g["select_names_sub1"]]
    assert list(res)[8:] == ["labels_knn_mIoU", "labels_knn_acc"]
    assert all(isinstance(v, float) and 0.0 <= v <= 1.0 for v in res.values())
    assert feats.X.dtype == torch.float32                  # the caller's matrix is neither cast in place nor kept
