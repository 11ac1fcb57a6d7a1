"""csrc/knn_cls.hip and octic_vits_amd.knn on the GPU.

Exact tests: features are integers in {-2 .. 2}, so every inner product is exact in f32 in any summation order and the expected
neighbours are ``np.lexsort((index, -similarity))`` in int64 - compared with ``==``.  Integer data is full of exact ties, which
is what checks the (similarity, index) rule across tile and split boundaries.
Real-valued tests: a float64 numpy oracle.  A similarity stays within D 2^-24 |q| |k| of the exact inner product (the worst case
of one f32 fmaf chain); probas stay within 1e-5 of the float64 formula on the same lists (the weights sum to 1, the exponent's
argument is at most 2 / 0.07 = 29 in magnitude so each weight carries a relative error of a few 1e-6, and the <= 200-term
rank-order sums add <= 200 2^-24).  No test here reads the reference; tests/golden/knn_cls.npz holds what the reference's own
KnnModule computed on the CPU (tests/golden/make_knn_cls_golden.py)."""
import os

import numpy as np
import pytest
import torch

import knn_cls_cases as KC

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IDX_GUARD, SIM_GUARD, GUARD_COLS = -7, -7.0, 3
PROBA_TOL = 1e-5


def run_topk(Q, K, kmax, splits):
    """knn_topk into sentinel-filled outputs GUARD_COLS wider than kmax; asserts the guard columns AND that every listed column
    was written, returns (idx, sim) [n, kmax]."""
    from octic_vits_amd import ops
    n = Q.shape[0]
    idx = torch.full((n, kmax + GUARD_COLS), IDX_GUARD, dtype=torch.int32, device=DEV)
    sim = torch.full((n, kmax + GUARD_COLS), SIM_GUARD, dtype=torch.float32, device=DEV)
    ops.knn_topk(Q, K, kmax, splits, out=(idx, sim))
    assert bool((idx[:, kmax:] == IDX_GUARD).all()) and bool((sim[:, kmax:] == SIM_GUARD).all()), "a guard column was written"
    assert bool((idx[:, :kmax] != IDX_GUARD).all()), "a listed column was not written"
    return idx[:, :kmax].contiguous(), sim[:, :kmax].contiguous()


def integer_case(n, M, seed, D=64):
    """Integer rows in {-2 .. 2}; Q is a view with ldq = D + 4, K every other row of a buffer (ldk = 2 D); blocks of one
    duplicated key row lie across the tile boundary at 128 and across the split boundaries of 2 and 5 splits of 1000 keys."""
    rng = np.random.RandomState(seed)
    q = rng.randint(-2, 3, size=(n, D)).astype(np.int64)
    k = rng.randint(-2, 3, size=(M, D)).astype(np.int64)
    for lo, hi in ((120, 136), (250, 262), (380, 389), (505, 520), (760, 775)):
        k[lo:min(hi, M)] = k[min(120, M - 1)]
    qbuf = torch.full((n, D + 4), 9.0, device=DEV)
    qbuf[:, :D] = torch.from_numpy(q.astype(np.float32)).to(DEV)
    kbuf = torch.full((2 * M, D), 9.0, device=DEV)
    kbuf[::2] = torch.from_numpy(k.astype(np.float32)).to(DEV)
    return q, k, qbuf[:, :D], kbuf[::2]


@pytest.mark.parametrize("M", [200, 389, 1000])
@pytest.mark.parametrize("n", [1, 67, 130])
def test_exact_neighbours_on_integer_features(n, M):
    """idx AND sim equal the int64 oracle for every kmax at the wave-width edges of the multi-pass insert and every split count;
    M = 200 with kmax = 200 is M == kmax."""
    q, k, Q, K = integer_case(n, M, 1000 + n + M)
    assert Q.stride(0) == 68 and K.stride(0) == 128
    s = q @ k.T
    order = np.stack([np.lexsort((np.arange(M), -row)) for row in s])
    for kmax in (1, 10, 63, 64, 65, 200):
        want = order[:, :kmax]
        want_s = np.take_along_axis(s, want, 1).astype(np.float32)
        for splits in (0, 1, 2, 5):
            idx, sim = run_topk(Q, K, kmax, splits)
            assert np.array_equal(idx.cpu().numpy(), want), f"kmax={kmax} splits={splits}"
            assert np.array_equal(sim.cpu().numpy(), want_s), f"kmax={kmax} splits={splits}"


def test_short_lists_end_on_minus_infinity_and_minus_one():
    """NaN similarities count as -inf and a key at -inf is never listed: with all but 3 key rows NaN, every list holds those 3
    in order and ends on (-inf, -1); a key row of -inf entries is not listed either."""
    rng = np.random.RandomState(5)
    q = rng.randint(1, 3, size=(70, 64)).astype(np.float32)
    k = np.full((300, 64), np.nan, dtype=np.float32)
    live = [7, 130, 299]
    k[live] = rng.randint(-2, 3, size=(3, 64))
    k[200] = -np.inf                                          # q > 0: the inner product is -inf
    for splits in (1, 2):
        idx, sim = run_topk(torch.from_numpy(q).to(DEV), torch.from_numpy(k).to(DEV), 10, splits)
        s = q.astype(np.int64) @ k[live].astype(np.int64).T
        order = np.stack([np.lexsort((np.arange(3), -row)) for row in s])
        assert np.array_equal(idx[:, :3].cpu().numpy(), np.asarray(live)[order])
        assert np.array_equal(sim[:, :3].cpu().numpy(), np.take_along_axis(s, order, 1).astype(np.float32))
        assert bool((idx[:, 3:] == -1).all()) and bool(torch.isneginf(sim[:, 3:]).all())


def test_results_are_bitwise_equal_across_splits_query_order_and_batching():
    rng = np.random.RandomState(11)
    n, M, D, kmax = 130, 1000, 128, 200
    Q = torch.from_numpy(rng.standard_normal((n, D)).astype(np.float32)).to(DEV)
    K = torch.from_numpy(rng.standard_normal((M, D)).astype(np.float32)).to(DEV)
    idx0, sim0 = run_topk(Q, K, kmax, 0)
    for splits in (1, 3):
        idx, sim = run_topk(Q, K, kmax, splits)
        assert torch.equal(idx, idx0) and torch.equal(sim.view(torch.int32), sim0.view(torch.int32)), splits
    perm = torch.from_numpy(rng.permutation(n)).to(DEV)
    idx, sim = run_topk(Q[perm].contiguous(), K, kmax, 0)
    assert torch.equal(idx, idx0[perm]) and torch.equal(sim.view(torch.int32), sim0[perm].view(torch.int32))
    for bs in (1, 7, 64):
        parts = [run_topk(Q[i:i + bs], K, kmax, 0) for i in range(0, n, bs)]
        idx, sim = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
        assert torch.equal(idx, idx0) and torch.equal(sim.view(torch.int32), sim0.view(torch.int32)), bs


def _golden():
    g = np.load(os.path.join(GOLDEN, "knn_cls.npz"))
    return g, KC.problem(g)


def _oracle_case(name):
    if name == "golden":
        p = _golden()[1]
        return p["queries"], p["keys"]
    rng = np.random.RandomState(1280)
    q, k = rng.standard_normal((64, 1280)), rng.standard_normal((512, 1280))
    return ((q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32),
            (k / np.linalg.norm(k, axis=1, keepdims=True)).astype(np.float32))


@pytest.mark.parametrize("name", ["golden", "D1280"])
def test_similarities_and_neighbour_sets_against_a_float64_oracle(name):
    """kmax = 200 with 2 splits.  Every returned similarity is within D 2^-24 |q| |k| of its pair's exact inner product, the lists
    are sorted and hold distinct keys, and the neighbour SET equals the oracle's wherever the boundary gap s[199] - s[200] exceeds
    twice that bound (every query of the golden problem: the maker's seed search saw to it)."""
    q, k = _oracle_case(name)
    n, D = q.shape
    M, kmax = k.shape[0], 200
    idx, sim = run_topk(torch.from_numpy(q).to(DEV), torch.from_numpy(k).to(DEV), kmax, 2)
    idx, sim = idx.cpu().numpy().astype(np.int64), sim.cpu().numpy().astype(np.float64)
    q64, k64 = q.astype(np.float64), k.astype(np.float64)
    exact = q64 @ k64.T
    bound = D * 2.0 ** -24 * np.linalg.norm(q64, axis=1)[:, None] * np.linalg.norm(k64, axis=1)[None, :]
    assert idx.min() >= 0 and idx.max() < M and all(len(set(r)) == kmax for r in idx.tolist())
    err = np.abs(sim - np.take_along_axis(exact, idx, 1)) / np.take_along_axis(bound, idx, 1)
    print(f"{name}: max |sim - exact| / bound = {err.max():.3e}")
    assert err.max() <= 1.0 and np.all(np.diff(sim, axis=1) <= 0)
    order = np.argsort(-exact, axis=1, kind="stable")
    gap = np.take_along_axis(exact, order[:, kmax - 1:kmax], 1)[:, 0] - np.take_along_axis(exact, order[:, kmax:kmax + 1], 1)[:, 0]
    edge = np.maximum(np.take_along_axis(bound, order[:, kmax - 1:kmax], 1), np.take_along_axis(bound, order[:, kmax:kmax + 1], 1))[:, 0]
    clear = gap > 2 * edge
    print(f"{name}: {int(clear.sum())} of {n} queries have a clear boundary")
    same = np.asarray([set(a) == set(b) for a, b in zip(idx.tolist(), order[:, :kmax].tolist())])
    assert same[clear].all()
    if name == "golden":
        assert clear.all()
    else:
        assert clear.sum() >= 5                                    # the check above is not vacuous
    # the sorted exact similarities of the returned keys match the oracle's 200 largest within the bound
    got = -np.sort(-np.take_along_axis(exact, idx, 1), axis=1)
    assert np.all(np.abs(got - np.take_along_axis(exact, order[:, :kmax], 1)) <= 2 * bound.max())


def _lists_for_vote(C, seed):
    """The kernel's own lists on the golden problem (kmax = 200), with rows 0 .. 2 cut short to (-inf, -1) tails, and labels in
    [0, C) of which three keys carry labels outside it."""
    p = _golden()[1]
    idx, sim = run_topk(torch.from_numpy(p["queries"]).to(DEV), torch.from_numpy(p["keys"]).to(DEV), 200, 0)
    for row, keep in ((0, 150), (1, 1), (2, 10)):
        idx[row, keep:] = -1
        sim[row, keep:] = float("-inf")
    rng = np.random.RandomState(seed)
    labels = p["key_labels"].copy() if C == KC.N_CLASSES else rng.randint(0, C, size=KC.N_KEYS)
    nearest = idx[5:7, 0].cpu().numpy()
    assert nearest[0] != nearest[1]
    labels[nearest[0]], labels[nearest[1]] = C + 100, -1                # the nearest neighbour of rows 5 and 6
    return idx, sim, labels.astype(np.int64)


@pytest.mark.parametrize("ks", [(200,), (10, 20, 100, 200), (1, 2, 5, 10, 20, 64, 100, 200)], ids=lambda k: f"nk{len(k)}")
@pytest.mark.parametrize("C", [16, 1000])
def test_vote_against_the_float64_formula(C, ks):
    from octic_vits_amd import ops
    idx, sim, labels = _lists_for_vote(C, 3)
    n = idx.shape[0]
    out = torch.full((len(ks), n, C), float("nan"), device=DEV)
    got = ops.knn_vote(sim, idx, torch.from_numpy(labels).to(DEV), C, 1 / KC.T, ks, out=out)
    assert got is out and not bool(torch.isnan(out).any()), "an element of probas was not written"
    want = KC.oracle_probas(sim.cpu().numpy(), idx.cpu().numpy(), labels, C, 1 / KC.T, ks)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
    print(f"C={C} ks={ks}: max |proba - f64| = {err:.3e}")
    assert err <= PROBA_TOL
    sums = got.sum(2).cpu().numpy()
    assert np.all(sums <= 1 + 1e-5)
    bad_keys = np.nonzero((labels < 0) | (labels >= C))[0]
    whole = ~np.isin(idx.cpu().numpy(), bad_keys).any(1)                # rows none of whose neighbours has a label outside [0, C)
    assert len(bad_keys) == 2 and whole.sum() >= 4 and not whole[5] and not whole[6]
    assert np.abs(sums[-1, whole] - 1).max() <= 1e-5                    # k = kmax: the whole softmax (cut rows included)
    if len(ks) > 1:
        assert sums[0, 8:].max() < 0.999                                # a prefix of the softmax over all 200 does not sum to 1
    assert sums[-1, 5] < 0.999 and sums[-1, 6] < 0.999                  # a label outside [0, C) casts no vote
    # a strided pair of lists gives the same bits
    wide_i = torch.full((n, 208), -3, dtype=torch.int32, device=DEV)
    wide_s = torch.full((n, 208), 5.0, device=DEV)
    wide_i[:, :200], wide_s[:, :200] = idx, sim
    again = ops.knn_vote(wide_s[:, :200], wide_i[:, :200], torch.from_numpy(labels).to(DEV), C, 1 / KC.T, ks)
    assert torch.equal(again.view(torch.int32), got.view(torch.int32))


def test_counters_follow_the_proba_then_class_index_rule_and_accumulate():
    from octic_vits_amd import ops
    ks = (10, 20, 100, 200)
    for C in (16, 1000):
        idx, sim, labels = _lists_for_vote(C, 4)
        n = idx.shape[0]
        rng = np.random.RandomState(C)
        targets = rng.randint(0, C, size=n) if C == 1000 else _golden()[1]["query_labels"].copy()
        if C == 1000:                                                    # a random target of 1000 never hits: take a neighbour's class
            near_idx = idx.cpu().numpy()[np.arange(n), np.arange(n) % 12]
            targets[8::2] = labels[near_idx[8::2]]
        targets[3], targets[4] = -1, C                                   # outside [0, C): no hit
        lab_t, tgt_t = torch.from_numpy(labels).to(DEV), torch.from_numpy(targets.astype(np.int64)).to(DEV)
        counters = torch.zeros(len(ks), 2, dtype=torch.int64, device=DEV)
        probas = ops.knn_vote(sim, idx, lab_t, C, 1 / KC.T, ks, targets=tgt_t, counters=counters)
        assert torch.equal(probas, ops.knn_vote(sim, idx, lab_t, C, 1 / KC.T, ks))
        want64 = KC.oracle_probas(sim.cpu().numpy(), idx.cpu().numpy(), labels, C, 1 / KC.T, ks)
        p32 = probas.cpu().numpy()
        ok = (targets >= 0) & (targets < C)
        for i, k in enumerate(ks):
            rank32 = KC.rank_of_target(p32[i], targets)
            assert counters[i].tolist() == [int((rank32 < 1).sum()), int((rank32 < 5).sum())], (C, k)
            # ... and the float64 oracle agrees wherever its decision does not hang on probas within 2e-5 of each other
            # (exact ties - the zero-vote classes - are decided by the class index in both)
            rank64 = KC.rank_of_target(want64[i], targets)
            pt = want64[i][np.arange(n), np.clip(targets, 0, C - 1)][:, None]
            near = ((np.abs(want64[i] - pt) <= KC.PROBA_BAR) & (want64[i] != pt)).any(1)
            clear = ok & ~near
            assert clear.sum() >= n // 2
            for top in (1, 5):
                assert np.array_equal((rank32 < top)[clear], (rank64 < top)[clear]), (C, k, top)
        ops.knn_vote(sim, idx, lab_t, C, 1 / KC.T, ks, targets=tgt_t, counters=counters)
        for i in range(len(ks)):
            rank32 = KC.rank_of_target(p32[i], targets)
            assert counters[i].tolist() == [2 * int((rank32 < 1).sum()), 2 * int((rank32 < 5).sum())]


def test_counters_on_the_crafted_tie():
    """All neighbours share class 7 of 16: class 7 leads and the zero-vote classes 0, 1, 2, 3 fill the top 5 by the index rule.  A
    target among 0 .. 3 hits top-5, one above misses; 7 hits top-1; targets outside [0, C) count nothing."""
    from octic_vits_amd import ops
    targets = [7, 0, 3, 4, 15, 1, 2, -1, 16, 6]
    n, kmax, ks = len(targets), 20, (1, 20)
    sim = torch.linspace(0.9, 0.1, kmax, device=DEV).repeat(n, 1).contiguous()
    idx = torch.arange(kmax, dtype=torch.int32, device=DEV).repeat(n, 1).contiguous()
    labels = torch.full((50,), 7, dtype=torch.int64, device=DEV)
    counters = torch.zeros(2, 2, dtype=torch.int64, device=DEV)
    probas = ops.knn_vote(sim, idx, labels, 16, 1 / KC.T, ks, targets=torch.tensor(targets, device=DEV), counters=counters)
    assert bool((probas[:, :, :7] == 0).all()) and bool((probas[:, :, 8:] == 0).all()) and abs(float(probas[1, 0, 7]) - 1) <= 1e-6
    assert counters.tolist() == [[1, 5], [1, 5]]                        # top-1: the 7; top-5: 7, 0, 3, 1, 2
    ops.knn_vote(sim, idx, labels, 16, 1 / KC.T, ks, targets=torch.tensor(targets, device=DEV), counters=counters)
    assert counters.tolist() == [[2, 10], [2, 10]]


# ------------------------------------------------------------------------------------------------ against the reference
def _flags(probas, targets, top):
    return KC.rank_of_target(probas, targets) < top


def test_module_and_evaluation_equal_the_reference_golden():
    """KnnModule.forward against the reference's KnnModule (CPU, float32 torch) on the clustered problem of the golden: probas
    within 1e-5 plus the reference's own recorded f32-vs-f64 spread, top-1 flags equal at every (query, k), top-5 flags equal at
    every unambiguous one, accuracies over the unambiguous cases equal; the same for both few-shot tries; eval_knn_features
    returns the reference's keys, its top-1 accuracies, and top-5 accuracies that equal the (proba, class index) rule on our
    own probas."""
    from octic_vits_amd import knn as KN
    g, p = _golden()
    Xk, Xq = torch.from_numpy(p["keys"]).to(DEV), torch.from_numpy(p["queries"]).to(DEV)
    yk, yq = torch.from_numpy(p["key_labels"]).to(DEV), torch.from_numpy(p["query_labels"]).to(DEV)
    tol = PROBA_TOL + float(g["ref_f32_f64_spread"])
    nb_knn = list(KC.NB_KNN)

    def compare(module, prefix, ks):
        out = module(Xq)
        assert list(out) == ks
        ours5 = []
        for i, k in enumerate(ks):
            pr = out[k].cpu().numpy()
            assert tuple(pr.shape) == (KC.N_QUERIES, KC.N_CLASSES)
            err = np.abs(pr.astype(np.float64) - g[f"{prefix}_probas"][i]).max()
            print(f"{prefix} k={k}: max |proba - reference| = {err:.3e} (tolerance {tol:.3e})")
            assert err <= tol
            assert np.array_equal(_flags(pr, p["query_labels"], 1), g[f"{prefix}_top1"][i]), (prefix, k)
            clear = ~g[f"{prefix}_ambiguous5"][i]
            f5 = _flags(pr, p["query_labels"], 5)
            assert np.array_equal(f5[clear], g[f"{prefix}_top5"][i][clear]), (prefix, k)
            assert f5[clear].mean() == g[f"{prefix}_top5"][i][clear].mean()
            ours5.append(f5.mean())
        return ours5

    full = KN.KnnModule(Xk, yk, nb_knn, KC.T, num_classes=KC.N_CLASSES)
    assert (full.nb_knn, full.max_k, full.T, full.num_classes) == (nb_knn, 200, KC.T, KC.N_CLASSES)
    sims, nl = full.compute_neighbors(Xq)
    assert tuple(sims.shape) == (KC.N_QUERIES, 200) and nl.dtype == torch.int64
    nl, ref_nl = nl.cpu().numpy(), g["full_neighbor_labels"]
    for lo, hi in zip([0] + nb_knn[:-1], nb_knn):          # the boundary gaps are clear at this seed: the same neighbours between them
        assert np.array_equal(np.sort(nl[:, lo:hi], 1), np.sort(ref_nl[:, lo:hi], 1)), (lo, hi)
    top5 = {("full", k): v for k, v in zip(nb_knn, compare(full, "full", nb_knn))}
    md = KN.create_module_dict(module=lambda **kw: KN.KnnModule(T=KC.T, num_classes=KC.N_CLASSES, **kw),
                               n_per_class_list=[KC.FEWSHOT_NPC], n_tries=KC.FEWSHOT_TRIES, nb_knn=nb_knn, train_features=Xk,
                               train_labels=yk)
    fk = g["fewshot_k_list"].tolist()
    few5 = [compare(md["5 per class"][str(t)], f"fewshot{t}", fk) for t in range(KC.FEWSHOT_TRIES)]
    for j, k in enumerate(fk):
        top5[("5 per class", k)] = sum(f[j] for f in few5) / KC.FEWSHOT_TRIES

    batches = [(Xq[i:i + 24], yq[i:i + 24]) for i in range(0, KC.N_QUERIES, 24)]            # 24, 24, 16: batches may differ
    res = KN.eval_knn_features(Xk, yk, iter(batches), nb_knn=KC.NB_KNN, temperature=KC.T, n_per_class_list=[-1, KC.FEWSHOT_NPC],
                               n_tries=KC.FEWSHOT_TRIES)
    assert [repr(k) for k in res] == list(g["result_keys"])
    assert list(KN.results_lines(res)) == list(g["result_line_keys"])
    for i, k in enumerate(nb_knn):
        assert res[("full", k)]["top-1"] == float(g["full_acc1"][i])
    for i, k in enumerate(fk):
        assert res[("5 per class", k)]["top-1"] == float(g["fewshot_acc1"][i])
    for key, v in res.items():
        assert set(v) == {"top-1", "top-5"} and v["top-5"] == top5[key], key
    for i, k in enumerate(nb_knn[2:], 2):                               # no ambiguous case at k = 100, 200: the reference's top-5
        assert res[("full", k)]["top-5"] == float(g["full_acc5"][i])


def test_eval_knn_end_to_end_on_a_tiny_backbone():
    """eval_knn on the tiny hybrid DINOv2 model of test_seg_knn_gpu.py: its result equals eval_knn_features on extract_features'
    rows, those rows equal F.normalize(model(x).float()) to 1e-6, and the dictionary has the reference's keys."""
    from octic_vits_amd import dinov2_models
    from octic_vits_amd import knn as KN
    torch.manual_seed(4)
    model = dinov2_models._dinov2(4, 256, 10, 4, False, 2, dict(img_size=32)).to(DEV).eval()
    g = torch.Generator().manual_seed(22)

    def batches(n_img, bs, first):
        return [(torch.randn(min(bs, n_img - i), 3, 32, 32, generator=g), (torch.arange(i, min(i + bs, n_img)) + first) % 6)
                for i in range(0, n_img, bs)]

    train, val = batches(40, 16, 0), batches(12, 8, 1)
    kw = dict(nb_knn=(3, 10), temperature=0.07, n_per_class_list=(-1, 4), n_tries=2)
    res = KN.eval_knn(model, train, val, **kw)
    assert list(res) == [("full", 3), ("full", 10), ("4 per class", 3), ("4 per class", 4)]
    assert all(set(v) == {"top-1", "top-5"} and 0.0 <= v["top-1"] <= v["top-5"] <= 1.0 for v in res.values())
    X, y = KN.extract_features(model, train)
    assert X.is_cuda and X.dtype == torch.float32 and tuple(X.shape) == (40, 256) and y.dtype == torch.int64
    assert torch.equal(y.cpu(), torch.arange(40) % 6)
    with torch.no_grad():
        want = torch.cat([torch.nn.functional.normalize(model(x.to(DEV)).float(), dim=1, p=2) for x, _ in train])
    assert float((X - want).abs().max()) <= 1e-6
    assert float((X.norm(dim=1) - 1).abs().max()) <= 1e-5
    again = KN.eval_knn_features(X, y, [KN.extract_features(model, [b]) for b in val], **kw)
    assert again == res
