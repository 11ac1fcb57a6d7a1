"""csrc/topk_metric.hip and octic_vits_amd.metrics on the GPU.

torchmetrics is not a dependency, so the oracle lives here, in two forms; every comparison is integer equality of ranks and
counters, and ratios are compared as the same float64 quotient of those integers.

(a) ``oracle_ranks``: explicit comparisons on the CPU (float64 copies of the f32 scores, NaN replaced by -inf, counts in int64)
    for both tie orders; ``oracle_any`` / ``oracle_class`` count rows from those ranks.
(b) ``restated_*``: what ``ImageNetReaLAccuracy.update`` and ``MulticlassAccuracy(average=micro|macro|none, top_k=k)`` compute,
    restated with ``torch.topk`` and one-hot products.  ``topk`` leaves ties open, so (b) is used only on rows whose scores are
    pairwise distinct (a scaled permutation of ``arange(C)`` per row), where it is determined and must agree exactly."""
import pytest
import torch

from octic_vits_amd import metrics
from octic_vits_amd.metrics import MetricType, TopkAccuracy

pytestmark = pytest.mark.gpu
DEV = "cuda"
KS = (1, 5)


# ------------------------------------------------------------------------------------------------ oracle (a)
def oracle_ranks(scores, targets, order, mapping=None):
    """int64 [G, n, A] from CPU tensors: scores [G, n, C], targets [n, A]."""
    s = scores.double()
    s = torch.where(torch.isnan(s), torch.full_like(s, float("-inf")), s)
    if mapping is not None:
        s = s[..., torch.as_tensor(mapping).long()]
    G, n, Cm = s.shape
    A = targets.shape[1]
    j = torch.arange(Cm)
    out = torch.full((G, n, A), Cm, dtype=torch.int64)
    for a in range(A):
        t = targets[:, a]
        ok = (t >= 0) & (t < Cm)
        tc = torch.where(ok, t, torch.zeros_like(t))
        st = s.gather(2, tc.view(1, n, 1).expand(G, n, 1))                      # [G, n, 1]
        before = s > st
        if order == 1:
            before = before | ((s == st) & (j.view(1, 1, Cm) < tc.view(1, n, 1)))
        out[:, :, a] = torch.where(ok.view(1, n), before.sum(-1), torch.full((G, n), Cm, dtype=torch.int64))
    return out


def oracle_any(ranks, Cm, ks=KS):
    """int64 [G, 1 + nk]: rows with a defined target, rows where some defined target has rank < k."""
    best = ranks.min(-1).values
    cols = [(best < Cm).sum(-1)] + [((best < Cm) & (best < k)).sum(-1) for k in ks]
    return torch.stack(cols, -1)


def oracle_class(ranks, targets, Cm, ks=KS):
    """int64 [G, Cm, 1 + nk] from ranks [G, n, 1] and targets [n, 1]."""
    G = ranks.shape[0]
    out = torch.zeros(G, Cm, 1 + len(ks), dtype=torch.int64)
    t = targets[:, 0]
    for r in range(t.shape[0]):
        if 0 <= int(t[r]) < Cm:
            out[:, int(t[r]), 0] += 1
            for i, k in enumerate(ks):
                out[:, int(t[r]), 1 + i] += (ranks[:, r, 0] < k).long()
    return out


# ------------------------------------------------------------------------------------------------ oracle (b)
def topk_onehot(preds, k):
    return torch.zeros(preds.shape, dtype=torch.int64).scatter_(1, preds.topk(k, dim=1).indices, 1)


def restated_multiclass(preds, target, k, num_classes):
    """(tp per class, support per class) of MulticlassAccuracy(top_k=k) on preds [n, C], target [n]."""
    hit = topk_onehot(preds, k).gather(1, target.view(-1, 1))[:, 0]
    tp = torch.zeros(num_classes, dtype=torch.int64).index_add_(0, target, hit)
    support = torch.bincount(target, minlength=num_classes)
    return tp, support


def restated_real(preds, target, k):
    """(matching rows, rows with a target) of ImageNetReaLAccuracy on preds [n, C], target [n, A] padded with -1."""
    C = preds.shape[1]
    target_oh = torch.zeros(preds.shape[0], C + 1, dtype=torch.int64)
    target_oh.scatter_(1, torch.where(target == -1, torch.full_like(target, C), target), 1)
    target_oh = target_oh[:, :C]
    match = ((topk_onehot(preds, k) * target_oh).sum(1) > 0)
    defined = target_oh.sum(1) > 0
    return int((match & defined).sum()), int(defined.sum())


# ------------------------------------------------------------------------------------------------ inputs
def tied_scores(G, n, C, seed, special=True):
    """CPU f32 [G, n, C] of integers from a range of 4 (ties everywhere) with +-inf and NaN entries."""
    g = torch.Generator().manual_seed(seed)
    s = torch.randint(-1, 3, (G, n, C), generator=g).float()
    if special:
        u = torch.rand(G, n, C, generator=g)
        s[u < 0.02] = float("inf")
        s[(u >= 0.02) & (u < 0.04)] = float("-inf")
        s[(u >= 0.04) & (u < 0.07)] = float("nan")
    return s


def distinct_scores(G, n, C, seed):
    """CPU f32 [G, n, C]: every row a scaled permutation of arange(C) (pairwise distinct, exact in f32)."""
    g = torch.Generator().manual_seed(seed)
    return torch.argsort(torch.rand(G, n, C, generator=g), dim=-1).float() * 0.25 - 3.0


def some_targets(n, A, Cm, seed):
    """CPU int64 [n, A]: classes, -1 padding, out-of-range values, duplicates within a row, rows that are all -1."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, Cm, (n, A), generator=g)
    if A > 1:
        pad = torch.rand(n, A, generator=g) < 0.3
        t[pad] = -1
        t[::5, 1] = t[::5, 0]                       # duplicated targets
    t[3::7] = -1                                    # rows without a target
    if n > 4:
        t[4, 0] = Cm                                # just past the classes: undefined
    if n > 9:
        t[9, 0] = 2 ** 40                           # far outside: undefined
    return t


def strided(scores_cpu, pad_r=2, pad_c=3):
    """The scores on the device as a view of a larger buffer: ld_r = C + pad_c (rows at every 4-byte alignment), ld_g =
    (n + pad_r) ld_r; the padding is NaN-free garbage that must not be read into a rank."""
    G, n, C = scores_cpu.shape
    buf = torch.full((G, n + pad_r, C + pad_c), 1.0e30, device=DEV)
    buf[:, :n, :C] = scores_cpu.to(DEV)
    return buf[:, :n, :C]


def run_rank(scores_dev, targets_cpu, order, mapping=None):
    from octic_vits_amd import ops
    G, n, _ = scores_dev.shape
    A = targets_cpu.shape[1]
    out = torch.full((G * n * A + 8,), -7, dtype=torch.int32, device=DEV)
    cmap = None if mapping is None else torch.as_tensor(mapping, dtype=torch.int32).to(DEV)
    rank = ops.topk_rank(scores_dev, targets_cpu.to(DEV), class_map=cmap, order=order, out=out[:G * n * A].view(G, n, A))
    assert bool((out[G * n * A:] == -7).all()), "rank wrote past its [G, n, A]"
    return rank


def check_case(G, n, C, A, seed, stride=True, mapping=None):
    """Ranks under both orders, the 'any' counters and (A == 1) the per-class counters against oracle (a)."""
    from octic_vits_amd import ops
    Cm = C if mapping is None else len(mapping)
    s = tied_scores(G, n, C, seed)
    t = some_targets(n, A, Cm, seed + 1)
    # a NaN, a +inf and a -inf at a target's own score
    for r, v in ((0, float("nan")), (1, float("inf")), (2, float("-inf"))):
        if r < n and 0 <= int(t[r, 0]) < Cm:
            s[:, r, int(t[r, 0]) if mapping is None else int(mapping[int(t[r, 0])])] = v
    sd = strided(s) if stride else s.to(DEV)
    for order in (0, 1):
        want = oracle_ranks(s, t, order, mapping)
        rank = run_rank(sd, t, order, mapping)
        assert torch.equal(rank.cpu().long(), want), f"ranks differ (order {order})"
        counters = torch.zeros(G, 1 + len(KS), dtype=torch.int64, device=DEV)
        ops.topk_count(rank, counters, KS, mode=ops.TOPK_ANY, num_classes=Cm)
        assert torch.equal(counters.cpu(), oracle_any(want, Cm))
        if A == 1:
            counters = torch.zeros(G, Cm, 1 + len(KS), dtype=torch.int64, device=DEV)
            ops.topk_count(rank, counters, KS, mode=ops.TOPK_CLASS, num_classes=Cm, targets=t.to(DEV).view(n))
            assert torch.equal(counters.cpu(), oracle_class(want, t, Cm))


# ------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("stride", [False, True])
@pytest.mark.parametrize("C", [5, 63, 64, 65, 255, 256, 257, 1000])
def test_ranks_and_counters_at_every_class_count(C, stride):
    """C below, at and above the 64 lanes and the 256-column round of the 16-byte path; contiguous (aligned rows where C % 4 ==
    0) and strided (ld_r = C + 3: rows at every alignment, so the 16-byte and the 4-byte path both run in one launch)."""
    check_case(3, 65, C, 2, 100 + C, stride=stride)
    check_case(3, 65, C, 1, 200 + C, stride=stride)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_ranks_and_counters_at_every_row_count(n):
    check_case(3, n, 257, 1, 300 + n)
    check_case(1, n, 64, 2, 400 + n, stride=False)


@pytest.mark.parametrize("G", [1, 3, 48])
def test_ranks_and_counters_at_every_group_count(G):
    check_case(G, 65, 65, 1, 500 + G)
    check_case(G, 65, 1000, 2, 550 + G, stride=False)


@pytest.mark.parametrize("A", [1, 2, 4, 5, 11, 16, 17, 32])
def test_ranks_and_counters_at_every_target_count(A):
    """A = 1, 2, 11, 32 and both sides of the register-array sizes 4 and 16 the kernel is instantiated for."""
    check_case(3, 63, 257, A, 600 + A)


def test_group_stride_past_2_to_31_elements():
    """Two groups 2^31 elements apart: the row offsets are 64-bit."""
    n, C = 5, 64
    s = tied_scores(2, n, C, 700)
    t = some_targets(n, 1, C, 701)
    buf = torch.empty(2 ** 31 + n * C, device=DEV)
    view = buf.as_strided((2, n, C), (2 ** 31, C, 1))
    view[0], view[1] = s[0].to(DEV), s[1].to(DEV)
    for order in (0, 1):
        assert torch.equal(run_rank(view, t, order).cpu().long(), oracle_ranks(s, t, order))


# ------------------------------------------------------------------------------------------------ mappings
def mapping_of(Cm, C, seed, repeat=False):
    g = torch.Generator().manual_seed(seed)
    m = torch.randperm(C, generator=g)[:Cm].tolist()
    if repeat and Cm > 2:
        m[2] = m[0]                     # two classes read one column: equal scores at different class indices
    return m


@pytest.mark.parametrize("Cm,repeat", [(1, False), (4, False), (4, True), (200, False), (200, True)])
def test_class_mapping_equals_the_gathered_scores(Cm, repeat):
    from octic_vits_amd import ops
    G, n, C = 3, 65, 1000
    m = mapping_of(Cm, C, 800 + Cm, repeat)
    for A in (1, 3):
        check_case(G, n, C, A, 810 + Cm + A, mapping=m)
    s = tied_scores(G, n, C, 820 + Cm)
    t = some_targets(n, 2, Cm, 821 + Cm)
    gathered = s[..., torch.tensor(m)].contiguous().to(DEV)
    for order in (0, 1):
        assert torch.equal(run_rank(strided(s), t, order, m), run_rank(gathered, t, order))
    for mt, tt in (("mean_accuracy", t[:, :1]), ("mean_per_class_accuracy", t[:, :1]), ("per_class_accuracy", t[:, :1]),
                   ("imagenet_real_accuracy", t)):
        for tie in ("strict", "index"):
            a = TopkAccuracy(mt, Cm, ks=(1, 2, 5), groups=G, class_mapping=m, tie=tie)
            b = TopkAccuracy(mt, Cm, ks=(1, 2, 5), groups=G, tie=tie)
            a.update(s.to(DEV), tt)
            b.update(gathered, tt)
            assert torch.equal(a.counters, b.counters) and torch.equal(a.rank, b.rank)


# ------------------------------------------------------------------------------------------------ oracle (b)
@pytest.mark.parametrize("tie", ["strict", "index"])
def test_all_metric_types_against_the_restated_reference_on_distinct_scores(tie):
    G, n, C = 3, 130, 37
    s = distinct_scores(G, n, C, 900)
    g = torch.Generator().manual_seed(901)
    t1 = torch.randint(0, C - 2, (n,), generator=g)                 # classes C-2 and C-1 have no sample
    tA = torch.randint(0, C, (n, 6), generator=g)
    tA[torch.rand(n, 6, generator=g) < 0.4] = -1
    tA[5] = -1
    m = {mt: TopkAccuracy(mt, C, ks=KS, groups=G, tie=tie, device=DEV) for mt in MetricType}
    mz = TopkAccuracy("mean_per_class_accuracy", C, ks=KS, groups=G, tie=tie, zero_support="zero")
    for lo, hi in ((0, 50), (50, 130)):                              # two updates
        for mt in MetricType:
            m[mt].update(s[:, lo:hi].to(DEV), (tA if mt == MetricType.IMAGENET_REAL_ACCURACY else t1)[lo:hi].to(DEV))
        mz.update(s[:, lo:hi].to(DEV), t1[lo:hi])
    got = {mt: m[mt].compute() for mt in MetricType}
    gotz = mz.compute()
    for gi in range(G):
        for i, k in enumerate(KS):
            tp, support = restated_multiclass(s[gi], t1, k, C)
            assert int(m[MetricType.MEAN_ACCURACY].counters[gi, 0]) == n
            assert int(m[MetricType.MEAN_ACCURACY].counters[gi, 1 + i]) == int(tp.sum())
            assert got[MetricType.MEAN_ACCURACY][gi][f"top-{k}"] == int(tp.sum()) / n
            for mt in (MetricType.PER_CLASS_ACCURACY, MetricType.MEAN_PER_CLASS_ACCURACY):
                assert torch.equal(m[mt].counters[gi, :, 0].cpu(), support) and torch.equal(m[mt].counters[gi, :, 1 + i].cpu(), tp)
            per = torch.where(support > 0, tp.double() / support.clamp(min=1).double(), torch.zeros(C, dtype=torch.float64))
            assert torch.equal(got[MetricType.PER_CLASS_ACCURACY][gi][f"top-{k}"], per)
            assert got[MetricType.MEAN_PER_CLASS_ACCURACY][gi][f"top-{k}"] == float(per.sum()) / int((support > 0).sum())
            assert gotz[gi][f"top-{k}"] == float(per.sum()) / C
            hits, rows = restated_real(s[gi], tA, k)
            assert m[MetricType.IMAGENET_REAL_ACCURACY].counters[gi].tolist()[0] == rows
            assert int(m[MetricType.IMAGENET_REAL_ACCURACY].counters[gi, 1 + i]) == hits
            assert got[MetricType.IMAGENET_REAL_ACCURACY][gi][f"top-{k}"] == hits / rows


# ------------------------------------------------------------------------------------------------ invariances
@pytest.mark.parametrize("mt", list(MetricType))
def test_pieces_reruns_and_cross_metric_identities(mt):
    G, n, C = 3, 65, 63
    s = tied_scores(G, n, C, 1000).to(DEV)
    A = 4 if mt == MetricType.IMAGENET_REAL_ACCURACY else 1
    t = some_targets(n, A, C, 1001)
    for tie in ("strict", "index"):
        whole = TopkAccuracy(mt, C, groups=G, tie=tie)
        whole.update(s, t)
        again = TopkAccuracy(mt, C, groups=G, tie=tie)
        again.update(s, t)
        assert torch.equal(whole.counters, again.counters) and torch.equal(whole.rank, again.rank)      # bitwise
        pieces = TopkAccuracy(mt, C, groups=G, tie=tie)
        ranks = []
        for lo, hi in ((0, 1), (1, 8), (8, n)):
            pieces.update(s[:, lo:hi], t[lo:hi])                     # row slices of the [G, n, C] tensor: views, ld_g = n C
            ranks.append(pieces.rank)
        assert torch.equal(pieces.counters, whole.counters) and torch.equal(torch.cat(ranks, 1), whole.rank)
        whole.reset()
        assert int(whole.counters.abs().sum()) == 0 and whole.rank is None
        whole.update(s, t)
        assert torch.equal(whole.counters, again.counters)
        if mt == MetricType.PER_CLASS_ACCURACY:                      # per-class hits and supports sum to the micro counters
            micro = TopkAccuracy("mean_accuracy", C, groups=G, tie=tie)
            micro.update(s, t)
            assert torch.equal(whole.counters.sum(1), micro.counters)
        if mt == MetricType.IMAGENET_REAL_ACCURACY:                  # ReaL with one target per row, all defined, is micro
            t1 = torch.randint(0, C, (n,), generator=torch.Generator().manual_seed(1002))
            real, micro = TopkAccuracy(mt, C, groups=G, tie=tie), TopkAccuracy("mean_accuracy", C, groups=G, tie=tie)
            real.update(s, t1.view(n, 1))
            micro.update(s, t1)
            assert torch.equal(real.counters, micro.counters) and real.compute() == micro.compute()
            assert int(real.counters[0, 0]) == n


# ------------------------------------------------------------------------------------------------ against what exists
@pytest.fixture(scope="module")
def small_probe():
    """embed_dim 64, 10 classes, a 2 x 2 x 3 grid; integer weights, biases and feature rows, so logits are exact and tie."""
    from octic_vits_amd import probe
    p = probe.LinearProbe(None, embed_dim=64, num_classes=10, n_last_blocks_list=(1, 4), learning_rates=(0.01, 0.1, 1.0),
                          batch_size=48, device=DEV)
    assert len(p.names) == 12
    g = torch.Generator().manual_seed(1100)
    p.flat.copy_(torch.randint(-1, 2, (p.flat.numel(),), generator=g).float())
    feats = [torch.randint(-1, 2, (B, p.width), generator=g).float().to(DEV) for B in (48, 17, 1)]
    return p, feats, g


def probe_logits(p, feats):
    return [p.forward_features(F).cpu().clone() for F in feats]


def test_evaluate_linear_classifiers_equals_probe_evaluate(small_probe):
    p, feats, g = small_probe
    labels = [torch.randint(0, 10, (F.shape[0],), generator=g).to(DEV) for F in feats]
    batches = list(zip(feats, labels))
    old = p.evaluate(batches, on_features=True)
    new = metrics.evaluate_linear_classifiers(p, batches, on_features=True)
    assert new["samples"] == old["samples"] == 66 and new["best_classifier"] == old["best_classifier"]
    assert list(new["classifiers"]) == list(old["classifiers"]) == p.names
    for name in p.names:
        assert set(new["classifiers"][name]) == {"top-1", "top-5"}
        assert new["classifiers"][name]["top-1"] == old["classifiers"][name]["top-1"]
        assert new["classifiers"][name]["top-5"] == old["classifiers"][name]["top-5"]
    assert len({old["classifiers"][n_]["top-1"] for n_ in p.names}) > 1          # the classifiers do differ
    # ... and the logits do tie at the label: the strict rule is what makes the two agree
    lg = torch.cat(probe_logits(p, feats), 1)
    lab = torch.cat(labels).cpu().view(-1, 1)
    assert not torch.equal(oracle_ranks(lg, lab, 0), oracle_ranks(lg, lab, 1))


def test_test_on_datasets_and_best_classifier_on_val(small_probe):
    p, feats, g = small_probe
    n = sum(F.shape[0] for F in feats)
    lg = torch.cat(probe_logits(p, feats), 1)                                    # [12, 66, 10]
    plain = torch.randint(0, 10, (n,), generator=g)
    real = torch.randint(0, 10, (n, 4), generator=g)
    real[torch.rand(n, 4, generator=g) < 0.5] = -1
    real[7] = -1
    mapping = [7, 2, 9, 2]                                                       # a repeated column
    mapped = torch.randint(0, 4, (n,), generator=g)

    def batches(t):
        out, lo = [], 0
        for F in feats:
            out.append((F, t[lo:lo + F.shape[0]]))                               # CPU targets: the driver uploads them
            lo += F.shape[0]
        return out

    val = metrics.evaluate_linear_classifiers(p, batches(plain), on_features=True)
    want_any = oracle_any(oracle_ranks(lg, plain.view(n, 1), 0), 10)
    top1 = [int(want_any[i, 1]) / int(want_any[i, 0]) for i in range(12)]
    assert [val["classifiers"][name]["top-1"] for name in p.names] == top1
    assert val["best_classifier"] == {"name": p.names[top1.index(max(top1))], "accuracy": max(top1)}
    chosen = p.names[min(range(12), key=lambda i: top1[i])]                      # NOT the best one
    ci = p.names.index(chosen)
    forced = metrics.evaluate_linear_classifiers(p, batches(plain), on_features=True, best_classifier_on_val=chosen)
    assert forced["best_classifier"] == {"name": chosen, "accuracy": top1[ci]} and forced["classifiers"] == val["classifiers"]

    got = metrics.test_on_datasets(p, [("plain", batches(plain), MetricType.MEAN_ACCURACY, None),
                                       ("real", batches(real), "imagenet_real_accuracy", None),
                                       ("mapped", batches(mapped), "mean_per_class_accuracy", mapping)], chosen, on_features=True)
    w_real = oracle_any(oracle_ranks(lg, real, 0), 10)[ci]
    w_cls = oracle_class(oracle_ranks(lg, mapped.view(n, 1), 0, mapping), mapped.view(n, 1), 4)[ci]
    per = w_cls[:, 1].double() / w_cls[:, 0].double()
    assert bool((w_cls[:, 0] > 0).all())
    assert got == {"plain_accuracy": 100.0 * top1[ci], "real_accuracy": 100.0 * (int(w_real[1]) / int(w_real[0])),
                   "mapped_accuracy": 100.0 * (float(per.sum()) / 4)}
    # per-class accuracy: vectors per classifier and no best classifier
    pc = metrics.evaluate_linear_classifiers(p, batches(mapped), metric_type="per_class_accuracy", class_mapping=mapping,
                                             on_features=True)
    assert pc["best_classifier"] is None and pc["samples"] == n
    assert torch.equal(pc["classifiers"][chosen]["top-1"], per)
    with pytest.raises(ValueError, match="per_class_accuracy"):
        metrics.test_on_datasets(p, [("x", batches(mapped), "per_class_accuracy", mapping)], chosen, on_features=True)


@pytest.fixture(scope="module")
def knn_case():
    g = torch.Generator().manual_seed(1200)
    C, M, D = 10, 300, 64
    centers = torch.randn(C, D, generator=g)
    y = torch.arange(M) % C
    f = torch.nn.functional.normalize(centers[y] + 1.5 * torch.randn(M, D, generator=g), dim=1)
    vy = torch.randint(0, C, (90,), generator=g)
    vf = torch.nn.functional.normalize(centers[vy] + 1.5 * torch.randn(90, D, generator=g), dim=1)
    val = [(vf[:64].to(DEV), vy[:64]), (vf[64:].to(DEV), vy[64:])]
    return f.to(DEV), y.to(DEV), val, C


def test_eval_knn_features_equals_knn_on_mean_accuracy(knn_case):
    from octic_vits_amd import knn
    f, y, val, _ = knn_case
    kw = dict(nb_knn=(10, 3, 20), temperature=0.07, n_per_class_list=(-1, 5), n_tries=2)
    old = knn.eval_knn_features(f, y, val, **kw)
    for averaging in ("mean_accuracy", "micro", metrics.AccuracyAveraging.MEAN_ACCURACY):
        assert metrics.eval_knn_features(f, y, val, accuracy_averaging=averaging, **kw) == old
    assert set(old) == {("full", 10), ("full", 3), ("full", 20), ("5 per class", 3), ("5 per class", 5)}
    assert len({v["top-1"] for v in old.values()}) > 1


def test_eval_knn_features_per_class_against_the_oracle(knn_case):
    from octic_vits_amd import knn
    f, y, val, C = knn_case
    module = knn.KnnModule(f, y, [3, 20], 0.07, num_classes=C)
    probas = {k: torch.cat([module(vf)[k].cpu() for vf, _ in val]) for k in (3, 20)}
    vy = torch.cat([t for _, t in val]).view(-1, 1)
    macro = metrics.eval_knn_features(f, y, val, nb_knn=(3, 20), accuracy_averaging="mean_per_class_accuracy")
    assert macro == metrics.eval_knn_features(f, y, val, nb_knn=(3, 20), accuracy_averaging="macro")
    none = metrics.eval_knn_features(f, y, val, nb_knn=(3, 20), accuracy_averaging=metrics.AccuracyAveraging.PER_CLASS_ACCURACY)
    for k in (3, 20):
        cnt = oracle_class(oracle_ranks(probas[k].unsqueeze(0), vy, 1), vy, C)[0]
        assert bool((cnt[:, 0] > 0).all())
        for i, top in enumerate(("top-1", "top-5")):
            per = cnt[:, 1 + i].double() / cnt[:, 0].double()
            assert torch.equal(none[("full", k)][top], per)
            assert macro[("full", k)][top] == float(per.sum()) / C
    # the probas are mostly exact zeros: the index rule is what ranks them
    assert not torch.equal(oracle_ranks(probas[3].unsqueeze(0), vy, 1), oracle_ranks(probas[3].unsqueeze(0), vy, 0))
