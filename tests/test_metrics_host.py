"""octic_vits_amd.metrics without a GPU: the reference's enums, the host reductions from hand-written integer counters (both
zero_support rules, a class without samples), argument validation, the GPU-only refusals, and the C ABI of csrc/topk_metric.hip
(declared, exported, bound, refusing bad shapes before any launch; the ABI version unchanged)."""
import ctypes
import subprocess

import pytest
import torch

from octic_vits_amd import _lib, knn, metrics, probe
from octic_vits_amd.build import SOURCES, build
from octic_vits_amd.metrics import AccuracyAveraging, MetricType, TopkAccuracy


def test_enums_carry_the_reference_names_and_values():
    assert {m.name: m.value for m in MetricType} == {
        "MEAN_ACCURACY": "mean_accuracy", "MEAN_PER_CLASS_ACCURACY": "mean_per_class_accuracy",
        "PER_CLASS_ACCURACY": "per_class_accuracy", "IMAGENET_REAL_ACCURACY": "imagenet_real_accuracy"}
    assert {a.name: a.value for a in AccuracyAveraging} == {
        "MEAN_ACCURACY": "micro", "MEAN_PER_CLASS_ACCURACY": "macro", "PER_CLASS_ACCURACY": "none"}
    assert str(MetricType.MEAN_ACCURACY) == "mean_accuracy" and str(AccuracyAveraging.MEAN_PER_CLASS_ACCURACY) == "macro"
    assert MetricType.MEAN_ACCURACY.accuracy_averaging is AccuracyAveraging.MEAN_ACCURACY
    assert MetricType.MEAN_PER_CLASS_ACCURACY.accuracy_averaging is AccuracyAveraging.MEAN_PER_CLASS_ACCURACY
    assert MetricType.PER_CLASS_ACCURACY.accuracy_averaging is AccuracyAveraging.PER_CLASS_ACCURACY
    assert MetricType.IMAGENET_REAL_ACCURACY.accuracy_averaging is None


def test_spellings_of_metric_type_and_averaging():
    for m in MetricType:
        assert metrics.as_metric_type(m) is m and metrics.as_metric_type(m.value) is m and metrics.as_metric_type(m.name) is m
    for a in AccuracyAveraging:
        assert metrics.as_accuracy_averaging(a) is a and metrics.as_accuracy_averaging(a.value) is a
        assert metrics.as_accuracy_averaging(a.name.lower()) is a and metrics.as_accuracy_averaging(MetricType[a.name]) is a
    with pytest.raises(ValueError):
        metrics.as_metric_type("accuracy")
    with pytest.raises(ValueError):
        metrics.as_accuracy_averaging("weighted")
    with pytest.raises(ValueError):
        metrics.as_accuracy_averaging(MetricType.IMAGENET_REAL_ACCURACY)


def test_host_reductions_from_hand_written_counters():
    ks = (1, 5)
    # micro / ReaL: [rows with a defined target, hits at 1, hits at 5]
    for mt in ("mean_accuracy", "imagenet_real_accuracy"):
        got = metrics.accuracies_from_counters(mt, [7, 3, 6], ks)
        assert got == {"top-1": 3 / 7, "top-5": 6 / 7}
        assert metrics.accuracies_from_counters(mt, [0, 0, 0], ks) == {"top-1": 0.0, "top-5": 0.0}
    # per class: [support, hits at 1, hits at 5] per class; class 2 has no sample
    c = torch.tensor([[4, 1, 4], [3, 3, 3], [0, 0, 0], [5, 0, 2]])
    per = metrics.accuracies_from_counters(MetricType.PER_CLASS_ACCURACY, c, ks)
    assert per["top-1"].dtype == torch.float64 and per["top-1"].tolist() == [1 / 4, 3 / 3, 0.0, 0 / 5]
    assert per["top-5"].tolist() == [4 / 4, 3 / 3, 0.0, 2 / 5]
    ex = metrics.accuracies_from_counters("mean_per_class_accuracy", c, ks, zero_support="exclude")
    ze = metrics.accuracies_from_counters("mean_per_class_accuracy", c, ks, zero_support="zero")
    s1 = float(torch.tensor([1 / 4, 3 / 3, 0.0, 0 / 5], dtype=torch.float64).sum())
    s5 = float(torch.tensor([4 / 4, 3 / 3, 0.0, 2 / 5], dtype=torch.float64).sum())
    assert ex == {"top-1": s1 / 3, "top-5": s5 / 3} and ze == {"top-1": s1 / 4, "top-5": s5 / 4}
    # the two rules agree once every class has a sample
    c[2] = torch.tensor([2, 1, 2])
    assert (metrics.accuracies_from_counters("mean_per_class_accuracy", c, ks, zero_support="exclude")
            == metrics.accuracies_from_counters("mean_per_class_accuracy", c, ks, zero_support="zero"))
    with pytest.raises(ValueError):
        metrics.accuracies_from_counters("mean_accuracy", c, ks)             # per-class counters for a micro metric
    with pytest.raises(ValueError):
        metrics.accuracies_from_counters("mean_accuracy", [7, 3, 6], ks, zero_support="drop")
    # an empty metric computes zeros without a device
    assert TopkAccuracy("mean_accuracy", 10, groups=2).compute() == [{"top-1": 0.0, "top-5": 0.0}] * 2
    assert build_metric_default_ks() == (1, 5)


def build_metric_default_ks():
    m = metrics.build_metric(MetricType.MEAN_PER_CLASS_ACCURACY, num_classes=7)
    assert isinstance(m, TopkAccuracy) and m.per_class and m.num_classes == 7 and m.tie == "strict"
    assert metrics.build_metric("imagenet_real_accuracy", num_classes=7, ks=(1, 2, 3)).ks == (1, 2, 3)
    return m.ks


def test_argument_validation():
    with pytest.raises(ValueError, match="ascending"):
        TopkAccuracy("mean_accuracy", 10, ks=(5, 1))
    with pytest.raises(ValueError, match="ascending"):
        TopkAccuracy("mean_accuracy", 10, ks=(1, 1))
    with pytest.raises(ValueError, match="ascending"):
        TopkAccuracy("mean_accuracy", 10, ks=(0, 1))
    with pytest.raises(ValueError, match="ascending"):
        TopkAccuracy("mean_accuracy", 10, ks=tuple(range(1, 10)))
    with pytest.raises(ValueError, match="tie"):
        TopkAccuracy("mean_accuracy", 10, tie="random")
    with pytest.raises(ValueError, match="zero_support"):
        TopkAccuracy("mean_accuracy", 10, zero_support="nan")
    with pytest.raises(ValueError, match="class_mapping"):
        TopkAccuracy("mean_accuracy", 2, class_mapping=[0, -1])
    with pytest.raises(ValueError, match="class_mapping"):
        TopkAccuracy("mean_accuracy", 2, class_mapping=[0.0, 1.0])
    with pytest.raises(ValueError, match="mapped classes"):
        TopkAccuracy("mean_accuracy", 3, class_mapping=[0, 1])
    scores, t1 = torch.zeros(6, 10), torch.zeros(6, dtype=torch.long)
    # a mapping that points past the scores' columns is refused at the update, before anything is uploaded
    with pytest.raises(ValueError, match=r"\[0, 10\)"):
        TopkAccuracy("mean_accuracy", 2, class_mapping=[0, 10]).update(scores, t1)
    with pytest.raises(ValueError, match="32"):
        TopkAccuracy("imagenet_real_accuracy", 10).update(scores, torch.zeros(6, 33, dtype=torch.long))
    for mt in ("per_class_accuracy", "mean_per_class_accuracy", "mean_accuracy"):
        with pytest.raises(ValueError, match="one target per row"):
            TopkAccuracy(mt, 10).update(scores, torch.zeros(6, 2, dtype=torch.long))
    with pytest.raises(ValueError, match="columns"):
        TopkAccuracy("mean_accuracy", 11).update(scores, t1)
    with pytest.raises(ValueError, match="groups"):
        TopkAccuracy("mean_accuracy", 10, groups=2).update(scores, t1)
    with pytest.raises(ValueError, match="target rows"):
        TopkAccuracy("mean_accuracy", 10).update(scores, torch.zeros(5, dtype=torch.long))
    with pytest.raises(ValueError, match="integers"):
        TopkAccuracy("mean_accuracy", 10).update(scores, torch.zeros(6))


def test_gpu_only_refusals():
    scores, t1 = torch.zeros(6, 10), torch.zeros(6, dtype=torch.long)
    with pytest.raises(RuntimeError, match="GPU only"):
        TopkAccuracy("mean_accuracy", 10, device="cpu")
    with pytest.raises(RuntimeError, match="GPU only"):
        TopkAccuracy("mean_accuracy", 10).update(scores, t1)
    with pytest.raises(RuntimeError, match="GPU only"):
        TopkAccuracy("imagenet_real_accuracy", 2, class_mapping=[3, 4]).update(scores, torch.zeros(6, 3, dtype=torch.long))
    from octic_vits_amd import ops
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.topk_rank(scores, t1)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.topk_count(torch.zeros(1, 6, 1, dtype=torch.int32), torch.zeros(1, 3, dtype=torch.int64), (1, 5), num_classes=10)
    p = probe.LinearProbe(None, embed_dim=64, num_classes=10, batch_size=16)
    for mt in MetricType:
        with pytest.raises(RuntimeError, match="GPU only"):
            metrics.evaluate_linear_classifiers(p, [], metric_type=mt)
    with pytest.raises(RuntimeError, match="GPU only"):
        metrics.test_on_datasets(p, [("val", [], "mean_accuracy", [0, 1])], None)
    with pytest.raises(KeyError):
        metrics.evaluate_linear_classifiers(p, [], best_classifier_on_val="no such classifier")
    f, y = torch.nn.functional.normalize(torch.randn(40, 64), dim=1), torch.arange(40) % 8
    for averaging in ("mean_per_class_accuracy", "macro", AccuracyAveraging.PER_CLASS_ACCURACY, "mean_accuracy"):
        with pytest.raises(RuntimeError, match="GPU only"):
            metrics.eval_knn_features(f, y, [(f, y)], nb_knn=(5,), accuracy_averaging=averaging)
    with pytest.raises(ValueError):
        metrics.eval_knn_features(f, y, [(f, y)], nb_knn=(5,), accuracy_averaging="weighted")
    with pytest.raises(NotImplementedError, match="gather_on_cpu"):
        metrics.eval_knn_features(f, y, [(f, y)], nb_knn=(5,), gather_on_cpu=True)
    with pytest.raises(NotImplementedError, match="gather_on_cpu"):
        metrics.eval_knn(None, [], [], gather_on_cpu=True)


def test_existing_refusals_name_the_new_module():
    p = probe.LinearProbe(None, embed_dim=64, num_classes=10, batch_size=16)
    with pytest.raises(NotImplementedError, match="octic_vits_amd.metrics"):
        p.evaluate([], metric_type="per_class_accuracy")
    with pytest.raises(NotImplementedError, match="octic_vits_amd.metrics"):
        p.evaluate([], class_mapping=[0, 1])
    with pytest.raises(NotImplementedError, match="octic_vits_amd.metrics") as e:
        knn._check_options("macro", False)
    assert "mean_accuracy" in str(e.value)


def test_symbols_declared_exported_bound_and_shapes_refused_before_any_launch():
    path = build()
    L = _lib.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    for s in ("octic_topk_rank", "octic_topk_count"):
        assert s in _lib._PROTOS and s in _lib.header_symbols() and f" {s}\n" in out
    assert "topk_metric.hip" in SOURCES
    header = open(_lib.HEADER_PATH).read()
    assert f"#define OCTIC_ABI_VERSION {_lib.ABI_VERSION}" in header and L.octic_abi_version() == _lib.ABI_VERSION == 20
    assert "#define OCTIC_TOPK_MAX_TARGETS 32" in header and metrics.MAX_TARGETS == 32
    a = ctypes.c_void_p(4096)
    ks = (ctypes.c_int * 2)(1, 5)

    def rank(scores=a, ld_g=6000, ld_r=1000, G=3, n=6, C=1000, cmap=None, Cm=1000, targets=a, A=1, order=0, out=a):
        return L.octic_topk_rank(scores, ld_g, ld_r, G, n, C, cmap, Cm, targets, A, order, out, None)

    assert rank(scores=None) == -4 and rank(targets=None) == -4 and rank(out=None) == -4
    assert rank(G=0) == -1 and rank(n=0) == -1 and rank(C=0) == -1 and rank(C=2 ** 31, Cm=2 ** 31) == -1
    assert rank(cmap=a, Cm=0) == -1 and rank(cmap=a, Cm=2 ** 31) == -1
    assert rank(Cm=999) == -1                                    # no mapping: Cm is C
    assert rank(A=0) == -1 and rank(A=33) == -1 and rank(order=2) == -1 and rank(order=-1) == -1
    assert rank(ld_r=999) == -1 and rank(ld_g=999) == -1 and rank(ld_r=-1000) == -1
    assert rank(G=2 ** 16, n=2 ** 15, ld_g=2 ** 40) == -1        # G n A = 2^31
    assert rank(G=2 ** 15, n=2 ** 11, A=32, ld_g=2 ** 40) == -1  # G n A = 2^31 through A
    assert rank(scores=ctypes.c_void_p(4098)) == -2 and rank(targets=ctypes.c_void_p(4100)) == -2

    def count(rk=a, G=3, n=6, A=1, Cm=1000, targets=a, mode=0, ks=ks, nk=2, counters=a):
        return L.octic_topk_count(rk, G, n, A, Cm, targets, mode, ks, nk, counters, None)

    assert count(rk=None) == -4 and count(ks=None) == -4 and count(counters=None) == -4 and count(mode=1, targets=None) == -4
    assert count(mode=2) == -1 and count(G=0) == -1 and count(n=0) == -1 and count(Cm=0) == -1 and count(nk=0) == -1
    assert count(nk=9) == -1 and count(A=33) == -1 and count(mode=1, A=2) == -1
    assert count(G=2 ** 16, n=2 ** 15) == -1
    assert count(ks=(ctypes.c_int * 2)(5, 1)) == -1 and count(ks=(ctypes.c_int * 2)(0, 1)) == -1
    assert count(ks=(ctypes.c_int * 2)(1, 1)) == -1
    assert count(counters=ctypes.c_void_p(4100)) == -2
