"""CPU-only: the C ABI of csrc/segknn.hip (declarations, exports, argument refusals before any launch, the plan query) and the
host pieces of octic_vits_amd.segmentation.KNNClassifier (grids, hyper-parameter names and their order against
tests/golden/seg_knn.npz, which make_seg_knn_golden.py recorded from the reference's own KNNClassifier; refused distances)."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

import seg_knn_cases as KC
from octic_vits_amd import _lib
from octic_vits_amd import segmentation as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KNN_SYMBOLS = ["octic_seg_knn_plan", "octic_seg_knn_workspace_bytes", "octic_seg_rownorms", "octic_seg_knn", "octic_seg_knn_vote"]
OK, ESHAPE, EALIGN, EDTYPE, ENULL = 0, -1, -2, -3, -4


def test_symbols_are_declared_exported_documented_and_the_abi_version_is_unchanged():
    L = _lib.lib()
    declared = _lib.header_symbols()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    for s in KNN_SYMBOLS:
        assert s in declared and s in _lib._PROTOS and hasattr(L, s) and s in text, s
    assert L.octic_abi_version() == 20 == _lib.ABI_VERSION
    from octic_vits_amd.build import SOURCES
    assert "segknn.hip" in SOURCES
    header = open(_lib.HEADER_PATH).read()
    assert "TOTAL ORDER: (distance, key row index)" in header          # the tie rule is stated where callers read it


def knn(L, Q=4096, ldq=64, n=100, K=8192, ldk=64, M=1000, D=64, qn=4096, kn=4096, skip=0, kmax=30, metrics=3, splits=1,
        il=4096, dl=4096, ic=4096, dc=4096, ldo=32, ws=4096):
    p = ctypes.c_void_p
    return L.octic_seg_knn(p(Q), ldq, n, p(K), ldk, M, D, p(qn), p(kn), p(skip), kmax, metrics, splits, p(il), p(dl), p(ic), p(dc),
                           ldo, p(ws), None)


def test_argument_refusals_return_their_codes_without_a_launch():
    """There is no device here: every call below must come back before touching one."""
    L = _lib.lib()
    p, null = ctypes.c_void_p(4096), ctypes.c_void_p(0)
    # bad D
    assert knn(L, D=60, ldq=60, ldk=60) == ESHAPE and knn(L, D=0) == ESHAPE and knn(L, D=32, ldq=32, ldk=32) == ESHAPE
    # k out of range
    assert knn(L, kmax=0) == ESHAPE and knn(L, kmax=33, ldo=40) == ESHAPE
    # fewer keys than neighbours, no rows, too many keys, unknown metric or split count
    # (M == kmax is served: asked of the queries that share octic_seg_knn's shape check and cannot launch - on a machine WITH a
    # device the entry point itself would run the kernel on the placeholder pointers)
    assert knn(L, M=29) == ESHAPE and L.octic_seg_knn_workspace_bytes(100, 29, 64, 30, 3, 1) == ESHAPE
    assert L.octic_seg_knn_workspace_bytes(100, 30, 64, 30, 3, 1) == 256
    assert L.octic_seg_knn_plan(100, 30, 64, 30, 3, (ctypes.c_int * 4)()) == OK
    assert knn(L, n=0) == ESHAPE and knn(L, M=2 ** 31) == ESHAPE and knn(L, metrics=0) == ESHAPE and knn(L, metrics=4) == ESHAPE
    assert knn(L, splits=-1) == ESHAPE and knn(L, splits=65) == ESHAPE
    # strides below the row width
    assert knn(L, ldq=32) == ESHAPE and knn(L, ldk=60) == ESHAPE and knn(L, ldo=29) == ESHAPE
    # null pointers: inputs, the outputs of a metric that is asked for, the workspace of a split launch
    assert knn(L, Q=0) == ENULL and knn(L, K=0) == ENULL and knn(L, qn=0) == ENULL and knn(L, kn=0) == ENULL
    assert knn(L, il=0) == ENULL and knn(L, dc=0) == ENULL and knn(L, metrics=1, dl=0) == ENULL and knn(L, metrics=2, ic=0) == ENULL
    assert knn(L, splits=3, ws=0) == ENULL
    # misaligned base or row stride
    assert knn(L, Q=4100) == EALIGN and knn(L, K=8196) == EALIGN and knn(L, ldq=66) == EALIGN and knn(L, ldk=65) == EALIGN
    assert knn(L, splits=3, ws=4096 + 64) == EALIGN

    assert L.octic_seg_rownorms(null, 64, 10, 64, p, None) == ENULL and L.octic_seg_rownorms(p, 64, 10, 64, null, None) == ENULL
    assert L.octic_seg_rownorms(p, 64, 0, 64, p, None) == ESHAPE and L.octic_seg_rownorms(p, 96, 10, 96, p, None) == ESHAPE
    assert L.octic_seg_rownorms(p, 32, 10, 64, p, None) == ESHAPE and L.octic_seg_rownorms(p, 66, 10, 64, p, None) == EALIGN

    def vote(idx=p, ldi=32, n=10, labels=p, esize=1, R=100, Lp=16, ks=(1, 3, 10, 30), out=p):
        arr = (ctypes.c_int * max(len(ks), 1))(*ks)
        return L.octic_seg_knn_vote(idx, ldi, n, labels, esize, R, Lp, arr, len(ks), out, None)

    assert vote(idx=null) == ENULL and vote(labels=null) == ENULL and vote(out=null) == ENULL
    assert vote(n=0) == ESHAPE and vote(R=0) == ESHAPE and vote(Lp=0) == ESHAPE and vote(ks=()) == ESHAPE
    assert vote(ks=tuple(range(1, 10))) == ESHAPE                       # more than 8 values
    assert vote(ks=(3, 1)) == ESHAPE and vote(ks=(1, 1)) == ESHAPE and vote(ks=(0, 3)) == ESHAPE and vote(ks=(1, 33), ldi=40) == ESHAPE
    assert vote(ldi=29) == ESHAPE and vote(esize=3) == EDTYPE and vote(esize=4, labels=ctypes.c_void_p(4098)) == EALIGN

    assert L.octic_seg_knn_workspace_bytes(100, 1000, 60, 30, 3, 0) == ESHAPE
    assert L.octic_seg_knn_workspace_bytes(100, 1000, 64, 33, 3, 0) == ESHAPE
    assert L.octic_seg_knn_workspace_bytes(100, 20, 64, 30, 3, 0) == ESHAPE
    assert L.octic_seg_knn_workspace_bytes(100, 1000, 64, 30, 3, 65) == ESHAPE
    assert L.octic_seg_knn_workspace_bytes(100, 1000, 64, 30, 3, 1) == 256
    # 3 splits of 8 key tiles: two metrics x (index, distance) x 3 x 100 x 30 four-byte entries, each part 256-byte aligned
    assert L.octic_seg_knn_workspace_bytes(100, 1000, 64, 30, 3, 3) == 4 * ((4 * 3 * 100 * 30 + 255) // 256 * 256)
    assert L.octic_seg_knn_workspace_bytes(100, 1000, 64, 30, 1, 3) == 2 * ((4 * 3 * 100 * 30 + 255) // 256 * 256)
    assert L.octic_seg_knn_workspace_bytes(100, 129, 64, 30, 1, 3) == 2 * ((4 * 2 * 100 * 30 + 255) // 256 * 256)   # 2 key tiles


def test_plan_splits_the_key_axis_only_while_query_tiles_leave_the_device_idle():
    """Without a device the library plans for 256 CUs.  splits >= 1 always; 1 once the query tiles fill the device; never
    more splits than a quarter of the key tiles, nor than 64."""
    out = (ctypes.c_int * 4)()
    L = _lib.lib()
    for n, M, D, kmax, metrics in [(1, 30, 64, 30, 3), (8192, 262144, 1280, 30, 3), (300, 2000, 64, 3, 1), (127, 129, 192, 1, 2),
                                   (40000, 3_564_000, 1280, 30, 3), (356_400, 3_207_600, 1280, 32, 3), (128 * 256, 10 ** 6, 64, 10, 1)]:
        assert L.octic_seg_knn_plan(n, M, D, kmax, metrics, out) == OK
        splits, qt, kt, cls = list(out)
        ktiles = -(-M // kt)
        assert qt == 128 and kt == 128 and 1 <= splits <= 64 and splits <= max(1, ktiles // 4) and cls == (1 if splits > 1 else 0)
        if -(-n // qt) >= 256:
            assert splits == 1
        assert _lib.plan("octic_seg_knn_plan", n, M, D, kmax, metrics) == (splits, qt, kt, cls)
    assert L.octic_seg_knn_plan(8192, 262144, 1280, 30, 3, out) == OK and out[0] == 4          # 64 query tiles on 256 CUs
    assert L.octic_seg_knn_plan(1, 262144, 1280, 30, 3, out) == OK and out[0] == 64
    assert L.octic_seg_knn_plan(100, 1000, 60, 30, 3, out) == ESHAPE and L.octic_seg_knn_plan(100, 1000, 64, 0, 3, out) == ESHAPE
    assert L.octic_seg_knn_plan(100, 1000, 64, 30, 3, None) == ENULL
    assert _lib.plan("octic_seg_knn_plan", 100, 1000, 60, 30, 3) is None


def test_grids_names_and_order_match_the_reference():
    g = np.load(os.path.join(GOLDEN, "seg_knn.npz"))
    clf = S.KNNClassifier(ignore_labels=KC.IGNORE)
    assert clf.hparam_grids == {"num_neighbors": (1, 3, 10, 30), "distance": ("cosine", "L2")}
    assert (clf.num_neighbors, clf.distance, clf.train_set_subsampling, clf.inference_bs, clf.train_set_chunk_size) == (1, "cosine", 1, 1024, 262144)
    names, grids = zip(*clf.hparam_grids.items())
    ours = [S.hparam_name("mIoU", names, p) for p in itertools.product(*grids)]
    assert ours == list(g["select_names_sub1"]) == list(g["select_names_sub3"])
    assert ours[0] == "mIoU_num_neighbors=1_distance=cosine" and ours[-1] == "mIoU_num_neighbors=30_distance=L2"
    keys = ["hparam_fitting.knn." + s for s in ours] + [f"labels_knn_{m}" for m in S.metrics_dict]
    assert sorted(keys) == list(g["eval_model_keys"])
    assert S.classifiers_dict["knn"] is S.KNNClassifier and list(S.classifiers_dict) == ["logreg", "knn"]


def test_select_hparams_takes_the_reference_choice_on_the_recorded_scores(monkeypatch):
    """select_hparams with fit / predict_grid / metric replaced by the recorded scores: one fit, one pass, the reference's keys
    in its order, and its choice (the first maximum)."""
    g = np.load(os.path.join(GOLDEN, "seg_knn.npz"))
    for sub in KC.SUBSAMPLINGS:
        scores = iter(g[f"select_scores_sub{sub}"].tolist())
        calls = []
        clf = S.KNNClassifier(ignore_labels=KC.IGNORE)
        monkeypatch.setattr(clf, "fit", lambda f, l: calls.append("fit"))
        monkeypatch.setattr(clf, "predict_grid", lambda f, ks, ds: calls.append("grid") or {(k, d): None for k in ks for d in ds})
        monkeypatch.setitem(S.metrics_dict, "mIoU", lambda yt, yp, ign: next(scores))
        metrics = clf.select_hparams(None, None, None, None)
        assert calls == ["fit", "grid"]
        assert list(metrics) == list(g[f"select_names_sub{sub}"]) and list(metrics.values()) == g[f"select_scores_sub{sub}"].tolist()
        assert (clf.num_neighbors, clf.distance) == (int(g[f"best_k_sub{sub}"]), str(g[f"best_distance_sub{sub}"]))
    tie = iter([0.5, 0.7, 0.7, 0.1])
    clf = S.KNNClassifier(ignore_labels=KC.IGNORE, num_neighbors=(3, 10))
    monkeypatch.setattr(clf, "fit", lambda f, l: None)
    monkeypatch.setattr(clf, "predict_grid", lambda f, ks, ds: {(k, d): None for k in ks for d in ds})
    monkeypatch.setitem(S.metrics_dict, "mIoU", lambda yt, yp, ign: next(tie))
    clf.select_hparams(None, None, None, None)
    assert (clf.num_neighbors, clf.distance) == (3, "L2")                # the first maximum
    one = S.KNNClassifier(ignore_labels=KC.IGNORE, num_neighbors=(10,), distance=("L2",))
    assert one.select_hparams(None, None, None, None) == {} and (one.num_neighbors, one.distance) == (10, "L2")


def test_refusals():
    for d in ("L1", "Linf", "inner_product"):
        with pytest.raises(NotImplementedError):
            S.KNNClassifier(ignore_labels=KC.IGNORE, distance=("cosine", d))
        clf = S.KNNClassifier(ignore_labels=KC.IGNORE)
        clf.distance = d
        with pytest.raises(NotImplementedError):
            clf._check_distance(clf.distance)
    with pytest.raises(ValueError):
        S.KNNClassifier(ignore_labels=KC.IGNORE, distance=("chebyshev",))
    with pytest.raises(ValueError):
        S.KNNClassifier(ignore_labels=KC.IGNORE, num_neighbors=(1, 33))
    with pytest.raises(ValueError):
        S.KNNClassifier(ignore_labels=KC.IGNORE, num_neighbors=(0,))
    with pytest.raises(ValueError):
        S.KNNClassifier(ignore_labels=KC.IGNORE, dtype="float16")
    X, lab = torch.zeros(64, 64), torch.zeros(64, 4, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU only"):
        S.KNNClassifier(ignore_labels=KC.IGNORE).fit(X, lab)
    fitted = S.KNNClassifier(ignore_labels=KC.IGNORE)
    fitted.train_X = X
    with pytest.raises(RuntimeError, match="GPU only"):
        fitted.predict(X)
    from octic_vits_amd import ops
    for call in (lambda: ops.seg_rownorms(X), lambda: ops.seg_knn(X, X, X[:, 0], X[:, 0], None, 3),
                 lambda: ops.seg_knn_vote(torch.zeros(4, 3, dtype=torch.int32), lab, (1, 3))):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()


def test_eval_model_still_refuses_knn_and_eval_features_checks_names():
    with pytest.raises(NotImplementedError):
        S.eval_model(torch.nn.Linear(2, 2), [], [], classifiers=("knn",))
    with pytest.raises(NotImplementedError):
        S.eval_model(torch.nn.Linear(2, 2), [], [], classifiers=("logreg", "knn"))
    with pytest.raises(ValueError):
        S.eval_model(torch.nn.Linear(2, 2), [], [], classifiers=("svm",))
    with pytest.raises(ValueError):
        S.eval_features(S.SegSplits(None, None, None, None, 0, 1), classifiers=("svm",))
    with pytest.raises(RuntimeError, match="GPU only"):
        S.extract_splits(torch.nn.Linear(2, 2), [], [])
    import inspect
    assert inspect.signature(S.eval_features).parameters["classifiers"].default == ("logreg", "knn")
    assert list(inspect.signature(S.extract_splits).parameters) == ["model", "train", "test", "val", "standardization", "val_seed"]
