"""CPU-only: the C ABI of csrc/knn_cls.hip (declarations, exports, argument refusals before any launch, workspace sizes, the plan
query) and the host pieces of octic_vits_amd.knn (the class mapping, filter_train's draw, the k_list rule and the result keys
against tests/golden/knn_cls.npz, which make_knn_cls_golden.py recorded from the reference's own knn.py; the refusals)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import knn_cls_cases as KC
from octic_vits_amd import _lib
from octic_vits_amd import knn as KN

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SYMBOLS = ["octic_knn_topk_plan", "octic_knn_topk_workspace_bytes", "octic_knn_topk", "octic_knn_vote"]
OK, ESHAPE, EALIGN, EDTYPE, ENULL = 0, -1, -2, -3, -4
KMAX = 256


def test_symbols_are_declared_exported_documented_and_the_abi_version_is_unchanged():
    L = _lib.lib()
    declared = _lib.header_symbols()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    for s in SYMBOLS:
        assert s in declared and s in _lib._PROTOS and hasattr(L, s) and s in text, s
    assert L.octic_abi_version() == 20 == _lib.ABI_VERSION
    from octic_vits_amd.build import SOURCES
    assert "knn_cls.hip" in SOURCES
    header = open(_lib.HEADER_PATH).read()
    assert "TOTAL ORDER: (similarity descending, key row index ascending)" in header   # the tie rule, where callers read it
    assert f"#define OCTIC_KNN_KMAX {KMAX}" in header and KMAX >= 200
    from octic_vits_amd import ops
    assert ops.KNN_CLS_KMAX == KMAX == KN.KMAX


def topk(L, Q=4096, ldq=64, n=100, K=8192, ldk=64, M=1000, D=64, kmax=200, splits=1, idx=4096, sim=4096, ldo=200, ws=4096):
    p = ctypes.c_void_p
    return L.octic_knn_topk(p(Q), ldq, n, p(K), ldk, M, D, kmax, splits, p(idx), p(sim), ldo, p(ws), None)


def vote(L, sim=4096, idx=4096, ldi=200, n=10, kmax=200, labels=4096, M=1000, C=16, inv_T=1 / 0.07, ks=(10, 20, 100, 200),
         probas=4096, targets=0, counters=0):
    p = ctypes.c_void_p
    arr = (ctypes.c_int * max(len(ks), 1))(*ks)
    return L.octic_knn_vote(p(sim), p(idx), ldi, n, kmax, p(labels), M, C, inv_T, arr, len(ks), p(probas), p(targets), p(counters),
                            None)


def test_argument_refusals_return_their_codes_without_a_launch():
    """There is no device here: every call below must come back before touching one."""
    L = _lib.lib()
    # bad D
    assert topk(L, D=60, ldq=60, ldk=60) == ESHAPE and topk(L, D=0) == ESHAPE and topk(L, D=32, ldq=32, ldk=32) == ESHAPE
    # k out of range, fewer keys than neighbours, no rows, too many keys, a split count out of range
    assert topk(L, kmax=0) == ESHAPE and topk(L, kmax=KMAX + 1, ldo=300) == ESHAPE
    assert topk(L, M=199) == ESHAPE and L.octic_knn_topk_workspace_bytes(100, 200, 64, 200, 1) == 256     # M == kmax is served
    assert topk(L, n=0) == ESHAPE and topk(L, M=2 ** 31) == ESHAPE and topk(L, splits=-1) == ESHAPE and topk(L, splits=65) == ESHAPE
    # strides below the row width
    assert topk(L, ldq=32) == ESHAPE and topk(L, ldk=60) == ESHAPE and topk(L, ldo=199) == ESHAPE
    # null pointers, the workspace of a split launch included
    assert topk(L, Q=0) == ENULL and topk(L, K=0) == ENULL and topk(L, idx=0) == ENULL and topk(L, sim=0) == ENULL
    assert topk(L, splits=3, ws=0) == ENULL
    # misaligned base or row stride
    assert topk(L, Q=4100) == EALIGN and topk(L, K=8196) == EALIGN and topk(L, ldq=66) == EALIGN and topk(L, ldk=65) == EALIGN
    assert topk(L, idx=4098) == EALIGN and topk(L, sim=4097) == EALIGN and topk(L, splits=3, ws=4096 + 64) == EALIGN

    assert vote(L, sim=0) == ENULL and vote(L, idx=0) == ENULL and vote(L, labels=0) == ENULL and vote(L, probas=0) == ENULL
    assert vote(L, targets=4096, counters=0) == ENULL
    assert vote(L, n=0) == ESHAPE and vote(L, M=0) == ESHAPE and vote(L, kmax=0) == ESHAPE and vote(L, kmax=KMAX + 1, ldi=300) == ESHAPE
    assert vote(L, ldi=199) == ESHAPE and vote(L, C=4) == ESHAPE and vote(L, inv_T=0.0) == ESHAPE and vote(L, inv_T=-1.0) == ESHAPE
    assert vote(L, ks=()) == ESHAPE and vote(L, ks=tuple(range(1, 10))) == ESHAPE                  # none, more than 8
    assert vote(L, ks=(20, 10)) == ESHAPE and vote(L, ks=(10, 10)) == ESHAPE and vote(L, ks=(0, 10)) == ESHAPE   # not ascending
    assert vote(L, ks=(10, 201)) == ESHAPE and vote(L, kmax=100, ks=(10, 101)) == ESHAPE             # above kmax
    assert vote(L, labels=4100) == EALIGN and vote(L, targets=4100, counters=4096) == EALIGN
    assert vote(L, targets=4096, counters=4100) == EALIGN and vote(L, sim=4098) == EALIGN

    ws = L.octic_knn_topk_workspace_bytes
    assert ws(100, 1000, 60, 200, 0) == ESHAPE and ws(100, 1000, 64, KMAX + 1, 0) == ESHAPE and ws(100, 100, 64, 200, 0) == ESHAPE
    assert ws(100, 1000, 64, 200, 65) == ESHAPE and ws(100, 1000, 64, 200, -1) == ESHAPE


def test_workspace_bytes_follow_the_resolved_split_count():
    ws = _lib.lib().octic_knn_topk_workspace_bytes
    part = lambda s, n, k: (4 * s * n * k + 255) // 256 * 256                 # noqa: E731
    assert ws(100, 1000, 64, 200, 1) == 256
    # 8 key tiles of 128: 3 splits of 3 tiles; (index, similarity) x 3 x 100 x 200 four-byte entries, each part 256-byte aligned
    assert ws(100, 1000, 64, 200, 3) == 2 * part(3, 100, 200)
    assert ws(100, 1000, 64, 200, 5) == 2 * part(4, 100, 200)                  # 2 tiles a split: 4 splits are not empty
    assert ws(100, 1000, 64, 200, 64) == 2 * part(8, 100, 200)                 # never more splits than key tiles
    assert ws(7, 200, 64, 200, 2) == 2 * part(2, 7, 200) and ws(7, 200, 64, 7, 5) == 2 * part(2, 7, 7)
    assert ws(100, 1000, 64, 200, 0) == 256                                    # the plan: too few key tiles to split


def test_plan_splits_the_key_axis_only_while_query_tiles_leave_the_device_idle():
    """Without a device the library plans for 256 CUs.  splits >= 1 always; 1 once the query tiles fill the device; never more
    than 64, and never more than the key tiles."""
    out = (ctypes.c_int * 4)()
    L = _lib.lib()
    for n, M, D, kmax in [(1, 200, 64, 200), (8192, 262144, 1280, 200), (300, 2000, 64, 3), (63, 129, 192, 1),
                          (50000, 1_281_167, 1280, 200), (256, 1_281_167, 1280, 200), (64 * 256, 10 ** 6, 64, 10),
                          (64 * 255 + 1, 10 ** 6, 64, 256), (64 * 255, 10 ** 6, 64, 256)]:
        assert L.octic_knn_topk_plan(n, M, D, kmax, out) == OK
        splits, qt, kt, cls = list(out)
        assert qt == 64 and kt == 128 and 1 <= splits <= 64 and splits <= -(-M // kt) and cls == (1 if splits > 1 else 0)
        if -(-n // qt) >= 256:
            assert splits == 1
        assert _lib.plan("octic_knn_topk_plan", n, M, D, kmax) == (splits, qt, kt, cls)
        assert L.octic_knn_topk_workspace_bytes(n, M, D, kmax, 0) == L.octic_knn_topk_workspace_bytes(n, M, D, kmax, splits)
    assert L.octic_knn_topk_plan(8192, 262144, 1280, 200, out) == OK and out[0] == 2        # 128 query tiles on 256 CUs
    assert L.octic_knn_topk_plan(1, 262144, 1280, 200, out) == OK and out[0] == 64
    assert L.octic_knn_topk_plan(64 * 255, 10 ** 6, 64, 256, out) == OK and out[0] == 2
    assert L.octic_knn_topk_plan(100, 1000, 60, 200, out) == ESHAPE and L.octic_knn_topk_plan(100, 1000, 64, 0, out) == ESHAPE
    assert L.octic_knn_topk_plan(100, 1000, 64, 200, None) == ENULL
    assert _lib.plan("octic_knn_topk_plan", 100, 1000, 60, 200) is None


def test_mapping_draw_k_list_and_result_keys_match_the_reference():
    g = np.load(os.path.join(GOLDEN, "knn_cls.npz"))
    p = KC.problem(g)
    labels = torch.from_numpy(p["key_labels"])
    mapping = KN.create_class_indices_mapping(labels)
    assert list(mapping) == sorted(set(p["key_labels"].tolist()))
    for c, rows in mapping.items():
        assert tuple(rows.shape) == (int((p["key_labels"] == c).sum()), 1)
        assert np.array_equal(rows[:, 0].numpy(), np.nonzero(p["key_labels"] == c)[0])
    torch.manual_seed(1234)
    state = torch.get_rng_state()
    for t in range(KC.FEWSHOT_TRIES):
        rows = KN.filter_train(mapping, KC.FEWSHOT_NPC, seed=t)
        assert rows.dim() == 1 and np.array_equal(rows.numpy(), g[f"fewshot{t}_rows"]), t
    assert torch.equal(torch.get_rng_state(), state)                     # the global generator is left alone
    assert KN.k_list_for(KC.NB_KNN, KC.FEWSHOT_NPC) == g["fewshot_k_list"].tolist() == [5]
    assert KN.k_list_for(KC.NB_KNN, 20) == [10, 20] and KN.k_list_for(KC.NB_KNN, 150) == [10, 20, 100, 150]
    assert KN.k_list_for(KC.NB_KNN, 1000) == [10, 20, 100, 200, 1000]

    made = []

    def module(train_features, train_labels, nb_knn):
        made.append((train_features, train_labels, nb_knn))
        return len(made) - 1

    X = torch.from_numpy(p["keys"])
    md = KN.create_module_dict(module=module, n_per_class_list=[-1, KC.FEWSHOT_NPC], n_tries=KC.FEWSHOT_TRIES, nb_knn=list(KC.NB_KNN),
                               train_features=X, train_labels=labels)
    assert list(md) == list(g["module_keys"]) == ["full", "5 per class"]
    assert list(md["full"]) == ["1"] and list(md["5 per class"]) == list(g["try_keys"]) == ["0", "1"]
    assert made[0][2] == list(KC.NB_KNN) and made[0][0] is X
    for t in range(KC.FEWSHOT_TRIES):
        f, l, ks = made[md["5 per class"][str(t)]]
        assert ks == [5] and torch.equal(f, X[g[f"fewshot{t}_rows"]]) and torch.equal(l, labels[g[f"fewshot{t}_rows"]])
    keys = [("full", k) for k in KC.NB_KNN] + [("5 per class", 5)]
    assert [repr(k) for k in keys] == list(g["result_keys"])
    lines = KN.results_lines({k: {"top-1": 0.5, "top-5": 0.75} for k in keys})
    assert list(lines) == list(g["result_line_keys"])


def test_results_lines_format():
    lines = KN.results_lines({("full", 10): {"top-1": 0.25, "top-5": torch.tensor(0.5)}, ("5 per class", 5): {"top-1": 0.0, "top-5": 1.0}})
    assert lines == {"('full', 10) Top 1": 25.0, "('full', 10) Top 5": 50.0, "('5 per class', 5) Top 1": 0.0,
                     "('5 per class', 5) Top 5": 100.0}
    assert all(type(v) is float for v in lines.values())


def test_refusals(monkeypatch):
    X, y = torch.zeros(300, 64), torch.arange(300) % 7
    for bad in ("mean_per_class_accuracy", "imagenet_real_accuracy"):
        with pytest.raises(NotImplementedError, match="mean_accuracy"):
            KN.eval_knn_features(X, y, [], accuracy_averaging=bad)
        with pytest.raises(NotImplementedError, match="mean_accuracy"):
            KN.eval_knn(torch.nn.Linear(2, 2), [], [], accuracy_averaging=bad)
    with pytest.raises(NotImplementedError, match="gather_on_cpu"):
        KN.eval_knn_features(X, y, [], gather_on_cpu=True)
    with pytest.raises(NotImplementedError, match="gather_on_cpu"):
        KN.eval_knn(torch.nn.Linear(2, 2), [], [], gather_on_cpu=True)
    with pytest.raises(ValueError, match="multiple of 64"):
        KN.KnnModule(torch.zeros(300, 96), y, [10], 0.07, num_classes=7)
    with pytest.raises(ValueError, match="list length"):
        KN.KnnModule(X, y, [10, KMAX + 1], 0.07, num_classes=7)
    with pytest.raises(ValueError, match="list length"):
        KN.KnnModule(X, y, [0, 10], 0.07, num_classes=7)
    with pytest.raises(ValueError, match="training rows"):
        KN.KnnModule(X[:100], y[:100], [10, 200], 0.07, num_classes=7)
    with pytest.raises(ValueError, match="5 classes"):
        KN.KnnModule(X, y, [10], 0.07, num_classes=4)
    with pytest.raises(ValueError, match="8 distinct"):
        KN.KnnModule(X, y, list(range(1, 10)), 0.07, num_classes=7)
    m = KN.KnnModule(X, y, [10, 20, 100, 200], 0.07, num_classes=7)
    assert (m.nb_knn, m.max_k, m.T, m.num_classes) == ([10, 20, 100, 200], 200, 0.07, 7)
    for call in (lambda: m(X[:4]), lambda: m.compute_neighbors(X[:4]), lambda: KN.eval_knn_features(X, y, []),
                 lambda: KN.extract_features(torch.nn.Linear(2, 2), []), lambda: KN.eval_knn(torch.nn.Linear(2, 2), [], [])):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()
    from octic_vits_amd import ops
    for call in (lambda: ops.knn_topk(X[:4], X, 10),
                 lambda: ops.knn_vote(torch.zeros(4, 10), torch.zeros(4, 10, dtype=torch.int32), y, 7, 1.0, (10,))):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()
    # the reference shards the training features over ranks: a group of more than one rank is refused, not mis-evaluated
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(NotImplementedError, match="more than one rank"):
        KN.KnnModule(X, y, [10], 0.07, num_classes=7)
    with pytest.raises(NotImplementedError, match="more than one rank"):
        KN.eval_knn_features(X, y, [])
    with pytest.raises(NotImplementedError, match="more than one rank"):
        KN.eval_knn(torch.nn.Linear(2, 2), [], [])
