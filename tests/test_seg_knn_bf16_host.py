"""CPU-only: the bf16 half of csrc/segknn.hip's C ABI (octic_seg_rownorms_bf16, octic_seg_knn_bf16: declared, exported,
documented, every refusal before a launch), KNNClassifier(dtype="bfloat16") on the host, the dtype rules of ops.seg_knn, and
tests/golden/seg_knn_bf16.npz against the numpy statement of the engine's rule (tests/golden/seg_knn_bf16_cases.py): the
float64 ordering of the bf16-rounded operands is a valid top-k of the distances the reference itself computed in bf16."""
import ctypes
import os

import numpy as np
import pytest
import torch

import seg_knn_bf16_cases as BC
import seg_knn_cases as KC
from octic_vits_amd import _lib, ops
from octic_vits_amd import segmentation as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEW_SYMBOLS = ["octic_seg_rownorms_bf16", "octic_seg_knn_bf16"]
OK, ESHAPE, EALIGN, EDTYPE, ENULL = 0, -1, -2, -3, -4


def test_constructor_accepts_bfloat16_and_reports_the_dtype():
    clf = S.KNNClassifier(ignore_labels=KC.IGNORE, dtype="bfloat16")
    assert clf.dtype == torch.bfloat16
    assert clf.hparam_grids == {"num_neighbors": (1, 3, 10, 30), "distance": ("cosine", "L2")}
    assert S.KNNClassifier(ignore_labels=KC.IGNORE).dtype == torch.float32
    assert S.KNNClassifier(ignore_labels=KC.IGNORE, dtype="float32").dtype == torch.float32
    for other in ("float16", "float64", "bf16", "half", ""):
        with pytest.raises(ValueError):
            S.KNNClassifier(ignore_labels=KC.IGNORE, dtype=other)
    X, lab = torch.zeros(64, 64), torch.zeros(64, 4, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU only"):          # no CPU path at this dtype either
        clf.fit(X, lab)
    clf.train_X = X
    with pytest.raises(RuntimeError, match="GPU only"):
        clf.predict(X)


def test_symbols_are_declared_exported_documented_and_the_abi_version_is_unchanged():
    L = _lib.lib()
    declared = _lib.header_symbols()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    for s in NEW_SYMBOLS:
        assert s in declared and s in _lib._PROTOS and hasattr(L, s) and s in text, s
    assert "eval_config.yaml" in text                                    # the reference lines the new entries stand for
    assert _lib._PROTOS["octic_seg_knn_bf16"] == _lib._PROTOS["octic_seg_knn"]          # the argument list of the f32 entry
    assert _lib._PROTOS["octic_seg_rownorms_bf16"] == _lib._PROTOS["octic_seg_rownorms"]
    assert L.octic_abi_version() == 20 == _lib.ABI_VERSION                # additive: a stale library lacks the symbol instead


def knn(L, Q=4096, ldq=64, n=100, K=8192, ldk=64, M=1000, D=64, qn=4096, kn=4096, skip=0, kmax=30, metrics=3, splits=1,
        il=4096, dl=4096, ic=4096, dc=4096, ldo=32, ws=4096):
    p = ctypes.c_void_p
    return L.octic_seg_knn_bf16(p(Q), ldq, n, p(K), ldk, M, D, p(qn), p(kn), p(skip), kmax, metrics, splits, p(il), p(dl), p(ic),
                                p(dc), ldo, p(ws), None)


def test_argument_refusals_return_their_codes_without_a_launch():
    """Every call below is refused, so none reaches a launch (none may: the pointers are placeholders)."""
    L = _lib.lib()
    p, null = ctypes.c_void_p(4096), ctypes.c_void_p(0)
    assert knn(L, D=60, ldq=64, ldk=64) == ESHAPE and knn(L, D=0) == ESHAPE and knn(L, D=32) == ESHAPE and knn(L, D=96, ldq=96, ldk=96) == ESHAPE
    assert knn(L, kmax=0) == ESHAPE and knn(L, kmax=33, ldo=40) == ESHAPE
    assert knn(L, M=29) == ESHAPE and knn(L, n=0) == ESHAPE and knn(L, M=2 ** 31) == ESHAPE
    assert knn(L, metrics=0) == ESHAPE and knn(L, metrics=4) == ESHAPE and knn(L, splits=-1) == ESHAPE and knn(L, splits=65) == ESHAPE
    assert knn(L, ldq=56) == ESHAPE and knn(L, ldk=56) == ESHAPE and knn(L, ldo=29) == ESHAPE
    assert knn(L, Q=0) == ENULL and knn(L, K=0) == ENULL and knn(L, qn=0) == ENULL and knn(L, kn=0) == ENULL
    assert knn(L, il=0) == ENULL and knn(L, dc=0) == ENULL and knn(L, metrics=1, dl=0) == ENULL and knn(L, metrics=2, ic=0) == ENULL
    assert knn(L, splits=3, ws=0) == ENULL and knn(L, splits=3, ws=4096 + 64) == EALIGN
    # rows of bf16 are 16-byte aligned: the base, and a stride that is a multiple of 8 ELEMENTS (4, fine for f32 rows, is not)
    assert knn(L, Q=4104) == EALIGN and knn(L, K=8200) == EALIGN
    assert knn(L, ldq=68) == EALIGN and knn(L, ldk=68) == EALIGN and knn(L, ldq=66) == EALIGN and knn(L, ldk=65) == EALIGN

    rn = L.octic_seg_rownorms_bf16
    assert rn(null, 64, 10, 64, p, None) == ENULL and rn(p, 64, 10, 64, null, None) == ENULL
    assert rn(p, 64, 0, 64, p, None) == ESHAPE and rn(p, 96, 10, 96, p, None) == ESHAPE and rn(p, 32, 10, 64, p, None) == ESHAPE
    assert rn(p, 68, 10, 64, p, None) == EALIGN and rn(ctypes.c_void_p(4104), 64, 10, 64, p, None) == EALIGN
    # the plan and the workspace answer for both element types: nothing in them depends on the rows
    assert L.octic_seg_knn_workspace_bytes(100, 1000, 64, 30, 3, 3) == 4 * ((4 * 3 * 100 * 30 + 255) // 256 * 256)
    assert _lib.plan("octic_seg_knn_plan", 8192, 262144, 1280, 30, 3)[1:3] == (128, 128)


def test_ops_refuse_cpu_tensors_and_mixed_dtypes():
    X = torch.zeros(64, 64)
    Xb = X.to(torch.bfloat16)
    for call in (lambda: ops.seg_rownorms(Xb), lambda: ops.seg_knn(Xb, Xb, X[:, 0], X[:, 0], None, 3)):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()
    for q, k in ((X, Xb), (Xb, X)):
        with pytest.raises(ValueError, match="share one dtype"):
            ops.seg_knn(q, k, X[:, 0], X[:, 0], None, 3)


def _golden():
    g = np.load(os.path.join(GOLDEN, "seg_knn_bf16.npz"))
    return g, KC.problem(g)


def test_the_golden_regenerates_its_features_and_holds_what_the_tests_need():
    g, p = _golden()
    assert p["keys"].shape == (KC.N_KEYS, KC.D) and p["queries"].shape == (KC.N_QUERIES, KC.D)
    for sub in KC.SUBSAMPLINGS:
        for d in KC.DISTANCES:
            ref = g[f"ref_{d}_sub{sub}"]
            assert ref.dtype == np.uint16 and ref.shape == (KC.N_QUERIES, len(range(0, KC.N_KEYS, sub)))
        assert g[f"pred_sub{sub}"].shape == (8, KC.N_QUERIES, KC.L) and g[f"pred_sub{sub}"].dtype == np.uint8
        assert list(g[f"select_names_sub{sub}"])[0] == "mIoU_num_neighbors=1_distance=cosine"
    # round_bf16 is torch's cast
    X = np.concatenate([p["keys"], p["queries"]])
    assert np.array_equal(BC.round_bf16(X), torch.from_numpy(X).to(torch.bfloat16).float().numpy())
    assert np.array_equal(BC.kept(p["key_labels"]),
                          ~np.isin(torch.from_numpy(p["key_labels"]).mode(dim=-1).values.numpy(), KC.IGNORE))
    assert int((~BC.kept(p["key_labels"])).sum()) > 0                    # ignored patches are in the fixture


def test_the_float64_ordering_of_the_rounded_operands_is_a_valid_topk_of_the_reference_distances():
    """Conditions (a) and (b) of the maker, recomputed from what the golden stores: enough clear boundaries in every cell, and
    the numpy statement of the engine's rule valid against the reference's bf16 distances with the slack the maker stored
    (L2: 0 steps, cosine: 1)."""
    g, p = _golden()
    keep_all = BC.kept(p["key_labels"])
    for sub in KC.SUBSAMPLINGS:
        keep = keep_all[::sub]
        ref = {d: g[f"ref_{d}_sub{sub}"] for d in KC.DISTANCES}
        counts = BC.clear_counts(ref, keep)
        assert [counts[(d, k)] for k, d in KC.grid()] == g[f"clear_sub{sub}"].tolist()
        if sub == 1:
            print("clear boundaries:", sum(counts.values()), "of", KC.N_QUERIES * len(counts), "smallest cell", min(counts.values()))
            assert BC.condition_a(counts, KC.N_QUERIES)
        lists = BC.f64_lists(p["queries"], p["keys"][::sub], keep, KC.KS[-1])
        for d in KC.DISTANCES:
            slack = BC.slack_steps(ref[d], keep, lists[d])
            print(f"sub {sub} {d}: {slack} bf16 steps")
            assert slack <= int(g[f"slack_{d}"]) <= BC.MAX_SLACK[d]
            # on a clear boundary the set is the reference's: every listed key lies at or below the k-th reference distance
            o = BC.ordinal(ref[d])
            for k in KC.KS:
                kth, clear = BC.boundaries(ref[d], keep)[k]
                assert (np.take_along_axis(o, lists[d][:, :k], 1).max(1)[clear] <= kth[clear]).all()
