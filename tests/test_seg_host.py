"""CPU-only: the host pieces of octic_vits_amd.segmentation against tests/golden/seg_*.npz, which make_seg_golden.py recorded
from the reference's own functions (dinov2/eval/segmentation/eval_segmentation.py, utils.py) with sklearn standing in for
cuML.  Integers must match exactly, metrics to 1e-12.  The L-BFGS driver runs on a float64 numpy objective; its bar is set by
the distance between the two reference solvers (sklearn's lbfgs and scipy's L-BFGS-B on the same problem), see below."""
import ctypes
import os

import numpy as np
import pytest
import torch

import seg_cases as SC
from octic_vits_amd import _lib
from octic_vits_amd import segmentation as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden(name):
    return np.load(os.path.join(GOLDEN, name))


# ------------------------------------------------------------------------------------------------ data handling
def test_patch_labels_equal_the_reference_rearrangement():
    g = golden("seg_data.npz")
    out = S.patch_labels(torch.from_numpy(g["image_labels"]), int(g["patch_size"]))
    assert out.dtype == torch.uint8 and np.array_equal(out.numpy(), g["patch_labels"])
    with pytest.raises(ValueError):
        S.patch_labels(torch.zeros(2, 10, 16, dtype=torch.uint8), 4)


@pytest.mark.parametrize("sub", [1, 3])
def test_fit_targets_keep_the_rows_and_labels_the_reference_passes_on(sub):
    """Sub-sampling, the ignore mask on the patch mode, and the label value <-> class index tables: the rows with a target
    >= 0 and their label values are what Classifier.fit hands to _fit (eval_segmentation.py:78-84, 331)."""
    g = golden("seg_data.npz")
    modes = torch.from_numpy(g["patch_modes"])
    assert 0 in g["patch_modes"] and 255 in g["patch_modes"]            # ties won by ignored values are in the fixture
    clf = S.LogregClassifier(ignore_labels=SC.IGNORE, train_set_subsampling=sub)
    classes, y = clf.targets_from_modes(modes[::sub])
    rows = np.arange(len(g["patch_modes"]))[::sub]
    kept = y.numpy() >= 0
    assert np.array_equal(rows[kept], g[f"fit_rows_sub{sub}"])
    assert np.array_equal(classes.numpy()[y.numpy()[kept]], g[f"fit_labels_sub{sub}"])
    assert np.array_equal(classes.numpy(), np.unique(g[f"fit_labels_sub{sub}"]))           # sklearn's classes_
    assert y.dtype == torch.int32 and int(y.max()) == classes.numel() - 1
    assert not np.array_equal(classes.numpy(), np.arange(classes.numel()))                 # non-contiguous label values


def test_upscale_equals_the_reference():
    g = golden("seg_data.npz")
    clf = S.LogregClassifier(ignore_labels=SC.IGNORE)
    clf.n_pixels_per_sample = g["upscale_out"].shape[1]
    out = clf.upscale(torch.from_numpy(g["upscale_in"]))
    assert out.dtype == torch.uint8 and np.array_equal(out.numpy(), g["upscale_out"])


def test_hyper_parameter_names_grids_and_result_keys():
    g = golden("seg_data.npz")
    clf = S.LogregClassifier(ignore_labels=SC.IGNORE)
    names, grids = zip(*clf.hparam_grids.items())
    import itertools
    ours = [S.hparam_name("mIoU", names, p) for p in itertools.product(*grids)]
    assert ours == list(g["hparam_names_default"])
    custom = S.LogregClassifier(ignore_labels=SC.IGNORE, C=(0.5, 20), max_iter=(100, 300), tol=(1e-6,), linesearch_max_iter=(20,),
                                lbfgs_hessian_rank=(7,))
    names, grids = zip(*custom.hparam_grids.items())
    assert [S.hparam_name("mIoU", names, p) for p in itertools.product(*grids)] == list(g["hparam_names_custom"])
    # the keys of the reference's eval_model on a two-point grid
    two = S.LogregClassifier(ignore_labels=SC.IGNORE, C=(0.01, 1.0))
    names, grids = zip(*two.hparam_grids.items())
    keys = [f"hparam_fitting.logreg.{S.hparam_name('mIoU', names, p)}" for p in itertools.product(*grids)]
    keys += [f"labels_logreg_{m}" for m in S.metrics_dict]
    assert sorted(keys) == list(g["eval_model_keys"])


def test_select_hparams_takes_the_reference_choice_on_known_scores(monkeypatch):
    """select_hparams with fit / predict / metric replaced by the recorded scores: the names, their order and the chosen
    grid point equal the reference's (the first maximum)."""
    g = golden("seg_data.npz")
    scores = iter(g["hparam_scores_default"].tolist())
    clf = S.LogregClassifier(ignore_labels=SC.IGNORE)
    monkeypatch.setattr(clf, "fit", lambda f, l: None)
    monkeypatch.setattr(clf, "predict", lambda f: None)
    monkeypatch.setitem(S.metrics_dict, "mIoU", lambda yt, yp, ign: next(scores))
    metrics = clf.select_hparams(None, None, None, None)
    assert list(metrics) == list(g["hparam_names_default"])
    assert list(metrics.values()) == g["hparam_scores_default"].tolist()
    assert clf.C == float(g["hparam_best_C_default"]) and clf.max_iter == 1000 and clf.lbfgs_hessian_rank == 5
    one = S.LogregClassifier(ignore_labels=SC.IGNORE, C=(2.5,))
    assert one.select_hparams(None, None, None, None) == {} and one.C == 2.5       # a grid of one point is not searched


@pytest.mark.parametrize("case", ["metric0", "metric1", "metric2", "metric_px"])
def test_metrics_from_a_numpy_confusion_matrix(case):
    """accuracy and mIoU (jaccard_score(average="macro"): labels present in the masked truth OR the masked prediction) from
    the confusion counts; the fixture has a class only in the predictions, one only in the truth, ignored 0 and 255."""
    g = golden("seg_data.npz")
    yt, yp = g[f"{case}_true"], g[f"{case}_pred"]
    if yp.ndim == 1:
        yp = np.repeat(yp[:, None], yt.shape[1], 1)
    conf = SC.numpy_confusion(yt, yp, SC.IGNORE)
    assert conf[0].sum() == 0 and conf[255].sum() == 0 and conf.sum() == (~np.isin(yt, SC.IGNORE)).sum()
    assert abs(S.miou_from_confusion(conf) - float(g[f"{case}_mIoU"])) <= 1e-12
    assert abs(S.accuracy_from_confusion(conf) - float(g[f"{case}_acc"])) <= 1e-12
    assert abs(S.miou_from_confusion(torch.from_numpy(conf)) - float(g[f"{case}_mIoU"])) <= 1e-12


# ------------------------------------------------------------------------------------------------ L-BFGS
@pytest.mark.parametrize("i", range(len(SC.CS)))
def test_lbfgs_reaches_the_reference_optimum_on_a_float64_objective(i):
    """J - J* of the driver's solution, J* = the lower of sklearn's and scipy's solutions of the same problem.  The two
    references are only converged to their own tolerances, so the driver may be at most 10x their distance above J*, with a
    floor of 1e-9 |J*|."""
    g = golden("seg_logreg.npz")
    Xtr, _ = SC.logreg_features(g)
    y = g["cls"][:SC.N_TRAIN]
    C = SC.CS[i]
    fun = SC.objective(Xtr, y, C)
    J_sk, J_sp = float(g[f"J_sklearn_{i}"]), float(g[f"J_scipy_{i}"])
    assert abs(fun(SC.pack(g[f"coef_{i}"], g[f"intercept_{i}"]))[0] - J_sk) <= 1e-12 * abs(J_sk)     # the stored problem is this one
    x, f, info = S.lbfgs(fun, np.zeros(SC.K * SC.D + SC.K), memory=5, max_iter=1000, tol=1e-12, linesearch_max_iter=50)
    J_star = min(J_sk, J_sp)
    bar = max(10 * abs(J_sk - J_sp), 1e-9 * abs(J_star))
    print(f"C={C:g}: J - J* = {f - J_star:.3e} (bar {bar:.3e}), {info}")
    assert f == fun(x)[0]
    assert f - J_star <= bar
    assert info["n_iter"] <= 1000 and info["status"] in ("converged", "linesearch", "max_iter")


def test_lbfgs_stopping_rules():
    A = np.diag(np.linspace(1.0, 50.0, 12))
    quad = lambda x: (0.5 * float(x @ A @ x), A @ x)
    x, f, info = S.lbfgs(quad, np.ones(12), memory=5, max_iter=200, tol=1e-10, linesearch_max_iter=20)
    assert info["status"] == "converged" and np.max(np.abs(A @ x)) <= 1e-10 * max(1.0, np.max(np.abs(x)))
    x, f, info = S.lbfgs(quad, np.ones(12), memory=5, max_iter=3, tol=1e-30, linesearch_max_iter=20)
    assert info["status"] == "max_iter" and info["n_iter"] == 3 and f < quad(np.ones(12))[0]
    # an objective with rounding noise far above the decrease still available: the search finds no lower point and the
    # best iterate comes back
    noisy = lambda x: (float(np.float32(0.5 * float(x @ A @ x) + 1e6) - np.float32(1e6)), A @ x)
    x, f, info = S.lbfgs(noisy, np.ones(12), memory=5, max_iter=200, tol=1e-14, linesearch_max_iter=10)
    assert info["status"] == "linesearch" and f <= noisy(np.ones(12))[0]
    x, f, info = S.lbfgs(quad, np.zeros(12))
    assert info == {"n_iter": 0, "n_eval": 1, "status": "converged"}


# ------------------------------------------------------------------------------------------------ ABI
SEG_SYMBOLS = ["octic_seg_ldd", "octic_seg_slabs", "octic_seg_workspace_bytes", "octic_seg_value_dlogits", "octic_seg_predict",
               "octic_seg_wgrad", "octic_seg_colstats_workspace_bytes", "octic_seg_colstats", "octic_seg_standardize",
               "octic_seg_patch_mode", "octic_seg_confusion"]


def test_symbols_are_exported_documented_and_prototyped():
    L = _lib.lib()
    declared = _lib.header_symbols()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    for s in SEG_SYMBOLS:
        assert s in declared and s in _lib._PROTOS and hasattr(L, s) and s in text, s
    assert L.octic_abi_version() == 20
    from octic_vits_amd.build import SOURCES
    assert "segeval.hip" in SOURCES


def test_argument_validation_without_gpu():
    """Unsupported shapes and null pointers return negative codes before any launch (there is no device here)."""
    L = _lib.lib()
    p = ctypes.c_void_p(4096)
    null = ctypes.c_void_p(0)
    assert L.octic_seg_ldd(150) == 160 and L.octic_seg_ldd(2) == 32 and L.octic_seg_ldd(256) == 256
    assert L.octic_seg_ldd(1) == -1 and L.octic_seg_ldd(257) == -1
    assert L.octic_seg_workspace_bytes(1000, 60, 10) == -1 and L.octic_seg_workspace_bytes(0, 64, 10) == -1
    assert L.octic_seg_workspace_bytes(1000, 64, 10) > 0 and L.octic_seg_slabs(1000, 64, 10) >= 1

    def value(C=10, D=64, N=100, X=p, W=p, y=p):
        return L.octic_seg_value_dlogits(X, D, N, D, W, p, C, y, p, p, p, None)

    assert value(C=1) == -1 and value(C=257) == -1 and value(D=60) == -1 and value(N=0) == -1
    assert value(X=null) == -4 and value(W=null) == -4 and value(y=null) == -4
    assert L.octic_seg_value_dlogits(ctypes.c_void_p(4100), 64, 100, 64, p, p, 10, p, p, p, p, None) == -2
    assert L.octic_seg_predict(p, 64, 100, 64, p, p, 1, p, None) == -1
    assert L.octic_seg_predict(p, 64, 100, 60, p, p, 10, p, None) == -1
    assert L.octic_seg_predict(p, 64, 100, 64, p, p, 10, null, None) == -4
    assert L.octic_seg_wgrad(p, 64, 100, 64, p, 257, p, 1.0, 1.0, p, p, p, None) == -1
    assert L.octic_seg_wgrad(p, 64, 100, 64, null, 10, p, 1.0, 1.0, p, p, p, None) == -4
    assert L.octic_seg_wgrad(p, 32, 100, 64, p, 10, p, 1.0, 1.0, p, p, p, None) == -1          # row stride below D
    assert L.octic_seg_colstats(p, 60, 100, 60, p, p, p, None) == -1 and L.octic_seg_colstats(p, 64, 100, 64, null, p, p, None) == -4
    assert L.octic_seg_standardize(p, 64, 0, 64, p, p, None) == -1 and L.octic_seg_standardize(p, 64, 10, 64, null, p, None) == -4
    assert L.octic_seg_patch_mode(null, 1, 10, 16, p, None) == -4 and L.octic_seg_patch_mode(p, 3, 10, 16, p, None) == -3
    assert L.octic_seg_patch_mode(p, 1, 0, 16, p, None) == -1
    assert L.octic_seg_confusion(p, 1, 10, 16, p, null, p, None) == -4 and L.octic_seg_confusion(p, 1, 10, 0, p, p, p, None) == -1


def test_device_pieces_refuse_cpu_tensors():
    X = torch.zeros(8, 64)
    lab = torch.zeros(8, 4, dtype=torch.uint8)
    for call in (lambda: S.Standardizer().fit(X), lambda: S.LogregClassifier((0, 255)).fit(X, lab),
                 lambda: S.mIoU(lab, lab, (0, 255)), lambda: S.accuracy(lab, lab[:, 0], (0, 255)),
                 lambda: S.patch_features(torch.nn.Identity(), torch.zeros(1, 3, 8, 8))):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()
    for kind in ("RobustScaler", "pca", "pca_whiten"):
        with pytest.raises(NotImplementedError):
            S.Standardizer(kind)
    with pytest.raises(NotImplementedError):
        S.eval_model(torch.nn.Linear(2, 2), [], [], classifiers=("logreg", "knn"))
