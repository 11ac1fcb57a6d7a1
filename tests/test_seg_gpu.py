"""csrc/segeval.hip and octic_vits_amd.segmentation on the GPU.

Yardstick for the value / gradient kernels (the rule of test_ssl_loss_gpu.py): the reference is the float64 torch
composition on the device; the kernel's maximum error, normalised by the largest float64 magnitude of that quantity, may
be at most 2x the error of the stock f32 torch composition (F.linear, F.cross_entropy, the two explicit gradient products) on
the same inputs, plus one f32 ulp (2^-23).  The solver, prediction, selection and standardisation bars are those of the
goldens (tests/golden/make_seg_golden.py); no test here reads the reference or imports sklearn."""
import os
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import seg_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ULP = 2.0 ** -23


def golden(name):
    return np.load(os.path.join(GOLDEN, name))


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def within(what, got, stock, ref):
    """max |got - ref| / max |ref|  <=  2 max |stock - ref| / max |ref| + one f32 ulp; prints the three figures first."""
    ref = ref.double()
    scale = float(ref.abs().max())
    err = float((got.double() - ref).abs().max()) / scale
    stock_err = float((stock.double() - ref).abs().max()) / scale
    print(f"{what}: kernel {err:.3e}  stock f32 {stock_err:.3e}  bar {2 * stock_err + ULP:.3e}")
    assert err <= 2 * stock_err + ULP, (what, err, stock_err)


def problem(N, D, C, seed, absent=True):
    g = _gen(seed)
    X = torch.randn(N, D, generator=g, device=DEV)
    W = torch.randn(C, D, generator=g, device=DEV) * 0.05
    b = torch.randn(C, generator=g, device=DEV) * 0.1
    y = torch.randint(0, C, (N,), generator=g, device=DEV)
    if absent:                                           # class 1 never occurs
        y[y == 1] = 0
    return X, W, b, y.to(torch.int32)


def evaluate(X, W, b, y, scale=1.0, lam=0.0):
    from octic_vits_amd import ops
    N, D = X.shape
    C = W.shape[0]
    dl = torch.empty(N, ops.seg_ldd(C), dtype=torch.float32, device=DEV)
    ws = ops.seg_workspace(N, D, C, DEV)
    value = torch.empty(1, dtype=torch.float64, device=DEV)
    dW, db = torch.empty_like(W), torch.empty_like(b)
    ops.seg_value_dlogits(X, W, b, y, dl, value, ws)
    ops.seg_wgrad(X, dl, W, scale, lam, dW, db, ws)
    return value, dl, dW, db


def composition(X, W, b, y, dtype, scale=1.0, lam=0.0):
    """The stock torch composition in ``dtype``: value, dlogits, dW, db."""
    X, W, b = X.to(dtype), W.to(dtype), b.to(dtype)
    logits = F.linear(X, W, b)
    value = F.cross_entropy(logits, y.long(), reduction="sum")
    dl = F.softmax(logits, dim=-1)
    dl[torch.arange(X.shape[0], device=X.device), y.long()] -= 1
    return value, dl, scale * (dl.T @ X) + lam * W, scale * dl.sum(0)


def check(tag, X, W, b, y, scale=1.0, lam=0.0):
    C = W.shape[0]
    value, dl, dW, db = evaluate(X, W, b, y, scale, lam)
    s32, s64 = composition(X, W, b, y, torch.float32, scale, lam), composition(X, W, b, y, torch.float64, scale, lam)
    assert float(dl[:, C:].abs().max()) == 0.0 if dl.shape[1] > C else True        # the padded classes are written as zero
    within(f"{tag} value", value[0], s32[0], s64[0])
    within(f"{tag} dlogits", dl[:, :C], s32[1], s64[1])
    within(f"{tag} dW", dW, s32[2], s64[2])
    within(f"{tag} db", db, s32[3], s64[3])


RAGGED = [(1, 64, 2), (1, 1024, 21), (127, 384, 21), (127, 1280, 2), (4099, 1024, 150), (4099, 64, 256), (50000, 384, 150),
          (50000, 1280, 256), (50000, 1280, 150), (4099, 1280, 21)]


@pytest.mark.parametrize("N,D,C", RAGGED)
def test_value_dlogits_and_gradient_against_float64(N, D, C):
    check(f"N={N} D={D} C={C}", *problem(N, D, C, N + D + C))


def test_scale_and_regulariser_enter_the_gradient():
    X, W, b, y = problem(4099, 384, 150, 5)
    check("C_reg=100, lambda=1", X, W, b, y, scale=100.0, lam=1.0)


def test_rows_with_a_target_outside_the_classes_contribute_nothing():
    X, W, b, y = problem(1000, 128, 21, 6)
    y2 = y.clone()
    y2[::3] = -1
    value, dl, dW, db = evaluate(X, W, b, y2)
    keep = y2 >= 0
    v2, dl2, dW2, db2 = evaluate(X[keep].contiguous(), W, b, y2[keep].contiguous())
    assert float(dl[~keep].abs().max()) == 0.0 and torch.equal(dl[keep], dl2)
    assert abs(float(value) - float(v2)) <= 1e-12 * abs(float(v2))
    assert float((dW - dW2).abs().max()) <= 1e-4 * float(dW2.abs().max())           # other slab boundaries: not bitwise
    # a strided (sub-sampled) view is read in place
    v3, dl3, dW3, db3 = evaluate(X[::2], W, b, y[::2].contiguous())
    v4, dl4, dW4, db4 = evaluate(X[::2].contiguous(), W, b, y[::2].contiguous())
    assert torch.equal(dl3, dl4) and torch.equal(dW3, dW4) and torch.equal(db3, db4) and torch.equal(v3, v4)


def test_full_size_case():
    check("N=392000 D=1280 C=150", *problem(392000, 1280, 150, 7))


def test_offsets_beyond_two_to_the_31():
    """N D = 2.18e9 > 2^31 (8.7 GB of features, generated on the device): dlogits on a strided row sample that includes the
    last rows, the gradient against float64 accumulated in chunks.  The stock arm is the f32 composition on the whole matrix."""
    N, D, C = 1_700_000, 1280, 150
    assert N * D > 2 ** 31
    X, W, b, y = problem(N, D, C, 8)
    value, dl, dW, db = evaluate(X, W, b, y)
    v32, dl32, dW32, db32 = composition(X, W, b, y, torch.float32)
    sample = torch.cat([torch.arange(0, N, 1009, device=DEV), torch.arange(N - 64, N, device=DEV)])
    ref_dl = composition(X[sample], W, b, y[sample], torch.float64)[1]
    within("2^31 dlogits (row sample)", dl[sample][:, :C], dl32[sample], ref_dl)
    del dl32
    v64 = torch.zeros((), dtype=torch.float64, device=DEV)
    dW64 = torch.zeros(C, D, dtype=torch.float64, device=DEV)
    db64 = torch.zeros(C, dtype=torch.float64, device=DEV)
    for i in range(0, N, 100_000):
        v, _, gw, gb = composition(X[i:i + 100_000], W, b, y[i:i + 100_000], torch.float64)
        v64 += v
        dW64 += gw
        db64 += gb
    within("2^31 value", value[0], v32, v64)
    within("2^31 dW", dW, dW32, dW64)
    within("2^31 db", db, db32, db64)


def test_two_evaluations_are_bitwise_equal():
    X, W, b, y = problem(50000, 1280, 150, 9)
    a, c = evaluate(X, W, b, y, 3.0, 1.0), evaluate(X, W, b, y, 3.0, 1.0)
    for u, v in zip(a, c):
        assert torch.equal(u, v)


@pytest.mark.parametrize("N,D,C", [(1, 64, 2), (4099, 384, 21), (50000, 1280, 150), (4099, 1024, 256)])
def test_predict_is_the_row_argmax(N, D, C):
    from octic_vits_amd import ops
    X, W, b, _ = problem(N, D, C, 10 + C)
    pred = torch.empty(N, dtype=torch.int32, device=DEV)
    ops.seg_predict(X, W, b, pred)
    logits = F.linear(X.double(), W.double(), b.double())
    want = logits.argmax(-1)
    # a row may differ only where the two best float64 logits are closer than the f32 rounding of the product
    diff = pred.long() != want
    top2 = logits.topk(2, dim=-1).values
    assert int(pred.min()) >= 0 and int(pred.max()) < C
    assert bool(((top2[:, 0] - top2[:, 1])[diff] <= 1e-4).all()) and int(diff.sum()) <= max(1, N // 1000)


# ------------------------------------------------------------------------------------------------ solver
def _logreg_fixture():
    g = golden("seg_logreg.npz")
    Xtr, Xh = SC.logreg_features(g)
    y = g["cls"][:SC.N_TRAIN]
    labels = torch.from_numpy(SC.LABEL_VALUES[y])[:, None].expand(-1, SC.PIXELS).contiguous()
    return g, Xtr, Xh, y, labels


@pytest.mark.parametrize("i", range(len(SC.CS)))
def test_fit_reaches_the_optimum_an_f32_objective_allows_and_predicts_as_sklearn(i):
    """gap = J64(W) - J* in float64 on the host; gap_hip <= 2 gap_f32cpu + 1e-7 |J*|, gap_f32cpu being what the same driver
    reaches with a numpy f32 objective (stored by the maker).  Held-out predictions: at most 0.5 % of the rows differ from
    sklearn's (the maker asserts that the f32 CPU run differs on none)."""
    from octic_vits_amd import segmentation as S
    g, Xtr, Xh, y, labels = _logreg_fixture()
    C = SC.CS[i]
    clf = S.LogregClassifier(ignore_labels=SC.IGNORE)
    clf.C = C
    clf.fit(torch.from_numpy(Xtr).to(DEV), labels.to(DEV))
    assert np.array_equal(clf.classes_.cpu().numpy(), SC.LABEL_VALUES)
    x = SC.pack(clf.coef_.cpu().numpy(), clf.intercept_.cpu().numpy())
    J_star = min(float(g[f"J_sklearn_{i}"]), float(g[f"J_scipy_{i}"]))
    gap = SC.objective(Xtr, y, C)(x)[0] - J_star
    bar = 2 * float(g[f"gap_f32cpu_{i}"]) + 1e-7 * abs(J_star)
    print(f"C={C:g}: gap_hip {gap:.3e} ({gap / abs(J_star):.2e} rel)  gap_f32cpu {float(g[f'gap_f32cpu_{i}']):.3e}  bar {bar:.3e}  "
          f"{clf.solver_info_}")
    assert gap <= bar
    pred = clf.predict(torch.from_numpy(Xh).to(DEV))
    assert pred.shape == (SC.N_HELD, SC.PIXELS) and pred.dtype == torch.uint8
    mism = int((pred[:, 0].cpu().numpy() != g[f"pred_held_{i}"]).sum())
    print(f"C={C:g}: {mism} of {SC.N_HELD} held-out rows differ from sklearn")
    assert mism <= 0.005 * SC.N_HELD


def test_select_hparams_takes_the_golden_choice():
    from octic_vits_amd import segmentation as S
    g, Xtr, Xh, _, _ = _logreg_fixture()
    clf = S.LogregClassifier(ignore_labels=SC.IGNORE, C=SC.CS)
    metrics = clf.select_hparams(torch.from_numpy(Xtr[:SC.N_SELECT]).to(DEV), torch.from_numpy(g["select_labels_train"]).to(DEV),
                                 torch.from_numpy(Xh).to(DEV), torch.from_numpy(g["select_labels_val"]).to(DEV))
    print({k: round(v, 4) for k, v in metrics.items()}, "golden", g["select_scores"])
    assert list(metrics) == list(g["select_names"])
    assert clf.C == float(g["select_best_C"])
    assert not hasattr(clf, "coef_")                     # unfit after the search, as the reference


def test_subsampled_fit_reads_a_row_stride():
    from octic_vits_amd import segmentation as S
    g, Xtr, Xh, y, labels = _logreg_fixture()
    X = torch.from_numpy(Xtr).to(DEV)
    a = S.LogregClassifier(ignore_labels=SC.IGNORE, train_set_subsampling=3, max_iter=(40,))
    a.C = 1.0
    a.fit(X, labels.to(DEV))
    b = S.LogregClassifier(ignore_labels=SC.IGNORE, max_iter=(40,))
    b.C = 1.0
    b.fit(X[::3].contiguous(), labels[::3].contiguous().to(DEV))
    assert a.n_fit_rows_ == b.n_fit_rows_ == len(range(0, SC.N_TRAIN, 3))
    assert torch.equal(a.coef_, b.coef_) and torch.equal(a.intercept_, b.intercept_)


# ------------------------------------------------------------------------------------------------ standardisation
def test_standardizer_against_sklearn():
    """mean_ / scale_ within 1e-10 x the column RMS (f64 accumulation over <= 1e5 rows bounds the reordering error near 1e-11);
    the transformed f32 rows within 2x the distance between numpy's f32 restatement and sklearn's output, plus one ulp."""
    from octic_vits_amd import segmentation as S
    g = golden("seg_standardize.npz")
    raw = torch.from_numpy(g["raw"]).to(DEV)
    rms = np.sqrt((g["raw"].astype(np.float64) ** 2).mean(0))
    st = S.Standardizer("StandardScaler").fit(raw)
    print("mean err / rms", float(np.abs(st.mean_.cpu().numpy() - g["mean"]).max() / rms.max()),
          "scale err", float(np.abs(st.scale_.cpu().numpy() - g["scale"]).max()), "restatement distance", float(g["restatement_distance"]))
    assert np.all(np.abs(st.mean_.cpu().numpy() - g["mean"]) <= 1e-10 * rms)
    assert np.all(np.abs(st.scale_.cpu().numpy() - g["scale"]) <= 1e-10 * rms)
    assert float(st.scale_[9]) == 1.0                    # the constant column
    X = raw.clone()
    out = st.transform(X)
    assert out.data_ptr() == X.data_ptr()                # in place
    want = g["transformed"].astype(np.float64)
    err = np.abs(out.cpu().numpy().astype(np.float64) - want)
    assert np.all(err <= 2 * float(g["restatement_distance"]) + ULP * np.maximum(1.0, np.abs(want)))
    # the other two kinds: two f32 roundings against the reference's one (center_div is float64 there)
    c = S.Standardizer("center").fit(raw)
    assert np.all(np.abs(c.mean_.cpu().numpy() - g["center_mean"]) <= 1e-10 * rms) and float(c.scale_.min()) == 1.0
    got = c.transform(raw.clone())[:32].cpu().numpy().astype(np.float64)
    assert np.all(np.abs(got - g["center_head"]) <= ULP * np.maximum(1.0, np.abs(g["center_head"])))
    cd = S.Standardizer("center_div").fit(raw)
    assert abs(float(cd.scale_[0]) - (float(g["center_div_std"]) + 1e-8)) <= 1e-10 * float(g["center_div_std"])
    got = cd.transform(raw.clone())[:32].cpu().numpy().astype(np.float64)
    assert np.all(np.abs(got - g["center_div_head"]) <= ULP * np.maximum(1.0, np.abs(g["center_div_head"])))


def test_column_statistics_on_many_rows_and_a_row_stride():
    from octic_vits_amd import ops
    g = _gen(12)
    X = torch.randn(100_003, 384, generator=g, device=DEV) * 3 + torch.linspace(-50, 50, 384, device=DEV)
    for view in (X, X[::2], X[:1], X[:63]):
        mean, var = ops.seg_colstats(view)
        m64 = view.double().mean(0)
        v64 = view.double().var(0, unbiased=False)
        rms = (view.double() ** 2).mean(0).sqrt()
        assert bool(((mean - m64).abs() <= 1e-10 * rms).all()) and bool(((var - v64).abs() <= 1e-10 * rms * rms).all())


# ------------------------------------------------------------------------------------------------ labels
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16, torch.int32, torch.int64])
@pytest.mark.parametrize("L", [1, 16, 196, 256])
def test_patch_mode_equals_torch_mode(dtype, L):
    from octic_vits_amd import ops
    g = torch.Generator().manual_seed(L)
    values = torch.tensor([0, 255, 3, 7, 12, 40, 41, 100, 200])
    R = 5001
    lab = values[torch.randint(0, 9, (R, L), generator=g)]
    lab[::5] = values[torch.randint(0, 2, (len(range(0, R, 5)), L), generator=g) * 3]          # two values only: many exact ties
    lab = lab.to(dtype)
    got = ops.seg_patch_mode(lab.to(DEV))
    assert got.dtype == torch.int32 and torch.equal(got.cpu().long(), lab.long().mode(dim=-1).values)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64])
def test_confusion_counts_equal_numpy_bincount(dtype):
    from octic_vits_amd import segmentation as S
    rng = np.random.RandomState(3)
    values = np.asarray([0, 255, 3, 7, 12, 40, 41, 100, 200])
    yt = values[rng.randint(0, 9, size=(7001, 196))]
    yp = values[rng.randint(0, 9, size=7001)]
    t, p = torch.from_numpy(yt).to(dtype).to(DEV), torch.from_numpy(yp).to(dtype).to(DEV)
    want = SC.numpy_confusion(yt, np.repeat(yp[:, None], 196, 1), SC.IGNORE)
    for pred in (p, p[:, None].expand(-1, 196)):
        conf = S.confusion_matrix(t, pred, SC.IGNORE)
        assert conf.dtype == torch.int64 and np.array_equal(conf.cpu().numpy(), want)
    px = torch.from_numpy(values[rng.randint(0, 9, size=(300, 16))]).to(dtype).to(DEV)       # per-pixel predictions
    want = SC.numpy_confusion(yt[:300, :16], px.cpu().numpy(), SC.IGNORE)
    assert np.array_equal(S.confusion_matrix(t[:300, :16].contiguous(), px, SC.IGNORE).cpu().numpy(), want)
    assert np.array_equal(S.confusion_matrix(t, p, ()).cpu().numpy(), SC.numpy_confusion(yt, np.repeat(yp[:, None], 196, 1), ()))


@pytest.mark.parametrize("case", ["metric0", "metric1", "metric2", "metric_px"])
def test_device_metrics_equal_the_reference(case):
    from octic_vits_amd import segmentation as S
    g = golden("seg_data.npz")
    yt, yp = torch.from_numpy(g[f"{case}_true"]).to(DEV), torch.from_numpy(g[f"{case}_pred"]).to(DEV)
    if yp.dim() == 1:
        yp = yp[:, None].expand(-1, yt.shape[1])
    assert abs(S.mIoU(yt, yp, SC.IGNORE) - float(g[f"{case}_mIoU"])) <= 1e-12
    assert abs(S.accuracy(yt, yp, SC.IGNORE) - float(g[f"{case}_acc"])) <= 1e-12


# ------------------------------------------------------------------------------------------------ backbones
def _model(kind):
    torch.manual_seed(4)
    if kind == "baseline_reg4":
        from octic_vits_amd import dinov2_vit
        return dinov2_vit.DinoVisionTransformer(
            patch_size=16, embed_dim=1024, depth=4, num_heads=16, mlp_ratio=4, num_register_tokens=4, init_values=1.0,
            block_fn=partial(dinov2_vit.Block, attn_class=dinov2_vit.MemEffAttention)).to(DEV).eval(), 224
    from octic_vits_amd import dinov2_models
    return dinov2_models._dinov2(4, 256, 10, 4, kind == "invariant", 2 if kind == "hybrid_reg2" else 0,
                                 dict(img_size=32)).to(DEV).eval(), 32


@pytest.mark.parametrize("kind", ["hybrid_reg2", "invariant", "baseline_reg4"])
def test_patch_features_equal_the_sliced_intermediate_layer_and_land_in_place(kind):
    from octic_vits_amd import segmentation as S
    model, side = _model(kind)
    x = torch.randn(3, 3, side, side, generator=_gen(13), device=DEV)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        tokens = model.get_intermediate_layers(x, n=1, norm=True)[0]
    ps = S._patch_size(model)
    ih = side // ps
    D = model.embed_dim
    want = tokens.float().reshape(3, ih, ih, D)
    fm = S.patch_features(model, x)
    assert fm.dtype == torch.float32 and fm.shape == (3, ih, ih, D) and torch.equal(fm, want)
    P = ih * ih
    out = torch.full((5 * P + 7, D), -3.0, device=DEV)
    view = S.patch_features(model, x, out=out, row0=P + 7)
    assert view.data_ptr() == out[P + 7:].data_ptr() and torch.equal(view, want)
    assert torch.equal(out[P + 7:4 * P + 7], want.reshape(3 * P, D))
    assert float(out[:P + 7].max()) == -3.0 == float(out[:P + 7].min()) and float(out[4 * P + 7:].max()) == -3.0
    with pytest.raises(ValueError):
        S.patch_features(model, x, out=out, row0=3 * P)


def test_eval_model_end_to_end(monkeypatch):
    """A 10-block hybrid ViT-H (D = 1280) on synthetic batches with 150 label values: result keys, the refit on train + val, the
    k-NN refusal, and the peak allocation of a fit above its feature matrix: below half the matrix (dlogits is 160 / 1280
    of it, the slab workspace at most a quarter)."""
    from octic_vits_amd import dinov2_models
    from octic_vits_amd import segmentation as S
    torch.manual_seed(1)
    model = dinov2_models._dinov2(16, 1280, 10, 16, False, 0, {}).to(DEV).eval()
    g = torch.Generator().manual_seed(14)
    P = 196

    def batches(n_img, bs):
        out = []
        for i in range(0, n_img, bs):
            n = min(bs, n_img - i)
            lab = torch.randint(1, 151, (n, 14, 14), generator=g).to(torch.uint8)
            lab[torch.rand(n, 14, 14, generator=g) < 0.05] = 255
            lab[torch.rand(n, 14, 14, generator=g) < 0.05] = 0
            out.append((torch.randn(n, 3, 224, 224, generator=g), lab.repeat_interleave(16, 1).repeat_interleave(16, 2)))
        return out

    train, test = batches(50, 8), batches(10, 4)
    fits = []
    orig = S.LogregClassifier.fit

    def spy(self, features, labels):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        orig(self, features, labels)
        torch.cuda.synchronize()
        fits.append((features.shape[0], len(self.classes_), torch.cuda.max_memory_allocated() - base,
                     features.numel() * 4, features.data_ptr()))

    monkeypatch.setattr(S.LogregClassifier, "fit", spy)
    kw = {"logreg": {"C": (0.01, 1.0), "max_iter": (25,)}}
    res = S.eval_model(model, train, test, classifiers=("logreg",), classifiers_kwargs=kw, val_seed=3)
    names = ["hparam_fitting.logreg.mIoU_C=0.01_max_iter=25_tol=1e-12_linesearch_max_iter=50_lbfgs_hessian_rank=5",
             "hparam_fitting.logreg.mIoU_C=1.0_max_iter=25_tol=1e-12_linesearch_max_iter=50_lbfgs_hessian_rank=5",
             "labels_logreg_mIoU", "labels_logreg_acc"]
    assert list(res) == names and all(isinstance(v, float) and 0.0 <= v <= 1.0 for v in res.values())
    # two grid fits on the 45 training images, then the refit on all 50 (validation rows first in the same matrix)
    assert [f[0] for f in fits] == [45 * P, 45 * P, 50 * P]
    assert fits[2][4] + 5 * P * 1280 * 4 == fits[0][4]
    for rows, classes, peak, xbytes, _ in fits:
        print(f"fit on {rows} rows, {classes} classes: peak {peak / 2 ** 20:.1f} MiB above X of {xbytes / 2 ** 20:.1f} MiB")
        assert classes == 150 and peak < 0.5 * xbytes
    # an explicit validation split gives the same layout; k-NN is refused before any work
    res2 = S.eval_model(model, train[:4], test, val=train[4:], classifiers_kwargs=kw, standardization="center")
    assert list(res2) == names
    with pytest.raises(NotImplementedError):
        S.eval_model(model, train, test, classifiers=("knn",))
    with pytest.raises(NotImplementedError):
        S.eval_model(model, train, test, standardization="pca")
