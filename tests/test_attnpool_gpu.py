"""Attentive-probe evaluation on the GPU (csrc/attnpool.hip, octic_vits_amd/classification.py).

Exactness: operands are small integers, so every float32 sum is exact and the kernels must return the float64 result bit for
bit.  Module level: the project's tolerance rule (tests/test_probe_gpu.py::within) - the engine's max-abs distance to a
float64 run of the stock modules is at most max(2 x the distance of the stock float32 composition on the same GPU and inputs,
1e-6 of the tensor's scale); every check prints both."""
import copy

import pytest
import torch
import torch.nn.functional as F

from octic_vits_amd import classification as CL

pytestmark = pytest.mark.gpu
DEV = "cuda"


def within(what, engine, stock, ref64):
    ref64 = ref64.double()
    d_eng = (engine.double() - ref64).abs().max().item()
    d_stock = (stock.double() - ref64).abs().max().item()
    scale = ref64.abs().max().item()
    bound = max(2.0 * d_stock, 1e-6 * scale)
    print(f"[attnpool-tol] {what}: engine {d_eng:.3e} stock {d_stock:.3e} bound {bound:.3e} scale {scale:.3e}")
    assert d_eng <= bound, (what, d_eng, d_stock, bound)


def ints(seed, *shape, lim=4):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-lim, lim + 1, shape, generator=g).float().to(DEV)


def same(what, got, want64):
    assert got.dtype == torch.float32
    assert torch.equal(got.double(), want64), (what, (got.double() - want64).abs().max().item())


# ------------------------------------------------------------------------------------------------ kernels, exact
# (B, N, D, G, C, ldx): every N edge, B, D, G (GH no multiple of 4 or of a tile) and C of the list, a handful of combinations
COMBOS = [(1, 1, 64, 1, 5, 64), (3, 4, 128, 3, 37, 132), (8, 15, 64, 5, 5, 64), (1, 16, 128, 1, 37, 128), (3, 17, 64, 3, 5, 80),
          (8, 33, 128, 5, 37, 128), (3, 196, 384, 3, 5, 388), (1, 257, 64, 5, 37, 64), (8, 16, 384, 1, 5, 384)]


@pytest.mark.parametrize("B,N,D,G,C,ldx", COMBOS)
def test_gemm_shaped_kernels_are_exact(B, N, D, G, C, ldx):
    from octic_vits_amd import ops
    H = D // 64
    GH = G * H
    GHp = (GH + 3) // 4 * 4
    T = lambda ts: ops.ptr_table(ts, DEV)
    z32 = lambda *s: torch.full(s, 77.0, device=DEV)
    xbuf = ints(1, B * N, ldx, lim=2)
    X2 = xbuf[:, :D]                                                       # row stride ldx >= D
    X3 = X2.as_strided((B, N, D), (N * ldx, ldx, 1))
    X64 = X3.double()
    q, kvw, kvb = ints(2, G, D), ints(3, G, 2 * D, D), ints(4, G, 2 * D)
    wk64, wv64, bv64 = kvw[:, :D].double(), kvw[:, D:].double(), kvb[:, D:].double()

    # fold
    U = z32(GHp, D)
    ops.attnpool_fold(T(list(q)), T([w[:D] for w in kvw]), G, D, U)
    U64 = 0.125 * torch.einsum("ghj,ghjd->ghd", q.double().view(G, H, 64), wk64.view(G, H, 64, D)).reshape(GH, D)
    same("fold", U[:GH], U64)
    assert bool((U[GH:] == 0).all())
    # scores: the existing NT product at this shape (GH padded to a multiple of 4)
    Ui = ints(5, GHp, D, lim=2)
    S = ops.dense_f32_nt(X2, Ui)
    same("scores", S, X2.double() @ Ui.double().T)
    # pooling: Z[b, c, :] = sum_n P[b, n, c] X[b, n, :]
    P = ints(6, B * N, GHp)
    Z = z32(B * GH * D)
    ops.attnpool_pool(P, X3, ldx, B, N, D, GH, Z)
    same("pool", Z.view(B, GH, D), torch.einsum("bnc,bnd->bcd", P.double().view(B, N, GHp)[:, :, :GH], X64))
    # value projection, into columns of a wider row
    Zi = ints(7, B, GH, D)
    row = z32(B, G * D + 8)
    ops.attnpool_value(Zi, T([w[D:] for w in kvw]), T([b[D:] for b in kvb]), B, G, D, row[:, 4:])
    want = torch.einsum("ghjd,bghd->bghj", wv64.view(G, H, 64, D), Zi.double().view(B, G, H, D)).reshape(B, G, D) + bv64[None]
    same("value", row[:, 4:4 + G * D], want.reshape(B, G * D))
    assert bool((row[:, :4] == 77).all() and (row[:, 4 + G * D:] == 77).all())
    # linear layer backward
    dl = ints(8, G, B, C)
    W = ints(9, G, C, D)
    dF = z32(B, G * D)
    ops.attnpool_dinput(dl, T(list(W)), G, B, C, D, 1.0, dF)
    same("dinput", dF, torch.einsum("gbc,gcd->bgd", dl.double(), W.double()).reshape(B, G * D))
    Fr = ints(10, B, G * D)
    dW = z32(G, C, D)
    ops.attnpool_dweight(dl, Fr, 0, D, G, B, C, D, 1.0, T(list(dW)))
    same("dweight", dW, torch.einsum("gbc,bgd->gcd", dl.double(), Fr.double().view(B, G, D)))
    ops.attnpool_dweight(dl, Fr, 0, 0, G, B, C, D, 0.5, T(list(dW)))       # a shared input (the Linear classifiers), alpha
    same("dweight shared", dW, 0.5 * torch.einsum("gbc,bd->gcd", dl.double(), Fr.double()[:, :D]))
    db = z32(G, (C + 3) // 4 * 4)                                          # rows 16-byte aligned, as the grid's flat buffer keeps them
    ops.attnpool_colsum(dl, B * C, C, G, B, C, 1.0, T(list(db)))
    same("colsum", db[:, :C], dl.double().sum(1))
    assert bool((db[:, C:] == 77).all())
    # value projection backward
    dp = ints(11, B, G * D)
    dZ = z32(B * GH * D)
    ops.attnpool_dz(dp, T([w[D:] for w in kvw]), B, G, D, dZ)
    same("dz", dZ.view(B, GH, D), torch.einsum("bghj,ghjd->bghd", dp.double().view(B, G, H, 64), wv64.view(G, H, 64, D)).reshape(B, GH, D))
    dkvw = z32(G, 2 * D, D)
    ops.attnpool_dwv(dp, Zi, B, G, D, T([w[D:] for w in dkvw]))
    same("dwv", dkvw[:, D:], torch.einsum("bghj,bghd->ghjd", dp.double().view(B, G, H, 64), Zi.double().view(B, G, H, D)).reshape(G, D, D))
    assert bool((dkvw[:, :D] == 77).all())
    # softmax backward on integer "probabilities" in {0, 1}: dS = P (dP - sum_n P dP), dP = X dZ^T
    Pb = (ints(12, B * N, GHp, lim=1).abs())
    dZi = ints(13, B, GH, D, lim=2)
    dS = z32(B * N, GHp)
    ops.attnpool_dscores(X3, ldx, dZi, Pb, B, N, D, GH, dS)
    dP64 = torch.einsum("bnd,bcd->bnc", X64, dZi.double())
    P64 = Pb.double().view(B, N, GHp)[:, :, :GH]
    dS64 = (P64 * (dP64 - (P64 * dP64).sum(1, keepdim=True))).float().double()      # the last product rounds once
    same("dscores", dS.view(B, N, GHp)[:, :, :GH], dS64)
    assert bool((dS[:, GH:] == 0).all())
    # dU (the existing TN product) and the unfold
    dSi = ints(14, B * N, GHp, lim=2)
    dU = ops.dense_f32_tn(dSi, X2)
    same("dU", dU, dSi.double().T @ X2.double())
    dUi = ints(15, GHp, D)
    dq, dkb = z32(G, D), z32(G, 2 * D)
    dkvw.fill_(77.0)
    ops.attnpool_unfold(T(list(q)), T([w[:D] for w in kvw]), dUi, G, D, T(list(dq)), T([w[:D] for w in dkvw]), T([b[:D] for b in dkb]))
    dU64 = dUi.double()[:GH].view(G, H, 1, D)
    same("dq", dq, 0.125 * (wk64.view(G, H, 64, D) * dU64).sum(-1).reshape(G, D))
    same("dwk", dkvw[:, :D], (0.125 * q.double().view(G, H, 64, 1) * dU64).reshape(G, D, D))
    assert bool((dkb[:, :D] == 0).all() and (dkb[:, D:] == 77).all() and (dkvw[:, D:] == 77).all())


def test_softmax_kernel():
    from octic_vits_amd import ops
    # N = 1: exactly one
    S = torch.randn(3, 8, device=DEV) * 50
    ops.attnpool_softmax(S, 3, 1, 6)
    assert bool((S[:, :6] == 1).all() and (S[:, 6:] == 0).all())
    # scores spread over +-200: finite, columns sum to one; a column of equal scores: 1 / N
    B, N, GH, ld = 3, 197, 70, 72
    S = (torch.rand(B * N, ld, device=DEV) * 400 - 200)
    S[:, 5] = 123.25
    ref = torch.softmax(S.double().view(B, N, ld), dim=1)
    ops.attnpool_softmax(S, B, N, GH)
    Pr = S.view(B, N, ld)
    assert bool(torch.isfinite(Pr).all())
    assert (Pr[:, :, :GH].double().sum(1) - 1).abs().max().item() <= 1e-6
    assert bool((Pr[:, :, 5] == torch.tensor(1.0 / N, dtype=torch.float32)).all())
    assert bool((Pr[:, :, GH:] == 0).all())
    assert (Pr[:, :, :GH].double() - ref[:, :, :GH]).abs().max().item() <= 1e-6


# ------------------------------------------------------------------------------------------------ module level
def _grid(D, G, C, B, reps=("patch",), model=None, **kw):
    kw.setdefault("n_iters", 8)
    kw.setdefault("warmup_iters", 3)
    return CL.ClassifierGrid(model, representations=reps, learning_rates=tuple(0.05 * (i + 1) for i in range(G)),
                             weight_decays=(0.1,), batch_size=B, num_classes=C, device=DEV,
                             **({} if model is not None else {"embed_dim": D}), **kw)


def _randomise(grid, seed):
    """Weights at a scale where the attention is far from uniform (the initialisation's 0.02 makes every score ~0)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    with torch.no_grad():
        for name, p in grid.classifiers.named_parameters():
            std = 1.0 if name.endswith(("query_token", "kv.bias")) else (0.1 if name.endswith("linear.bias") else p.shape[-1] ** -0.5)
            p.copy_(torch.randn(p.shape, generator=g, device=DEV) * std)


def _feats(grid, B, N, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    out = {}
    for s in grid.sources:
        shape = (B, N, s.K) if s.attn else (B, s.K)
        out[s.name] = torch.randn(shape, generator=g, device=DEV)
    labels = torch.randint(0, grid.num_classes, (B,), generator=g, device=DEV)
    return out, labels


def _stock(grid, feats, labels, dtype):
    """Logits [G, B, C], loss and gradients of the stock modules on a copy of the grid's weights."""
    mods = copy.deepcopy(grid.classifiers).to(dtype)
    for p in mods.parameters():
        p.grad = None
    out = mods({k: v.to(dtype) for k, v in feats.items()})
    pred = torch.stack(list(out.values()), dim=-1)                        # [B, C, G]
    loss = F.cross_entropy(pred, labels[:, None].expand(-1, pred.shape[-1]))
    loss.backward()
    return pred.permute(2, 0, 1).detach(), loss.detach(), {n: p.grad for n, p in mods.named_parameters()}


def _compare_forward_backward(B, N, D, G, C):
    grid = _grid(D, G, C, B)
    _randomise(grid, 1)
    feats, labels = _feats(grid, B, N, 2)
    l32, loss32, g32 = _stock(grid, feats, labels, torch.float32)
    l64, loss64, g64 = _stock(grid, feats, labels, torch.float64)
    logits = grid.forward_features(feats).clone()
    grid.backward(labels)
    torch.cuda.synchronize()
    within("logits", logits, l32, l64)
    within("loss", grid.loss.mean(), loss32, loss64)
    for name, p in grid.classifiers.named_parameters():
        within(f"grad {name}", p.grad, g32[name], g64[name])
        if name.endswith("kv.bias"):
            assert bool((p.grad[:D] == 0).all()), name
    return grid


@pytest.mark.parametrize("B,N,D,G,C", [(8, 33, 128, 3, 10), (3, 196, 384, 5, 37)])
def test_module_forward_backward_against_float64(B, N, D, G, C):
    _compare_forward_backward(B, N, D, G, C)


def test_module_at_a_real_width():
    _compare_forward_backward(8, 256, 1280, 2, 1000)


def test_one_token():
    B, D, G, C = 5, 128, 3, 10
    grid = _grid(D, G, C, B)
    _randomise(grid, 3)
    feats, labels = _feats(grid, B, 1, 4)
    grid.forward_features(feats)
    x = feats["patch"][:, 0]
    for g in range(G):
        m = grid.classifiers[G + g]                                       # the cls_avg_patch classifiers come first
        w, b = m.kv.weight.detach()[D:], m.kv.bias.detach()[D:]
        within(f"pooled {g}", grid.pooled("patch", B)[:, g], F.linear(x, w, b), F.linear(x.double(), w.double(), b.double()))
    grid.backward(labels)
    for g in range(G):
        m = grid.classifiers[G + g]
        assert bool((m.query_token.grad == 0).all() and (m.kv.weight.grad[:D] == 0).all())
        assert bool((m.kv.weight.grad[D:] != 0).any())


def test_batch_independence_and_repeatability():
    B, N, D, G, C = 8, 33, 128, 3, 10
    grid = _grid(D, G, C, B)
    _randomise(grid, 5)
    feats, labels = _feats(grid, B, N, 6)
    grid.forward_features(feats)
    full = grid.pooled("patch", B).clone()
    for b in (0, 5):
        grid.forward_features({k: v[b:b + 1] for k, v in feats.items()})
        assert torch.equal(grid.pooled("patch", 1)[0], full[b])
    other = _grid(D, G, C, B)
    other.load_state_dict(grid.state_dict())
    for gr in (grid, other):
        gr.iteration = 2
        gr.step_features(feats, labels)
    torch.cuda.synchronize()
    assert torch.equal(grid.flat, other.flat) and torch.equal(grid.loss, other.loss)
    assert not torch.equal(grid.flat, torch.zeros_like(grid.flat))


def test_no_stock_kernels_in_the_step(monkeypatch):
    grid = _grid(128, 3, 10, 8)
    feats, labels = _feats(grid, 8, 33, 7)
    before = grid.flat.clone()

    def trap(name):
        def f(*a, **k):
            raise AssertionError(f"{name}: a stock kernel was reached inside ClassifierGrid.step_features")
        return f
    with monkeypatch.context() as m:
        for mod, attr in ((F, "linear"), (torch, "mm"), (torch, "bmm"), (torch, "matmul"), (torch, "addmm"), (F, "softmax"),
                          (F, "scaled_dot_product_attention"), (F, "cross_entropy")):
            m.setattr(mod, attr, trap(attr))
        grid.iteration = 2
        grid.step_features(feats, labels)
        torch.cuda.synchronize()
    assert not torch.equal(before, grid.flat) and bool(torch.isfinite(grid.flat).all())


# ------------------------------------------------------------------------------------------------ with a backbone
def _backbone(registers=0):
    from octic_vits_amd.dinov2_vit import DinoVisionTransformer
    torch.manual_seed(0)
    m = DinoVisionTransformer(img_size=56, patch_size=14, embed_dim=128, depth=2, num_heads=2, num_register_tokens=registers)
    return m.to(DEV).eval().requires_grad_(False)


def _train_grid(model, B):
    return CL.ClassifierGrid(model, representations=("cls", "patch"), learning_rates=(0.05, 0.2), weight_decays=(0.0, 0.1),
                             batch_size=B, num_classes=10, n_iters=8, warmup_iters=3)


def _stock_training(state, keys, hyper, feats, labels, dtype, steps, n_iters=8, warmup=3):
    """The stock modules under torch.optim.AdamW(lr=0, weight_decay=0, betas=(0.9, 0.95)) with the reference's grouping and
    schedule, on fixed features."""
    torch.manual_seed(0)
    mods = CL.AllClassifiers({k: (CL.AttnPoolClassifier if k[0] == "patch" else CL.LinearClassifier)(
        256 if k[0] == "cls_avg_patch" else 128, 10) for k in keys})
    mods.load_state_dict(state)
    mods = mods.to(DEV).to(dtype)
    groups = []
    for i, key in enumerate(keys):
        base_lr, wd = hyper[key]
        for name, p in mods[i].named_parameters():
            groups.append({"params": [p], "base_lr": base_lr, "weight_decay": 0.0 if "bias" in name else wd})
    opt = torch.optim.AdamW(groups, lr=0.0, weight_decay=0.0, betas=(0.9, 0.95))
    sched = CL.lr_schedule(n_iters, warmup)
    fz = {k: v.to(dtype) for k, v in feats.items()}
    for it in range(steps):
        for pg in opt.param_groups:
            pg["lr"] = sched[it] * pg["base_lr"]
        pred = torch.stack(list(mods(fz).values()), dim=-1)
        loss = F.cross_entropy(pred, labels[:, None].expand(-1, pred.shape[-1]))
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    return mods


def test_training_five_steps_capture_and_checkpoints():
    B = 8
    model = _backbone()
    grid = _train_grid(model, B)
    assert len(grid) == 12 and [s.name for s in grid.sources] == ["cls", "cls_avg_patch", "patch"]
    g = torch.Generator(device=DEV).manual_seed(11)
    images = torch.randn(B, 3, 56, 56, generator=g, device=DEV)
    labels = torch.randint(0, 10, (B,), generator=g, device=DEV)
    state0 = {k: v.clone() for k, v in grid.state_dict().items()}
    feats = CL.features(model, images, ("cls", "patch"))
    # load_state_dict of the stock modules' state reproduces their logits
    l32 = torch.stack(list(copy.deepcopy(grid.classifiers)(feats).values()))
    l64 = torch.stack(list(copy.deepcopy(grid.classifiers).double()({k: v.double() for k, v in feats.items()}).values()))
    fresh = _train_grid(model, B)
    fresh.load_state_dict({"module." + k: v for k, v in state0.items()})
    within("logits after load_state_dict", fresh.forward_features(feats), l32.detach(), l64.detach())
    # five steps
    losses = [grid.step(images, labels).mean().item() for _ in range(5)]
    print("[attnpool-train] losses", losses)
    assert losses[4] < losses[1] and grid.iteration == 5
    m32 = _stock_training(state0, grid.keys, grid.hyper, feats, labels, torch.float32, 5)
    m64 = _stock_training(state0, grid.keys, grid.hyper, feats, labels, torch.float64, 5)
    p32, p64 = dict(m32.named_parameters()), dict(m64.named_parameters())
    for name, p in grid.classifiers.named_parameters():
        within(f"trained {name}", p.detach(), p32[name].detach(), p64[name].detach())
    # a captured replay equals the eager step bitwise
    eager, graphed = _train_grid(model, B), _train_grid(model, B)
    for gr in (eager, graphed):
        gr.load_state_dict(state0)
        gr.iteration = 1
    replay = graphed.capture(images, labels)
    for _ in range(2):
        le = eager.step(images, labels).clone()
        lg = replay(images, labels).clone()
        torch.cuda.synchronize()
        assert torch.equal(le, lg)
        assert torch.equal(eager.flat, graphed.flat)
    assert graphed.iteration == 3 and not torch.equal(eager.flat, fresh.flat)


def test_evaluate_keep_best_and_eval_model():
    model = _backbone(registers=4)
    reps = ("cls", "objects", "patch")
    grid = CL.ClassifierGrid(model, representations=reps, learning_rates=(0.05, 0.2), weight_decays=(0.0, 0.1), batch_size=6,
                             num_classes=7, n_iters=4, warmup_iters=2)
    assert [(s.name, s.attn) for s in grid.sources] == [("cls", False), ("cls_avg_patch", False), ("reg", True), ("patch", True)]
    _randomise(grid, 21)
    g = torch.Generator(device=DEV).manual_seed(22)
    batches = []
    for B in (6, 4):
        images = torch.randn(B, 3, 56, 56, generator=g, device=DEV)
        labels = torch.randint(0, 7, (B, 3), generator=g, device=DEV)
        labels[:, 1:][torch.rand(B, 2, generator=g, device=DEV) < 0.5] = -1
        labels[0] = -1                                                    # a row without any valid label is left out
        batches.append((images, labels))
    batches.append((torch.randn(3, 3, 56, 56, generator=g, device=DEV), torch.randint(0, 7, (3,), generator=g, device=DEV)))
    res = grid.evaluate(batches)
    hits, n = torch.zeros(len(grid), device=DEV), 0
    for images, labels in batches:
        feats = CL.features(model, images, reps)
        assert feats["reg"].shape[1] == 4                                 # the pooling also runs at N = 4
        pred = torch.stack([o.argmax(-1) for o in grid.classifiers(feats).values()])      # [G, B]
        t = labels if labels.dim() == 2 else labels[:, None]
        hits += ((pred[:, :, None] == t[None]) & (t >= 0)[None]).any(-1).sum(1)
        n += int((t >= 0).any(-1).sum())
    assert res["samples"] == n == 11
    assert list(res["accuracy"]) == grid.keys
    assert torch.allclose(torch.tensor(list(res["accuracy"].values())), (hits / n).cpu(), atol=1e-6)
    assert set(res["best"]) == {"cls", "cls_avg_patch", "reg", "patch"}
    for source, key in res["best"].items():
        accs = [a for k, a in res["accuracy"].items() if k[0] == source]
        assert res["accuracy"][key] == max(accs) and key == [k for k in grid.keys if k[0] == source][accs.index(max(accs))]
    grid.keep_best(res)
    assert grid.keys == list(res["best"].values()) and len(grid.classifiers) == 4
    again = grid.evaluate(batches)
    assert [again["accuracy"][k] for k in grid.keys] == [res["accuracy"][k] for k in grid.keys]
    single = [(im, lb if lb.dim() == 1 else lb[:, 0].clamp(min=0)) for im, lb in batches]
    out = CL.eval_model(model, single, batches, {"a": batches, "b": batches[:1]}, representations=reps, learning_rates=(0.05, 0.2),
                        weight_decays=(0.0,), batch_size=6, num_classes=7, n_iters=4, warmup_iters=2)
    assert list(out) == [f"{s}_{t}_acc" for t in ("a", "b") for s in ("cls", "cls_avg_patch", "reg", "patch")]
    assert all(0.0 <= v <= 1.0 for v in out.values())
