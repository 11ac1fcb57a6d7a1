"""GPU: the linear-probe kernels (csrc/probe.hip) and octic_vits_amd/probe.py against stock torch on the same inputs.

Tolerance rule for every float comparison: the yardstick is the float64 result, the margin is the distance to it of the
stock float32 torch composition on the same GPU and inputs; the engine must be within max(2 x that distance, 1e-6 of the
tensor's scale) (both are float32 sums of the same length in different orders; the floor only keeps an exact-zero yardstick
from making the check vacuous).  Distances are max-abs; every check prints both."""
import os
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from octic_vits_amd import probe

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda"


def within(what, engine, stock, ref64):
    ref64 = ref64.double()
    d_eng = (engine.double() - ref64).abs().max().item()
    d_stock = (stock.double() - ref64).abs().max().item()
    scale = ref64.abs().max().item()
    bound = max(2.0 * d_stock, 1e-6 * scale)
    print(f"[probe-tol] {what}: engine {d_eng:.3e} stock {d_stock:.3e} bound {bound:.3e} scale {scale:.3e}")
    assert d_eng <= bound, (what, d_eng, d_stock, bound)
    return d_eng, d_stock


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _tokens(g, B, T, D, n, dtype, prefix):
    xs = [torch.randn(B, T, D, generator=g, device=DEV).to(dtype) for _ in range(n)]
    return xs, [(x[:, prefix:], x[:, 0]) for x in xs]


def _slices(p):
    return {name: slice(h["col0"], h["col0"] + h["out_dim"]) for name, h in p.heads.items()}


def stock_step(p, F, labels, dtype):
    """The reference's composition with stock torch in `dtype`: per classifier linear -> CrossEntropyLoss -> autograd."""
    out = {}
    for name, sl in _slices(p).items():
        W = p.weights[name].detach().to(dtype).requires_grad_(True)
        b = p.biases[name].detach().to(dtype).requires_grad_(True)
        logits = Fn.linear(F[:, sl].to(dtype), W, b)
        loss = torch.nn.CrossEntropyLoss()(logits, labels)
        loss.backward()
        out[name] = (logits.detach(), loss.detach(), W.grad, b.grad)
    return out


def engine_logits_loss_grad(p, opt, F, labels):
    """Forward, loss, and the gradient through the update kernel's -g mode (mu = 0, lr = 1, W = 0)."""
    B = F.shape[0]
    logits = p.forward_features(F).clone()
    p.loss_and_grad(labels, B, train=True)
    loss = p.loss.clone()
    keep = p.flat.clone()
    p.flat.zero_()
    p.momentum.zero_()
    for g in opt.param_groups:
        g["lr"], g["momentum"] = 1.0, 0.0
    opt.step()
    neg_g = p.flat.clone()
    p.flat.copy_(keep)
    p.momentum.zero_()
    return logits, loss, neg_g


# ------------------------------------------------------------------------------------------------ 1. features
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("T,reg", [(197, 0), (257, 4), (1370, 0), (201, 4)])
def test_feature_kernel_equals_create_linear_input(dtype, T, reg):
    B, D = 5, 128
    _, pairs = _tokens(_gen(T + reg), B, T, D, 4, dtype, 1 + reg)
    p = probe.LinearProbe(None, embed_dim=D, num_classes=10, batch_size=B, device=DEV)
    F = p.features_from_tokens(pairs)
    pairs64 = [(a.double(), c.double()) for a, c in pairs]
    for n, avg, sl in ((1, False, slice(3 * D, 4 * D)), (1, True, slice(3 * D, 5 * D)), (4, False, slice(0, 4 * D)),
                       (4, True, slice(0, 5 * D))):
        want = probe.create_linear_input(pairs, n, avg)
        got = F[:, sl]
        assert got.shape == want.shape
        assert torch.equal(got[:, :n * D], want[:, :n * D]), "class columns are copies: bitwise"
        if avg:
            ref = torch.cat([c for _, c in pairs64[-n:]] + [pairs64[-1][0].mean(dim=1)], dim=-1)
            within(f"features {dtype} T={T} reg={reg} n={n} mean columns", got[:, n * D:], want[:, n * D:], ref[:, n * D:])


# ------------------------------------------------------------------------------------------------ 2. forward, loss, gradient
CASES = {
    "golden_shape": dict(B=16, D=64, C=10, rates=(0.8, 1.6), batch=16, world=1),
    "ragged_c1000_d64": dict(B=80, D=64, C=1000, rates=(0.8, 1.6), batch=128, world=1),
    "ragged_c10_d1280": dict(B=80, D=1280, C=10, rates=(0.8, 1.6), batch=128, world=1),
    "batch_200_c100_d128": dict(B=200, D=128, C=100, rates=(0.8, 1.6), batch=200, world=1),   # several batch chunks per tile
    "full_48": dict(B=128, D=1280, C=1000, rates=probe.DEFAULT_LEARNING_RATES, batch=128, world=1),
    "full_52": dict(B=128, D=1280, C=1000, rates=probe.DEFAULT_LEARNING_RATES, batch=128, world=8),
}


@pytest.mark.parametrize("case", list(CASES))
def test_forward_loss_and_gradient_against_float64(case):
    c = CASES[case]
    g = _gen(7)
    p = probe.LinearProbe(None, embed_dim=c["D"], num_classes=c["C"], batch_size=c["batch"], learning_rates=c["rates"],
                          world_size=c["world"], device=DEV, generator=g)
    if case.startswith("full"):
        assert len(p) == int(case.split("_")[1])
    for name in p.names:                                     # non-zero biases too
        p.biases[name].normal_(0, 0.01, generator=g)
    opt = probe.ProbeSGD(p)
    F = torch.randn(c["B"], p.width, generator=g, device=DEV)
    labels = torch.randint(0, c["C"], (c["B"],), generator=g, device=DEV)
    logits, loss, neg_g = engine_logits_loss_grad(p, opt, F, labels)
    s32 = stock_step(p, F, labels, torch.float32)
    s64 = stock_step(p, F, labels, torch.float64)
    n_w = c["C"] * p.sum_k
    off = 0
    worst = {}
    for i, name in enumerate(p.names):
        K = p.heads[name]["out_dim"]
        gw = -neg_g[off:off + c["C"] * K].view(c["C"], K)
        gb = -neg_g[n_w + i * c["C"]:n_w + (i + 1) * c["C"]]
        off += c["C"] * K
        for what, eng, j in (("logits", logits[i], 0), ("loss", loss[i], 1), ("grad W", gw, 2), ("grad b", gb, 3)):
            d = within(f"{case} {name} {what}", eng, s32[name][j], s64[name][j])
            worst[what] = max(worst.get(what, (0.0, 0.0)), d)
    print(f"[probe-tol] {case} worst (engine, stock) distances: {worst}")


# ------------------------------------------------------------------------------------------------ 3. metrics
def test_topk_counters_equal_torch_topk_on_given_logits():
    NC, B, C = 52, 128, 1000
    g = torch.Generator().manual_seed(11)
    logits = torch.randn(NC * B, C, generator=g)
    top6 = logits.topk(6, dim=1).values
    assert int((top6[:, 1:] == top6[:, :-1]).any(dim=1).sum()) == 0, "ties among the six largest: the tie rule would decide"
    labels = torch.randint(0, C, (B,), generator=g)
    ranks = torch.tensor([1, 2, 5, 6, 1000])[torch.randint(0, 5, (NC * B,), generator=g)]
    order = logits.argsort(dim=1, descending=True)
    rows = torch.arange(NC * B)
    lab_rows = labels.repeat(NC)
    at_rank = order[rows, ranks - 1]                          # swap the label's value with the value of the planted rank
    a, b = logits[rows, lab_rows].clone(), logits[rows, at_rank].clone()
    logits[rows, lab_rows], logits[rows, at_rank] = b, a
    assert torch.equal((logits > logits[rows, lab_rows][:, None]).sum(dim=1) + 1, ranks)
    p = probe.LinearProbe(None, embed_dim=64, num_classes=C, batch_size=B, world_size=8, device=DEV)
    assert len(p) == NC
    lg = logits.view(NC, B, C).to(DEV)
    want1 = torch.zeros(NC, dtype=torch.int64)
    want5 = torch.zeros(NC, dtype=torch.int64)
    p.loss_sum.zero_()
    p.topk.zero_()
    for rows_b in (slice(0, B), slice(0, 80)):                # a full batch, then a ragged one: the counters accumulate
        nb = rows_b.stop
        part = lg[:, rows_b].contiguous()
        p.logits(nb).copy_(part)
        lab = labels[rows_b].to(DEV)
        p.loss_and_grad(lab, nb, train=False)
        tk = part.topk(5, dim=2).indices.cpu()
        hit = tk == labels[rows_b][None, :, None]
        want1 += hit[:, :, 0].sum(dim=1)
        want5 += hit.any(dim=2).sum(dim=1)
    got = p.topk.cpu().long()
    assert torch.equal(got[:, 0], want1) and torch.equal(got[:, 1], want5)
    assert want1.sum() > 0 and (want5 - want1).sum() > 0 and (want5 < B + 80).all()


# ------------------------------------------------------------------------------------------------ 4. golden trajectory
def _stock_modules(p, dtype):
    mods, groups = {}, []
    for name, h in p.heads.items():
        m = torch.nn.Linear(h["out_dim"], p.num_classes).to(DEV, dtype)
        with torch.no_grad():
            m.weight.copy_(p.weights[name])
            m.bias.copy_(p.biases[name])
        mods[name] = m
        groups.append({"params": list(m.parameters()), "lr": h["lr"]})
    return mods, torch.optim.SGD(groups, momentum=0.9, weight_decay=0)


def _stock_iteration(p, mods, opt, F, labels):
    sl = _slices(p)
    ls = {n: torch.nn.CrossEntropyLoss()(m(F[:, sl[n]].to(m.weight.dtype)), labels) for n, m in mods.items()}
    opt.zero_grad()
    sum(ls.values()).backward()
    opt.step()
    return torch.stack([ls[n].detach() for n in p.names])


def test_five_iteration_golden_trajectory():
    g = np.load(os.path.join(GOLDEN, "probe_trajectory.npz"))
    names = list(g["names"])
    B, C, iters = int(g["batch"]), int(g["classes"]), int(g["iters"])
    toks = torch.from_numpy(g["tokens"]).to(DEV)
    labels = torch.from_numpy(g["labels"]).to(DEV)
    pairs = [(x[:, 1:], x[:, 0]) for x in toks]
    p = probe.LinearProbe(None, embed_dim=toks.shape[-1], num_classes=C, batch_size=B, learning_rates=tuple(g["base_rates"]),
                          device=DEV)
    assert p.names == names
    p.load_state_dict({f"classifiers_dict.{n}.linear.{k}": (torch.from_numpy(g[f"w0_{n}"]) if k == "weight" else torch.zeros(C))
                       for n in names for k in ("weight", "bias")})
    F = p.features_from_tokens(pairs).clone()
    mods, sopt = _stock_modules(p, torch.float32)
    opt = probe.ProbeSGD(p, momentum=0.9)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, iters, eta_min=0)
    ssched = torch.optim.lr_scheduler.CosineAnnealingLR(sopt, iters, eta_min=0)
    losses, slosses = [], []
    for it in range(iters):
        assert [gr["lr"] for gr in opt.param_groups] == list(g["lrs"][it])
        losses.append(p.step_features(F, labels).clone())
        sched.step()
        slosses.append(_stock_iteration(p, mods, sopt, F, labels))
        ssched.step()
    within("trajectory losses", torch.stack(losses).cpu(), torch.stack(slosses).cpu(), torch.from_numpy(g["losses"]))
    for n in names:
        m = mods[n]
        for what, eng, stock in (("w", p.weights[n], m.weight), ("b", p.biases[n], m.bias),
                                 ("mw", p.momentum_w[n], sopt.state[m.weight]["momentum_buffer"]),
                                 ("mb", p.momentum_b[n], sopt.state[m.bias]["momentum_buffer"])):
            within(f"trajectory {n} {what}", eng.detach().cpu(), stock.detach().cpu(), torch.from_numpy(g[f"{what}_{n}"]))


# ------------------------------------------------------------------------------------------------ 5. backbones
def _small_hybrid(reg=2):
    from octic_vits_amd import dinov2_models
    torch.manual_seed(3)
    return dinov2_models._dinov2(4, 256, 10, 4, False, reg, dict(img_size=32)).to(DEV).eval()


def _twin(p, model, **kw):
    q = probe.LinearProbe(model, num_classes=p.num_classes, batch_size=p.batch_size, **kw)
    q.load_state_dict(p.state_dict())
    return q


def test_graph_replay_equals_eager_bitwise_and_refuses_stale_inputs():
    model = _small_hybrid()
    g = _gen(5)
    B, C = 8, 10
    a = probe.LinearProbe(model, num_classes=C, batch_size=B, learning_rates=(0.4, 0.8, 1.6), generator=g)
    b = _twin(a, model, learning_rates=(0.4, 0.8, 1.6))
    oa, ob = probe.ProbeSGD(a), probe.ProbeSGD(b)
    sa = torch.optim.lr_scheduler.CosineAnnealingLR(oa, 6, eta_min=0)
    sb = torch.optim.lr_scheduler.CosineAnnealingLR(ob, 6, eta_min=0)
    batches = [(torch.randn(B, 3, 32, 32, generator=g, device=DEV), torch.randint(0, C, (B,), generator=g, device=DEV))
               for _ in range(4)]
    replay = b.capture(*batches[0])
    assert torch.equal(a.flat, b.flat), "capturing must not train"
    for x, y in batches[1:]:
        la = a.step(x, y).clone()
        sa.step()
        lb = replay(x, y).clone()
        sb.step()
        assert torch.equal(la, lb)
        assert torch.equal(a.flat, b.flat) and torch.equal(a.momentum, b.momentum)
    assert len({gr["lr"] for gr in oa.param_groups}) > 1 and oa.param_groups[0]["lr"] != a.heads[a.names[0]]["lr"]
    assert float(a.momentum.abs().max()) > 0
    with pytest.raises(ValueError):
        replay(batches[0][0][:4], batches[0][1][:4])
    with torch.no_grad():
        next(model.parameters()).add_(0.0)
    with pytest.raises(RuntimeError, match="changed since the capture"):
        replay(*batches[1])


def test_state_dict_round_trip_continues_bitwise_and_reference_checkpoint_loads():
    g = _gen(9)
    B, C, D = 16, 10, 64
    a = probe.LinearProbe(None, embed_dim=D, num_classes=C, batch_size=B, learning_rates=(0.8, 1.6), device=DEV, generator=g)
    oa = probe.ProbeSGD(a)
    sa = torch.optim.lr_scheduler.CosineAnnealingLR(oa, 6, eta_min=0)
    F = torch.randn(B, a.width, generator=g, device=DEV)
    labels = torch.randint(0, C, (B,), generator=g, device=DEV)
    for _ in range(2):
        a.step_features(F, labels)
        sa.step()
    b = probe.LinearProbe(None, embed_dim=D, num_classes=C, batch_size=B, learning_rates=(0.8, 1.6), device=DEV)
    ob = probe.ProbeSGD(b)
    sb = torch.optim.lr_scheduler.CosineAnnealingLR(ob, 6, eta_min=0)
    b.load_state_dict({k: v.cpu() for k, v in a.state_dict().items()})
    ob.load_state_dict(oa.state_dict())
    sb.load_state_dict(sa.state_dict())
    for _ in range(3):
        la = a.step_features(F, labels).clone()
        sa.step()
        lb = b.step_features(F, labels).clone()
        sb.step()
        assert torch.equal(la, lb) and torch.equal(a.flat, b.flat) and torch.equal(a.momentum, b.momentum)
    # a checkpoint with the reference's keys, as AllClassifiers(nn.ModuleDict of LinearClassifier).state_dict() writes it
    mods, _ = _stock_modules(a, torch.float32)
    with torch.no_grad():
        for m in mods.values():
            m.weight.normal_(0, 0.02, generator=g)
            m.bias.normal_(0, 0.02, generator=g)
    ckpt = {f"classifiers_dict.{n}.linear.{k}": v for n, m in mods.items() for k, v in m.state_dict().items()}
    b.load_state_dict(ckpt)
    for n, m in mods.items():
        assert torch.equal(b.weights[n], m.weight) and torch.equal(b.biases[n], m.bias)
    assert list(b.state_dict()) == list(ckpt)


def _backbone(kind):
    torch.manual_seed(1)
    if kind == "hybrid_huge_10_blocks":
        from octic_vits_amd import dinov2_models
        return dinov2_models._dinov2(16, 1280, 10, 16, False, 0, {}).to(DEV).eval(), 224
    from octic_vits_amd import dinov2_vit
    return dinov2_vit.DinoVisionTransformer(
        patch_size=16, embed_dim=1024, depth=6, num_heads=16, mlp_ratio=4, num_register_tokens=4, init_values=1.0,
        block_fn=partial(dinov2_vit.Block, attn_class=dinov2_vit.MemEffAttention)).to(DEV).eval(), 224


@pytest.mark.parametrize("kind", ["hybrid_huge_10_blocks", "vit_large_reduced_reg4"])
def test_end_to_end_step_and_evaluate_against_the_stock_composition(kind):
    model, side = _backbone(kind)
    g = _gen(21)
    B, C = 16, 100
    p = probe.LinearProbe(model, num_classes=C, batch_size=B, learning_rates=(0.4, 1.6), generator=g)
    opt = probe.ProbeSGD(p)
    x = torch.randn(B, 3, side, side, generator=g, device=DEV)
    y = torch.randint(0, C, (B,), generator=g, device=DEV)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        pairs = model.get_intermediate_layers(x, 4, return_class_token=True)
    pairs = [(a.clone(), c.clone()) for a, c in pairs]
    Fs = probe.create_linear_input(pairs, 4, True)             # stock features: the widest layout holds the other three
    w0 = {n: (p.weights[n].clone(), p.biases[n].clone()) for n in p.names}
    s32, s64 = stock_step(p, Fs, y, torch.float32), stock_step(p, Fs, y, torch.float64)
    loss = p.step(x, y).clone()
    assert torch.equal(p.features[:B, :4 * p.embed_dim], Fs[:, :4 * p.embed_dim])
    for i, n in enumerate(p.names):
        lr = p.heads[n]["lr"]
        within(f"{kind} {n} loss", loss[i], s32[n][1], s64[n][1])
        for what, eng, k in (("W", p.weights[n], 2), ("b", p.biases[n], 3)):
            w_start = w0[n][0 if k == 2 else 1]
            within(f"{kind} {n} updated {what}", eng, w_start - lr * s32[n][k], w_start.double() - lr * s64[n][k])
    # evaluation: the training batch, a fresh one and a ragged one against top-k on stock logits
    batches = [(x, y)] + [(torch.randn(nb, 3, side, side, generator=g, device=DEV),
                           torch.randint(0, C, (nb,), generator=g, device=DEV)) for nb in (B, 5)]
    res = p.evaluate(batches)
    n_img = sum(b[0].shape[0] for b in batches)
    assert res["samples"] == n_img
    # Yardstick: float64 logits on stock features.  A row counts for certain when its label's logit clears the boundary (the
    # largest / 5th largest of the OTHER logits) by more than TOL, and may go either way inside TOL: f32 logits of scale ~1 lie
    # within 5e-7 of the float64 ones at K = 6400 (measured, NOTES), TOL is 20 x that.  A random backbone gives near-ties.
    TOL = 1e-5
    lo1, hi1, lo5, hi5 = ({n: 0 for n in p.names} for _ in range(4))
    sl = _slices(p)
    for xb, yb in batches:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            pr = model.get_intermediate_layers(xb, 4, return_class_token=True)
        Fb = probe.create_linear_input(pr, 4, True)
        for n in p.names:
            lg = Fn.linear(Fb[:, sl[n]].double(), p.weights[n].double(), p.biases[n].double())
            lab = lg.gather(1, yb[:, None])[:, 0]
            others = lg.scatter(1, yb[:, None], float("-inf")).topk(5, dim=1).values
            m1, m5 = lab - others[:, 0], lab - others[:, 4]
            lo1[n] += int((m1 > TOL).sum())
            hi1[n] += int((m1 > -TOL).sum())
            lo5[n] += int((m5 > TOL).sum())
            hi5[n] += int((m5 > -TOL).sum())
    print(f"[probe-tol] {kind} evaluate: rows inside the tie margin, top-1 {sum(hi1.values()) - sum(lo1.values())}, "
          f"top-5 {sum(hi5.values()) - sum(lo5.values())} of {n_img * len(p)}; certain top-1 hits {sum(lo1.values())}")
    assert sum(lo1.values()) > 0, "the trained batch must give some certain hits"
    for n in p.names:
        got1, got5 = round(res["classifiers"][n]["top-1"] * n_img), round(res["classifiers"][n]["top-5"] * n_img)
        assert lo1[n] <= got1 <= hi1[n], (n, got1, lo1[n], hi1[n])
        assert lo5[n] <= got5 <= hi5[n], (n, got5, lo5[n], hi5[n])
    want1 = {n: res["classifiers"][n]["top-1"] * n_img for n in p.names}
    best, acc = "", 0
    for n in p.names:
        if want1[n] / n_img > acc:
            best, acc = n, want1[n] / n_img
    assert res["best_classifier"] == {"name": best, "accuracy": acc}
