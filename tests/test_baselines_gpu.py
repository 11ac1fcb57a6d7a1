"""The standard DeiT-III / DINOv2 baselines on the MI355X: the lift GEMM as a Conv2d patch embedding, small models against
the reference goldens (f32), the full-size ViT-H/14 and ViT-L/16 under bf16 autocast, one train step against a plain-torch
restatement, the block stack without library GEMMs / ATen attention / eager norms, captured and graphed forwards, and the
DINOv2 multi-crop pass and SSL step."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import baseline_cases as BC
import cases

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LS = ["deit_tiny_patch16_LS", "deit_small_patch16_LS", "deit_medium_patch16_LS", "deit_base_patch16_LS",
      "deit_large_patch16_LS", "deit_huge_patch14_LS"]


# ------------------------------------------------------------------------------------------------ 1. patch embedding
@pytest.mark.parametrize("p,D", [(14, 1280), (16, 1024)])
def test_lift_patch_embedding_equals_conv2d(p, D):
    """LiftFn with proj.weight viewed as [D, Cin p p] = conv2d + flatten + position + class row (f32): pins the im2col
    column order to Conv2d's (c, kh, kw); K = 588 -> 592 for p = 14."""
    from octic_vits_amd.vit_models import PatchEmbed
    pe = PatchEmbed(img_size=224, patch_size=p, embed_dim=D).cuda()
    cases.fill_parameters(pe, salt=f"pe{p}.")
    x = cases.randn(f"pe{p}.img", 2, 3, 224, 224).cuda()
    n = (224 // p) ** 2
    pos = cases.randn(f"pe{p}.pos", n, D).cuda().requires_grad_(True)
    cls = cases.randn(f"pe{p}.cls", D).cuda().requires_grad_(True)
    got = pe.tokens(x, pos, cls)
    want = torch.cat((cls.expand(2, 1, D), F.conv2d(x, pe.proj.weight, pe.proj.bias, stride=p).flatten(2).transpose(1, 2) + pos),
                     dim=1)
    scale = float(want.detach().abs().max())
    assert got.shape == want.shape == (2, 1 + n, D)
    assert float((got - want).abs().max()) <= 1e-4 * scale
    cot = cases.randn(f"pe{p}.cot", 2, 1 + n, D).cuda()
    g = torch.autograd.grad((got * cot).sum(), [pe.proj.weight, pe.proj.bias, pos, cls])
    w = torch.autograd.grad((want * cot).sum(), [pe.proj.weight, pe.proj.bias, pos, cls])
    for a, b in zip(g, w):
        assert float((a - b).abs().max()) <= 1e-4 * max(1.0, float(b.abs().max()))


# ------------------------------------------------------------------------------------------------ 2. reference goldens
def _check_golden(name, got, tol=1e-3):
    want = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert set(got) == set(want.files)
    for k in want.files:
        if not want[k].size:
            continue
        scale = max(1.0, float(np.abs(want[k]).max()))
        err = float(np.abs(got[k] - want[k]).max())
        assert err <= tol * scale, f"{name}:{k} max err {err:.3e} scale {scale:.3g}"


@pytest.mark.parametrize("name", list(BC.DEIT_CASES))
def test_deit_baseline_f32_forward_matches_the_reference(name):
    from functools import partial
    from octic_vits_amd.vit_models import vit_models
    make = lambda **kw: vit_models(mlp_ratio=4, qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6), **kw)
    _check_golden(name, BC.run_deit_case(make, name, device="cuda"))


@pytest.mark.parametrize("name", list(BC.DINO_CASES))
def test_dino_baseline_f32_forward_matches_the_reference(name):
    """masks, 4 register tokens, a 96 x 96 crop on the 224 model (interpolate_pos_encoding with the 0.1 offset)."""
    from octic_vits_amd.dinov2_vit import DinoVisionTransformer
    _check_golden(name, BC.run_dino_case(lambda **kw: DinoVisionTransformer(**kw), name, device="cuda"))


# ------------------------------------------------------------------------------------------------ 3. full size, bf16
@pytest.mark.timeout(1800)
@pytest.mark.parametrize("name", ["deit_huge_patch14_LS", "deit_large_patch16_LS"])
def test_full_size_bf16_forward_and_gradients_match_f32(name):
    """The rule of tests/test_vith_gpu.py: f32 logits within 1e-3 of scale of the CPU run, bf16-autocast logits within 5e-2,
    sampled parameter gradients within max(3e-2, 2 x the CPU model's own bf16-autocast distance) in relative L2."""
    from octic_vits_amd.deit_models import create_model
    torch.manual_seed(0)
    ref = create_model(name, num_classes=1000)
    cases.fill_parameters(ref, salt="bl.")
    for b in ref.blocks:                              # O(1) layer scales: the branches matter
        b.gamma_1.data.fill_(0.5), b.gamma_2.data.fill_(0.5)
    net = create_model(name, num_classes=1000)
    net.load_state_dict(ref.state_dict())
    net = net.cuda()
    img = cases.randn("bl.img", 2, 3, 224, 224)
    cot = cases.randn("bl.cot", 2, 1000)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    ref.eval(), net.eval()
    with torch.no_grad():
        want = ref(img)
        got = net(img.cuda()).float().cpu()
    scale = max(1.0, float(want.abs().max()))
    assert float((got - want).abs().max()) <= 1e-3 * scale
    names = [n for n, _ in ref.named_parameters()]
    sample = sorted(set(names[::11] + [n for n in names if n.startswith(("pos_embed", "cls_token", "patch_embed", "head",
                                                                           "norm."))]))

    def grads_of(model, x, c, dev=None):
        for p in model.parameters():
            p.grad = None
        if dev is None:
            out = model(x)
        else:
            with torch.autocast(dev, dtype=torch.bfloat16):
                out = model(x)
        (out.float() * c).sum().backward()
        ps = dict(model.named_parameters())
        return out.detach().float().cpu(), {n: ps[n].grad.detach().float().cpu().double().numpy() for n in sample}

    ref.train(), net.train()
    out_ref, g_ref = grads_of(ref, img, cot)
    _, g_yard = grads_of(ref, img, cot, "cpu")
    out_got, g_got = grads_of(net, img.cuda(), cot.cuda(), "cuda")
    assert torch.allclose(out_got, out_ref, rtol=5e-2, atol=5e-2 * scale)
    bad = []
    for n in sample:
        w = g_ref[n]
        den = max(float(np.linalg.norm(w)), 1e-6)
        rel, rel_y = float(np.linalg.norm(g_got[n] - w)) / den, float(np.linalg.norm(g_yard[n] - w)) / den
        if rel > max(3e-2, 2.0 * rel_y):
            bad.append(f"{n}: {rel:.4f} (cpu bf16 {rel_y:.4f})")
    assert not bad, "; ".join(bad[:8])


# ------------------------------------------------------------------------------------------------ 4. train step
def _small_deit(seed=0, **kw):
    from octic_vits_amd.vit_models import vit_models
    from functools import partial
    torch.manual_seed(seed)
    spec = dict(img_size=64, patch_size=16, embed_dim=256, depth=2, num_heads=4, num_classes=10, mlp_ratio=4, qkv_bias=True,
                norm_layer=partial(nn.LayerNorm, eps=1e-6))
    spec.update(kw)
    m = vit_models(**spec)
    cases.fill_parameters(m, salt="tr.")
    return m


def _restated_loss(P, x, y, depth=2, H=4, p=16):
    """deit/vit.py vit_models + Layer_scale_init_Block in plain torch (no engine code), f64 on the CPU."""
    t = F.conv2d(x, P["patch_embed.proj.weight"], P["patch_embed.proj.bias"], stride=p).flatten(2).transpose(1, 2)
    t = t + P["pos_embed"]
    B, N, D = t.shape
    t = torch.cat((P["cls_token"].expand(B, 1, D), t), dim=1)
    for i in range(depth):
        q = f"blocks.{i}."
        h = F.layer_norm(t, (D,), P[q + "norm1.weight"], P[q + "norm1.bias"], 1e-6)
        qkv = (h @ P[q + "attn.qkv.weight"].t() + P[q + "attn.qkv.bias"]).reshape(B, N + 1, 3, H, D // H).permute(2, 0, 3, 1, 4)
        a = torch.softmax((qkv[0] * (D // H) ** -0.5) @ qkv[1].transpose(-2, -1), dim=-1) @ qkv[2]
        a = a.transpose(1, 2).reshape(B, N + 1, D) @ P[q + "attn.proj.weight"].t() + P[q + "attn.proj.bias"]
        t = t + P[q + "gamma_1"] * a
        h = F.layer_norm(t, (D,), P[q + "norm2.weight"], P[q + "norm2.bias"], 1e-6)
        h = F.gelu(h @ P[q + "mlp.fc1.weight"].t() + P[q + "mlp.fc1.bias"]) @ P[q + "mlp.fc2.weight"].t() + P[q + "mlp.fc2.bias"]
        t = t + P[q + "gamma_2"] * h
    t = F.layer_norm(t, (D,), P["norm.weight"], P["norm.bias"], 1e-6)[:, 0]
    return F.binary_cross_entropy_with_logits(t @ P["head.weight"].t() + P["head.bias"], y)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_train_step_matches_a_plain_torch_restatement(mode):
    """Trainer.step (forward + backward + FusedLamb + EMA) against the restated model, oracle/lamb_ref.py's LAMB and EMA in
    f64: loss, gradients, updated parameters and EMA at the tolerances of test_train_gpu.py (f32 1e-3, bf16 3e-2)."""
    from oracle.lamb_ref import LambRef, ema_update, weight_decay_of
    from octic_vits_amd.train import Trainer, synthetic_batch
    tol = 1e-3 if mode == "f32" else 3e-2
    net = _small_deit().cuda()
    tr = Trainer(net, lr=3e-3, weight_decay=0.05, ema_decay=0.9, autocast=(mode == "bf16"), tuned_gemms=False)
    x, y = synthetic_batch(4, 10, "cuda", 5, img_size=64)
    order = tr.optimizer.params
    name_of = {id(p): n for n, p in net.named_parameters()}
    P = {n: p.detach().double().cpu().requires_grad_(True) for n, p in net.named_parameters()}
    loss_ref = _restated_loss(P, x.double().cpu(), y.double().cpu())
    loss_ref.backward()
    net.train()                                       # the step's gradients, by the same engine path (the fused
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=(mode == "bf16")):      # optimizer reuses .grad as scratch)
        out = net(x)
    F.binary_cross_entropy_with_logits(out.float(), y).backward()
    got_grads = {name_of[id(p)]: p.grad.detach().double().cpu().numpy() for p in order}
    for p in order:
        p.grad = None
    loss = float(tr.step(x, y))
    assert abs(loss - float(loss_ref.detach())) <= tol * max(1.0, abs(float(loss_ref.detach())))
    names = [name_of[id(p)] for p in order]
    grads = [P[n].grad.numpy() for n in names]
    for n, g in zip(names, grads):
        assert np.linalg.norm(got_grads[n] - g) <= tol * max(np.linalg.norm(g), 1e-6) + 1e-7, f"grad {n}"
    ref = LambRef([P[n].shape for n in names], weight_decay_of([(n, tuple(P[n].shape)) for n in names], 0.05,
                                                               net.no_weight_decay()), lr=3e-3, eps=1e-8)
    cur = ref.step([P[n].detach().numpy() for n in names], grads)
    ema = ema_update([P[n].detach().numpy() for n in names], cur, 0.9)
    assert abs(float(tr.optimizer.last_grad_norm) - ref.last_grad_norm) <= tol * ref.last_grad_norm
    for n, p, q, e_f, e_r in zip(names, order, cur, tr.optimizer.ema_state(), ema):
        assert np.linalg.norm(p.detach().double().cpu().numpy() - q) <= tol * np.linalg.norm(q) + 1e-6, f"param {n}"
        assert np.linalg.norm(e_f.double().cpu().numpy() - e_r) <= tol * np.linalg.norm(e_r) + 1e-6, f"ema {n}"


# ------------------------------------------------------------------------------------------------ narrow weight gradients
@pytest.mark.parametrize("M,N,K", [(12608, 576, 192), (12608, 192, 768), (12608, 1152, 384), (12608, 384, 1536),
                                   (300, 128, 64), (7, 64, 192)])
def test_dense_wgrad_narrow_shapes(M, N, K):
    """csrc/dense_wgrad.hip's 64 x 64 path (the weight gradients of the D = 192 / 384 blocks): fp64 reference within 2e-4 of
    scale (test_dense_gemm_gpu.py's bound), small-integer operands exact, bitwise repeatable, strided operands."""
    from octic_vits_amd import _lib, ops
    assert ops.dense_wgrad_ok(M, N, K) and int(_lib.lib().octic_dense_wgrad_tile(M, N, K)) == 64
    g = torch.Generator(device="cpu").manual_seed(N + K)
    dy = torch.randn(M, N, generator=g).to("cuda", torch.bfloat16)
    x = torch.randn(M, K + 64, generator=g).to("cuda", torch.bfloat16)[:, 32:32 + K]          # row stride K + 64
    want = dy.double().t() @ x.double()
    got = ops.dense_wgrad_tn(dy, x)
    scale = max(1.0, float(want.abs().max()))
    assert float((got.double() - want).abs().max()) <= 2e-4 * scale
    assert torch.equal(ops.dense_wgrad_tn(dy, x), got)
    di = torch.randint(-3, 4, (M, N), generator=g).to("cuda", torch.bfloat16)
    xi = torch.randint(-3, 4, (M, K), generator=g).to("cuda", torch.bfloat16)
    assert torch.equal(ops.dense_wgrad_tn(di, xi).double(), di.double().t() @ xi.double())


# ------------------------------------------------------------------------------------------------ 5. no library paths
_FORBIDDEN_ATEN = ("mm", "addmm", "bmm", "baddbmm", "matmul", "linear", "native_layer_norm", "native_layer_norm_backward",
                   "gelu", "gelu_backward")


class _AtenLog(torch.utils._python_dispatch.TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.seen = set()

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.seen.add(func.overloadpacket.__name__)
        return func(*args, **(kwargs or {}))


@pytest.mark.parametrize("name", LS)
def test_block_stack_stays_on_hip(name, monkeypatch):
    """bf16 forward + backward of every `_LS` block stack (depth 2) with SDPA, F.linear, torch.mm, torch.bmm and
    F.layer_norm patched to raise, and no ATen GEMM / LayerNorm / GELU / attention op dispatched."""
    from octic_vits_amd.deit_models import create_model
    torch.manual_seed(1)
    net = create_model(name, num_classes=10, drop_path_rate=0.1)
    net.blocks = nn.ModuleList(net.blocks[:2])                    # the factory's dims at a reduced depth
    del net.blocks[-1]._next_norm
    net = net.cuda().train()
    x = torch.randn(2, 3, 224, 224, device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        tok = net.patch_embed.tokens(x, net.pos_embed[0], net.cls_token.flatten())
    cot = torch.randn_like(tok)

    def boom(*a, **k):
        raise AssertionError("a library / ATen path was reached inside the block stack")
    log = _AtenLog()
    with monkeypatch.context() as m:
        for mod, attr in ((F, "scaled_dot_product_attention"), (F, "linear"), (torch, "mm"), (torch, "bmm"),
                          (F, "layer_norm"), (F, "gelu")):
            m.setattr(mod, attr, boom)
        with log, torch.autocast("cuda", dtype=torch.bfloat16):
            t = tok
            for blk in net.blocks:
                t = blk(t)
            (t.float() * cot).sum().backward()
    torch.cuda.synchronize()
    bad = {op for op in log.seen if op in _FORBIDDEN_ATEN or "scaled_dot_product" in op or "flash_attention" in op
           or "efficient_attention" in op}
    assert not bad, sorted(bad)
    assert all(p.grad is not None for p in net.blocks.parameters())


# ------------------------------------------------------------------------------------------------ 6. graphs
def test_captured_step_equals_eager_and_graphed_forward_equals_eager():
    from octic_vits_amd.serve import GraphedForward
    from octic_vits_amd.train import Trainer, synthetic_batch
    ma, mb = _small_deit(drop_path_rate=0.0).cuda(), _small_deit(drop_path_rate=0.0).cuda()
    ta, tb = Trainer(ma, lr=1e-3), Trainer(mb, lr=1e-3)
    batches = [synthetic_batch(8, 10, "cuda", seed=s, img_size=64) for s in range(4)]
    gs = tb.capture(*batches[0], warmup=2)
    for _ in range(2):
        ta.step(*batches[0])
    la, lb = [], []
    for x, y in batches[1:] * 2:
        la.append(float(ta.step(x, y).detach()))
        lb.append(float(gs.replay(x, y)))
    assert la == lb, (la, lb)
    assert len(set(la)) == len(la)
    for (n, pa), pb in zip(ma.named_parameters(), mb.parameters()):
        assert torch.equal(pa, pb), n
    for ea, eb in zip(ta.optimizer.ema_state(), tb.optimizer.ema_state()):
        assert torch.equal(ea, eb)
    x = batches[1][0]
    ma.eval()
    gf = GraphedForward(ma, x)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        want = ma(x)
    assert torch.equal(gf(x), want)


def test_compiled_baseline_equals_eager():
    """torch.compile of a baseline: the patch embedding traces through torch.ops.octic.lift (proj.weight viewed as
    [D, Cin p p]) and the blocks through vit._traced_block; forward and gradients equal the eager engine path within bf16
    tolerance (the rule of test_dispatch_gpu.py::test_whole_model_compiles_and_its_train_step_equals_eager)."""
    import torch._dynamo as dynamo
    from octic_vits_amd import dispatch  # noqa: F401
    net = _small_deit(drop_path_rate=0.0).cuda().train()
    x = torch.randn(4, 3, 64, 64, device="cuda")

    def run(m):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return m(x)

    def grads(m):
        for p in net.parameters():
            p.grad = None
        out = run(m)
        out.float().square().mean().backward()
        return out.detach().float(), {n: p.grad.detach().float().clone() for n, p in net.named_parameters()}

    o1, g1 = grads(net)
    dynamo.reset()
    ex = dynamo.explain(run)(net)
    assert ex.graph_count >= 1
    ops_in_graphs = {str(n.target) for gm in ex.graphs for n in gm.graph.nodes if n.op == "call_function"}
    assert any("octic.lift" in t for t in ops_in_graphs), sorted(ops_in_graphs)[:20]
    assert any("octic.dense_linear" in t or "octic.dense_mlp" in t for t in ops_in_graphs)
    dynamo.reset()
    o2, g2 = grads(torch.compile(net, backend="aot_eager"))
    assert float((o1 - o2).abs().max()) <= 2e-2 * float(o1.abs().max())
    for n in g1:
        assert float((g1[n] - g2[n]).norm()) <= 3e-2 * float(g1[n].norm()) + 1e-9, n


# ------------------------------------------------------------------------------------------------ 7. DINOv2
def _small_dino(seed=0, **kw):
    from octic_vits_amd.dinov2_vit import DinoVisionTransformer
    torch.manual_seed(seed)
    spec = dict(img_size=224, patch_size=16, embed_dim=256, depth=2, num_heads=4, init_values=1e-5, drop_path_rate=0.0,
                drop_path_uniform=True)
    spec.update(kw)
    return DinoVisionTransformer(**spec)


def test_dino_ragged_list_forward_equals_the_per_set_forward():
    from octic_vits_amd import dinov2_models
    m = _small_dino(num_register_tokens=4).cuda().eval()
    cases.fill_parameters(m, salt="rg.")
    g = cases.randn("rg.g", 2, 3, 224, 224).cuda()
    loc = cases.randn("rg.l", 4, 3, 96, 96).cuda()
    masks = (cases.randn("rg.m", 2, 196) > 0.5).cuda()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        got = m.forward_features([g, loc], [masks, None])
        assert m._single_use_pass
        want = [m.forward_features(g, masks), m.forward_features(loc, None)]
        prev, dinov2_models.RAGGED_LISTS = dinov2_models.RAGGED_LISTS, False
        try:
            loop = m.forward_features([g, loc], [masks, None])
            assert not m._single_use_pass
        finally:
            dinov2_models.RAGGED_LISTS = prev
    for a, b, c in zip(got, want, loop):
        for k in ("x_norm_clstoken", "x_norm_regtokens", "x_norm_patchtokens", "x_prenorm"):
            scale = max(1.0, float(b[k].abs().max()))
            assert float((a[k].float() - b[k].float()).abs().max()) <= 2e-2 * scale, k
            assert torch.equal(b[k], c[k]), k


def test_dino_ssl_step_takes_the_ragged_pass_and_matches_f32():
    """One SSLTrainer step (DINO + iBOT + KoLeo, both centerings) on a small DinoVisionTransformer under bf16 autocast on the
    GPU: the single-use ragged pass is taken with no gradient reducer installed (never the reducer / set-by-set combination).
    The yardstick is this package's own f32 CPU run of the same step (torch AdamW, no autocast; the CPU backbone is pinned to
    the reference by the baseline goldens): losses within 3e-2, the parameter update as a whole within 25 % relative L2 -
    AdamW's first update is ~lr * sign(g), and bf16 flips the sign of near-zero gradients, so this bounds the step, not
    each element."""
    import random
    from oracle import ssl_ref as SR
    from octic_vits_amd import ops
    from octic_vits_amd.ssl import SSLMetaArch, SSLTrainer
    kw = dict(head_n_prototypes=256, head_hidden_dim=128, head_bottleneck_dim=64, local_crops_number=2)
    random.seed(11)
    imgs = SR.collate(cases.randn("bl.ssl.g", 4, 3, 224, 224), cases.randn("bl.ssl.l", 4, 3, 96, 96), (0.1, 0.5), 0.5,
                      196, SR.MaskingGenerator((14, 14), max_num_patches=98))
    for centering in ("centering", "sinkhorn_knopp"):
        runs = []
        for dev in ("cuda", "cpu"):
            torch.manual_seed(11)
            arch = SSLMetaArch(lambda: _small_dino(drop_path_rate=0.0), 256, centering=centering, **kw)
            cases.fill_parameters(arch.student, salt="bl.ssl.")
            for k in arch.student:
                arch.teacher[k].load_state_dict(arch.student[k].state_dict())
            arch = arch.to(dev)
            before = {n: p.detach().float().cpu().clone() for n, p in arch.student.backbone.named_parameters()}
            tr = SSLTrainer(arch, lr=1e-3, autocast=(dev == "cuda"), fused_optimizer=(dev == "cuda"))
            bb = arch.student.backbone
            seen_dest = []
            orig = bb.forward_features_list

            def spy(*a, _orig=orig, **k):
                seen_dest.append(ops.GRAD_DEST)
                return _orig(*a, **k)
            bb.forward_features_list = spy
            loss = tr.step({k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in imgs.items()}, teacher_temp=0.07,
                           momentum=0.99)
            if dev == "cuda":
                assert bb._single_use_pass, "the multi-crop step did not take the single-use ragged pass"
                assert seen_dest == [None]
            runs.append(({k: float(v) for k, v in loss.items()},
                         {n: p.detach().float().cpu() - before[n] for n, p in bb.named_parameters()}))
        (lg, dg), (lc, dc) = runs
        for k in lc:
            assert abs(lg[k] - lc[k]) <= 3e-2 * max(1.0, abs(lc[k])), (centering, k, lg[k], lc[k])
        # AdamW's first update is ~lr * sign(g): compare the update as a whole (bf16 flips the sign of near-zero gradients)
        num = sum(float((dg[n] - dc[n]).pow(2).sum()) for n in dc)
        den = sum(float(dc[n].pow(2).sum()) for n in dc)
        assert num ** 0.5 <= 0.25 * den ** 0.5, (centering, (num / den) ** 0.5)


def test_dino_ssl_step_with_batch_subset_stochastic_depth():
    """The recipe's uniform drop path 0.4 (> 0.1: batch-subset stochastic depth on the ragged stream): two SSLTrainer steps
    run on the single-use pass, losses finite, every trained backbone tensor moves."""
    from octic_vits_amd.ssl import SSLMetaArch, SSLTrainer, synthetic_multicrop_batch
    torch.manual_seed(5)
    arch = SSLMetaArch(lambda: _small_dino(drop_path_rate=0.4), 256, head_n_prototypes=256, head_hidden_dim=128,
                       head_bottleneck_dim=64).cuda()
    before = {n: p.detach().clone() for n, p in arch.student.backbone.named_parameters()}
    tr = SSLTrainer(arch, lr=1e-3)
    images = synthetic_multicrop_batch(4, "cuda", seed=5)
    for _ in range(2):
        loss = tr.step(images, teacher_temp=0.04, momentum=0.992)
        assert arch.student.backbone._single_use_pass
        assert all(bool(torch.isfinite(v)) for v in loss.values())
    moved = [n for n, p in arch.student.backbone.named_parameters() if not torch.equal(p, before[n])]
    assert len(moved) >= len(before) - 2, sorted(set(before) - set(moved))      # (mask_token / registers may see none)


def test_dino_set_by_set_pass_is_refused_under_a_gradient_reducer():
    """The reducer hands each weight one destination per pass: a list forward that cannot take the single-row-tensor pass
    (here: f32, no autocast) refuses instead of launching two weight gradients into it."""
    from octic_vits_amd import ops
    m = _small_dino().cuda().train()
    g = torch.randn(2, 3, 224, 224, device="cuda")
    loc = torch.randn(2, 3, 96, 96, device="cuda")

    class _Dest:
        def get(self, ptr):
            return None
    prev, ops.GRAD_DEST = ops.GRAD_DEST, _Dest()
    try:
        with pytest.raises(RuntimeError, match="gradient reducer"):
            m.forward_features([g, loc], [None, None])
    finally:
        ops.GRAD_DEST = prev
