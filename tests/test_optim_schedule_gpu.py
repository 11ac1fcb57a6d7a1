"""GPU: schedule-driven hyper-parameters of the fused LAMB / AdamW step (octic_lamb_step_hp / octic_adamw_step_hp read the
per-tensor lr and the EMA decay from device memory; train.FusedLamb.param_groups feeds them).  The new entry points equal
the scalar ones bit for bit at a uniform lr; per-group lr / weight decay changed at every step follow the foreach LAMB and
torch.optim.AdamW; a captured step follows a warm-up-then-cosine schedule and a changing EMA decay exactly like eager steps;
SSLTrainer runs the DINOv2 recipe's groups and schedules; a checkpoint taken in the middle of a schedule resumes bitwise."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


def _toy_params(dev="cuda"):
    g = torch.Generator().manual_seed(5)
    shapes = [(7,), (33, 17), (160, 160), (1000, 130), (3,), (70001,)]
    return [torch.randn(*s, generator=g).to(dev).requires_grad_(True) for s in shapes]


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


@pytest.mark.parametrize("adam", [False, True])
def test_hp_entry_points_equal_the_scalar_ones_at_a_uniform_lr(adam):
    """octic_*_step_hp with lr[i] = x and *ema_decay = d against octic_*_step(lr = x, ema_decay = d): parameters, moments,
    EMA, bf16 copies and the workspace BITWISE, over three steps whose lr and decay change (the first one clipped)."""
    from octic_vits_amd import _lib
    from octic_vits_amd.train import FusedLamb
    L = _lib.lib()
    runs = []
    for hp in (False, True):
        ps = _toy_params()
        groups = [{"params": [p for p in ps if p.ndim <= 1], "weight_decay": 0.0},
                  {"params": [p for p in ps if p.ndim > 1], "weight_decay": 0.02}]
        opt = FusedLamb(groups, lr=3e-3, ema_decay=0.9, adam=adam)
        shadows = [torch.zeros_like(p, dtype=torch.bfloat16) for p in opt.params]
        s_ptrs = torch.tensor([s.data_ptr() for s in shadows], dtype=torch.int64, device="cuda")
        gen = torch.Generator().manual_seed(11)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for step, (lr, decay) in enumerate([(3e-3, 0.9), (1e-3, 0.99), (2.5e-3, 0.95)]):
            grads = [(torch.randn(p.shape, generator=gen) * (5.0 if step == 0 else 0.1)).cuda() for p in opt.params]
            opt.g_ptrs.copy_(torch.tensor([g.data_ptr() for g in grads], dtype=torch.int64))
            common = [_vp(opt.p_ptrs), _vp(opt.g_ptrs), _vp(opt.m_ptrs), _vp(opt.v_ptrs), _vp(opt.e_ptrs), _vp(opt.wd),
                      _vp(opt.chunk_tensor), _vp(opt.chunk_off), _vp(opt.chunk_len), _vp(opt.tensor_chunk_begin),
                      opt.ntensors, opt.nchunks, _vp(opt.ws)]
            if hp:
                opt.lr, opt.ema_decay = lr, decay
                opt.push_hyper()
                fn = L.octic_adamw_step_hp if adam else L.octic_lamb_step_hp
                # an EMA without its decay is refused before any launch
                assert fn(*common, _vp(opt.lr_t), 0.9, 0.999, 1e-8, 1.0, 0, None, _vp(s_ptrs), stream) < 0
                rc = fn(*common, _vp(opt.lr_t), 0.9, 0.999, 1e-8, 1.0, 0, _vp(opt.ema_decay_t), _vp(s_ptrs), stream)
            else:
                fn = L.octic_adamw_step if adam else L.octic_lamb_step
                rc = fn(*common, lr, 0.9, 0.999, 1e-8, 1.0, 0, decay, _vp(s_ptrs), stream)
            assert rc == 0
            torch.cuda.synchronize()
        runs.append(([p.detach().clone() for p in opt.params], [opt.m, opt.v, opt.ema, opt.ws], shadows))
    (pa, sa, ha), (pb, sb, hb) = runs
    assert all(torch.equal(a, b) for a, b in zip(pa, pb))
    assert all(torch.equal(a, b) for a, b in zip(sa, sb))
    assert all(torch.equal(a, b) for a, b in zip(ha, hb))
    assert not torch.equal(pb[-1], _toy_params()[3])


def _groups(ps):
    return [{"params": [ps[0], ps[4]], "lr": 0.0, "weight_decay": 0.0},         # lr 0: these tensors never move
            {"params": [ps[1], ps[2]], "lr": 1e-3, "weight_decay": 0.02},
            {"params": [ps[3], ps[5]], "lr": 3e-3, "weight_decay": 0.05}]


def _schedule(step):
    """(lr, weight_decay) of the three groups at this step: groups 1 and 2 change at every step."""
    return [(0.0, 0.0), (1e-3 * (1 + step), 0.02 + 0.01 * step), (3e-3 / (1 + step), 0.05 - 0.01 * step)]


def _apply(groups, step):
    for g, (lr, wd) in zip(groups, _schedule(step)):
        g["lr"], g["weight_decay"] = lr, wd


def test_fused_lamb_param_groups_follow_per_step_lr_and_wd_like_the_foreach_lamb():
    from octic_vits_amd.train import FusedLamb, Lamb, ModelEma
    pa, pb = _toy_params(), _toy_params()
    b0 = [p.detach().clone() for p in pb]
    ref = Lamb(_groups(pa), lr=3e-3, weight_decay=0.02)
    order_a = [p for g in ref.param_groups for p in g["params"]]

    class _M:
        def __init__(self, ps): self.ps = ps
        def parameters(self): return self.ps
    ema = ModelEma(_M(order_a), decay=0.9)
    fused = FusedLamb(_groups(pb), lr=3e-3, ema_decay=0.9)
    assert [g["lr"] for g in fused.param_groups] == [0.0, 1e-3, 3e-3]
    gen = torch.Generator().manual_seed(11)
    for step in range(4):
        _apply(ref.param_groups, step)
        _apply(fused.param_groups, step)
        for a, b in zip(order_a, fused.params):
            gr = (torch.randn(a.shape, generator=gen) * (5.0 if step == 0 else 0.1)).cuda()
            a.grad, b.grad = gr.clone(), gr.clone()
        ref.step()
        ema.update(_M(order_a))
        fused.step()
        for a, b in zip(order_a, fused.params):
            assert torch.allclose(a, b, rtol=2e-5, atol=1e-6), f"step {step}: {(a - b).abs().max()}"
        for e_ref, e_f in zip(ema.params, fused.ema_state()):
            assert torch.allclose(e_ref, e_f, rtol=2e-5, atol=1e-6)
    assert torch.equal(pb[0], b0[0]) and torch.equal(pb[4], b0[4])
    assert all(not torch.equal(pb[i], b0[i]) for i in (1, 2, 3, 5))


def test_fused_adamw_param_groups_follow_per_step_lr_and_wd_like_torch_adamw():
    from octic_vits_amd.train import FusedLamb
    pa, pb = _toy_params(), _toy_params()
    b0 = [p.detach().clone() for p in pb]
    ref = torch.optim.AdamW(_groups(pa), lr=3e-3, betas=(0.9, 0.999), eps=1e-8)
    order_a = [p for g in ref.param_groups for p in g["params"]]
    fused = FusedLamb(_groups(pb), lr=3e-3, eps=1e-8, max_grad_norm=None, adam=True)
    gen = torch.Generator().manual_seed(12)
    for step in range(4):
        _apply(ref.param_groups, step)
        _apply(fused.param_groups, step)
        for a, b in zip(order_a, fused.params):
            gr = (torch.randn(a.shape, generator=gen) * 0.1).cuda()
            a.grad, b.grad = gr.clone(), gr.clone()
        ref.step()
        fused.step()
        for a, b in zip(order_a, fused.params):
            assert torch.allclose(a, b, rtol=2e-5, atol=1e-6), f"step {step}: {(a - b).abs().max()}"
    assert torch.equal(pb[0], b0[0]) and torch.equal(pb[4], b0[4])
    assert all(not torch.equal(pb[i], b0[i]) for i in (1, 2, 3, 5))


_KW = dict(img_size=32, patch_size=4, in_chans=3, num_classes=10, embed_dim=128, depth=4, num_heads=2, mlp_ratio=4.0,
           drop_path_rate=0.0, octic_equi_break_layer=2)


def _scheduled_run(graphed, set_values, steps=7):
    """Two warm-up steps on batch 0 (a capture's own eager warm-up, or plain steps), then `steps` steps on batches 1-3 with
    set_values(optimizer, i) in front of every one: losses, parameters, EMA."""
    from octic_vits_amd.model import OcticVisionTransformer
    from octic_vits_amd.train import Trainer, synthetic_batch
    torch.manual_seed(0)
    tr = Trainer(OcticVisionTransformer(**_KW).cuda(), lr=1e-3)
    batches = [synthetic_batch(8, 10, "cuda", seed=s, img_size=32) for s in range(4)]
    gs = tr.capture(*batches[0], warmup=2) if graphed else None
    if not graphed:
        for _ in range(2):
            tr.step(*batches[0])
    losses = []
    for i in range(steps):
        x, y = batches[1 + i % 3]
        set_values(tr.optimizer, i)
        losses.append(float(gs.replay(x, y) if graphed else tr.step(x, y).detach()))
    return (losses, [p.detach().clone() for p in tr.raw_model.parameters()],
            [e.clone() for e in tr.optimizer.ema_state()])


def _same(a, b):
    la, pa, ea = a
    lb, pb, eb = b
    assert la == lb, (la, lb)
    assert all(torch.equal(x, y) for x, y in zip(pa, pb))
    assert all(torch.equal(x, y) for x, y in zip(ea, eb))


def test_captured_step_follows_an_lr_and_wd_schedule_like_eager_steps():
    """The whole step as one hipGraph, param_groups[*]["lr"] (warm-up then cosine) and the decay group's weight decay set on
    the host before every replay: BITWISE the eager trainer's losses, weights and EMA; the same replays at a constant lr
    give other losses (the schedule reached the kernels)."""
    from octic_vits_amd.schedules import CosineScheduler
    lr_s = CosineScheduler(2e-3, 1e-5, total_iters=7, warmup_iters=3, start_warmup_value=1e-5)
    wd_s = CosineScheduler(0.02, 0.1, total_iters=7)

    def scheduled(opt, i):
        for g in opt.param_groups:
            g["lr"] = float(lr_s[i])
        opt.param_groups[1]["weight_decay"] = float(wd_s[i])

    eager = _scheduled_run(False, scheduled)
    replay = _scheduled_run(True, scheduled)
    _same(eager, replay)
    assert len(set(eager[0])) == len(eager[0])
    constant = _scheduled_run(True, lambda opt, i: None)
    # (the loss of an iteration is taken before its update: the first one is common to both runs)
    assert constant[0][0] == replay[0][0] and constant[0][1] != replay[0][1] and constant[0][-1] != replay[0][-1]


def test_captured_step_follows_a_changing_ema_decay_like_eager_steps():
    decays = [0.5, 0.9, 0.7, 0.99, 0.8, 0.6, 0.95]

    def scheduled(opt, i):
        opt.ema_decay = decays[i]

    eager = _scheduled_run(False, scheduled)
    replay = _scheduled_run(True, scheduled)
    _same(eager, replay)
    constant = _scheduled_run(True, lambda opt, i: None)          # the trainer's 0.99996
    assert constant[0] == replay[0]                               # the EMA does not feed back into the loss ...
    assert not all(torch.equal(x, y) for x, y in zip(constant[2], replay[2]))   # ... and follows the decay


def test_ssl_recipe_groups_and_schedules_fused_match_torch_adamw():
    """SSLTrainer(optim_groups=...) with the recipe's per-iteration lr, wd, momentum, teacher temperature and a last-layer lr
    frozen at 0 for two iterations: the fused path (per-tensor lr from layer-wise decay on octic_adamw_step_hp) against the
    torch.optim.AdamW twin over four f32 steps; during the freeze the head's last layer stays bitwise where it started."""
    from octic_vits_amd import ssl as S
    from octic_vits_amd.schedules import build_schedulers
    from test_ssl_gpu import _batch, _pair, _to
    _, a = _pair()
    _, b = _pair()
    images = _to(_batch(), "cuda")
    og = {"layerwise_decay": 0.9, "patch_embed_lr_mult": 0.2}
    ta = S.SSLTrainer(a, lr=2e-3, autocast=False, fused_optimizer=True, clip_grad=0.5, optim_groups=og)
    tb = S.SSLTrainer(b, lr=2e-3, autocast=False, fused_optimizer=False, clip_grad=0.5, optim_groups=og)
    lr_s, wd_s, mom_s, temp_s, last_s = build_schedulers(
        dict(lr=2e-3, min_lr=1e-4, epochs=3, warmup_epochs=1, weight_decay=0.04, weight_decay_end=0.2,
             freeze_last_layer_epochs=1),
        dict(momentum_teacher=0.9, final_momentum_teacher=1.0, teacher_temp=0.07, warmup_teacher_temp=0.04,
             warmup_teacher_temp_epochs=2), epoch_length=3)
    start = {n: p.detach().clone() for n, p in a.student.named_parameters()}
    for it in range(1, 5):                                      # last_layer_lr = 0 at iterations 1 and 2
        kw = dict(teacher_temp=float(temp_s[it]), momentum=float(mom_s[it]), lr=float(lr_s[it]), wd=float(wd_s[it]),
                  last_layer_lr=float(last_s[it]))
        la, lb = ta.step(images, **kw), tb.step(images, **kw)
        for k in lb:
            assert float(la[k].detach()) == pytest.approx(float(lb[k].detach()), rel=2e-4, abs=1e-5), (it, k)
        if it == 2:
            now = dict(a.student.named_parameters())
            frozen = [n for n in start if "last_layer" in n]
            assert frozen and all(torch.equal(now[n], start[n]) for n in frozen)
            moved = [n for n, p in now.items() if p.requires_grad and p.ndim >= 2 and "last_layer" not in n
                     and not torch.equal(p, start[n])]
            assert len(moved) > 40
    assert any(not torch.equal(p, start[n]) for n, p in a.student.named_parameters() if "last_layer.weight_v" in n)
    opt = ta._fused_opts["backbone"][0]
    assert len({round(g["lr_multiplier"], 12) for g in opt.param_groups}) >= 5
    tol = lambda n: 2 * 2e-3 * 4 if n.endswith(("qkv.lin_A1.bias", "qkv.bias")) else 2e-6
    for (n, pa), (_, pb) in zip(a.student.named_parameters(), b.student.named_parameters()):
        assert torch.allclose(pa, pb, rtol=2e-4, atol=tol(n)), n
    for (n, pa), (_, pb) in zip(a.teacher.named_parameters(), b.teacher.named_parameters()):
        assert torch.allclose(pa, pb, rtol=2e-4, atol=tol(n)), n


def test_state_dict_in_the_middle_of_a_schedule_resumes_bitwise_also_in_a_replay():
    """FusedLamb.state_dict after three scheduled steps, loaded into a fresh optimizer over copies of the parameters: the
    restored groups (lr, weight decay, numeric extra keys) carry on - first eagerly, then as a captured step replayed with
    new values pushed in front of each replay - BITWISE like the original.  A checkpoint without groups still loads."""
    from octic_vits_amd.train import FusedLamb

    def groups(ps):
        gs = _groups(ps)
        for g in gs:
            g.update(initial_lr=g["lr"], lr_multiplier=0.5, name="g")
        return gs

    pa = _toy_params()
    A = FusedLamb(groups(pa), lr=3e-3, ema_decay=0.9)
    gen = torch.Generator().manual_seed(21)
    grads = lambda: [(torch.randn(p.shape, generator=gen) * 0.1).cuda() for p in A.params]
    for step in range(3):
        _apply(A.param_groups, step)
        for p, g in zip(A.params, grads()):
            p.grad = g
        A.step()
    sd = A.state_dict()
    pb = [p.detach().clone().requires_grad_(True) for p in pa]
    B = FusedLamb(groups(pb), lr=1.0, ema_decay=0.5)
    B.load_state_dict(sd)
    for ga, gb in zip(A.param_groups, B.param_groups):
        assert {k: v for k, v in ga.items() if k != "params"} == {k: v for k, v in gb.items() if k != "params"}
    # step 3: no new values - both run on what the checkpoint restored
    for p, q, g in zip(A.params, B.params, grads()):
        p.grad, q.grad = g, g.clone()
    A.step()
    B.step()
    assert all(torch.equal(p, q) for p, q in zip(A.params, B.params))
    # B's step captured once; steps 4-6: A eager, B replays with the schedule's values pushed before each replay
    static = [torch.zeros_like(p) for p in B.params]
    for q, s in zip(B.params, static):
        q.grad = s
    B.prepare_capture()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        B.step()
    for step in range(4, 7):
        _apply(A.param_groups, step)
        _apply(B.param_groups, step)
        for p, s, g in zip(A.params, static, grads()):
            s.copy_(g)
            p.grad = g
        A.step()
        assert B.push_hyper()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(p, q) for p, q in zip(A.params, B.params)), step
    assert torch.equal(A.m, B.m) and torch.equal(A.v, B.v) and torch.equal(A.ema, B.ema)
    # a checkpoint written before the groups were saved: one lr for every tensor, the constructor's weight decay
    old = dict(sd)
    old.pop("param_groups")
    C = FusedLamb(groups([p.detach().clone().requires_grad_(True) for p in pa]), lr=1.0, ema_decay=0.5)
    C.load_state_dict(old)
    assert [g["lr"] for g in C.param_groups] == [3e-3] * 3
    assert [g["weight_decay"] for g in C.param_groups] == [0.0, 0.02, 0.05]
