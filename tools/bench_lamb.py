"""Developer micro-benchmark: the fused LAMB + EMA step on the ViT-H parameter set (355.8 M parameters, 982 tensors), HIP-event
time per step and GB/s at 54 B per parameter.  OCTIC_LIB selects a library build (A/B of kernel variants).
--ab: in one process, alternate the scalar entry point (octic_lamb_step: lr and EMA decay as launch arguments) with the one
FusedLamb calls (octic_lamb_step_hp: both read from device memory), 8 blocks of 10 launches each, and print each one's mean
and spread."""
import ctypes, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from octic_vits_amd.deit_models import create_model
from octic_vits_amd.train import FusedLamb, param_groups_weight_decay, library_gemm_layers

torch.manual_seed(0)
model = create_model("hybrid_deit_huge_patch14", num_classes=1000, drop_path_rate=0.5, img_size=224).cuda()
opt = FusedLamb(param_groups_weight_decay(model, 0.02, model.no_weight_decay()), ema_decay=0.99996, shadow_layers=library_gemm_layers(model))
n = sum(p.numel() for p in opt.params)
for p in opt.params:
    p.grad = torch.randn_like(p) * 1e-3


def entry_step(hp):
    """One launch of either entry point on the optimizer's tables, nothing around it (the gradient table is current after
    one FusedLamb.step)."""
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    o = opt
    lib = o._lib.lib()
    head = (vp(o.p_ptrs), vp(o.g_ptrs), vp(o.m_ptrs), vp(o.v_ptrs), vp(o.e_ptrs), vp(o.wd), vp(o.chunk_tensor), vp(o.chunk_off),
            vp(o.chunk_len), vp(o.tensor_chunk_begin), o.ntensors, o.nchunks, vp(o.ws))
    tail = (float(o.betas[0]), float(o.betas[1]), float(o.eps), float(o.max_grad_norm or 0.0), 0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if hp:
        rc = lib.octic_lamb_step_hp(*head, vp(o.lr_t), *tail, vp(o.ema_decay_t), vp(o.s_ptrs), stream)
    else:
        rc = lib.octic_lamb_step(*head, float(o.lr), *tail, float(o.ema_decay or 0.0), vp(o.s_ptrs), stream)
    o._lib.check(rc)


def block(fn, k=10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(k):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / k


if "--ab" in sys.argv:
    opt.step()
    times = {"octic_lamb_step": [], "octic_lamb_step_hp": []}
    for rep in range(8):
        for name, fn in (("octic_lamb_step", lambda: entry_step(False)),
                         ("octic_lamb_step_hp", lambda: entry_step(True)))[::1 if rep % 2 == 0 else -1]:
            times[name].append(block(fn))
    for name, t in times.items():
        print(f"{name:20s} mean {statistics.mean(t):.3f} ms  stdev {statistics.stdev(t):.3f}  min {min(t):.3f}  max {max(t):.3f}"
              f"  ({len(t)} blocks of 10 steps, {n / 1e6:.1f} M parameters)")
    sys.exit(0)
best = 1e9
for rep in range(4):
    best = min(best, block(opt.step))
print(f"lamb step ({os.environ.get('OCTIC_LIB', 'default lib')}): {best:.3f} ms for {n / 1e6:.1f} M parameters = {n * 54 / best / 1e9:.0f} GB/s at 54 B/param")
