"""Developer tool (needs the GPU): where a masked ring launch's time goes at the headline shape (ViT-H/14, batch 64, T = 257) -
unmasked, all kept (the prologue on live items), Bernoulli, alternating, all dropped (1030 dead items) - for the input gradients of
fc1 and qkv and for fc2 + residual.  Back-to-back warm launches, HIP events.

    python tools/bench_ring_skip.py"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from octic_vits_amd import ops  # noqa: E402

DEV = "cuda"
B, T = 64, 257
M = B * T

def run(cin, cout, fused):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(M, 8 * cin, generator=g).to(torch.bfloat16).to(DEV)
    w32 = [(torch.randn(s, generator=g) * 0.1).to(DEV) for s in [(cout, cin)] * 4 + [(2 * cout, 2 * cin)]]
    wb, _ = ops.linear_prep(w32, None, cin, cout, torch.bfloat16, want_wb=True)
    od = torch.float32 if fused else torch.bfloat16
    y = torch.empty(M, 8 * cout, dtype=od, device=DEV)
    resid = torch.randn(M, 8 * cout, device=DEV) if fused else None
    gen = torch.Generator().manual_seed(5)
    masks = {"unmasked": None, "all kept": torch.full((B,), 2.0), "bernoulli": torch.bernoulli(torch.full((B,), 0.5), generator=gen) * 2,
             "alternating": torch.tensor([2.0 * (b & 1) for b in range(B)]), "all dropped": torch.zeros(B)}
    for name, m in masks.items():
        ss = None if m is None else m.to(DEV)
        rs = (ss if ss is not None else torch.full((B,), 2.0, device=DEV)) if fused else None
        def call():
            ops.linear_fwd(ops.pview(x, cin), wb, None, ops.pview(y, cout), M, cin, cout, torch.bfloat16, od, x,
                           resid_v=None if resid is None else ops.pview(resid, cout), rs=rs, rps=T if fused else 1, dropped=ss, dropped_rps=T)
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(100):
            call()
        b.record()
        torch.cuda.synchronize()
        kept = "" if m is None else f" kept {int((m != 0).sum())}/{B}"
        print(f"cin {cin} cout {cout} fused {fused} {name:12s}{kept}: {a.elapsed_time(b) * 10:.1f} us per launch (back to back, warm)", flush=True)


run(640, 160, False)
run(480, 160, False)
run(640, 160, True)
