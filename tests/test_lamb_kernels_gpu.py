"""GPU: the fused multi-tensor LAMB / AdamW step (csrc/lamb.hip: octic_lamb_step, octic_adamw_step and their _hp twins) through
the C ABI, against oracle/lamb_ref.py (numpy float64, no code shared with the product), at the places where such kernels
go wrong: every alignment of every operand (the 16-byte-vector and the element paths of gradsq / stage 1 / stage 2, which
decide independently), every tail length, chunk edges and far chunk offsets, more tensors than one workgroup of the ratio
kernel holds, the trust-ratio gates, the clip edges, the host and device step counters far into a run, non-finite
gradients - and that nothing outside a tensor's extent is ever written.

The harness builds the pointer tables and the chunk list itself (the rule of train.FusedLamb.__init__, restated).  Each of
p, g, m, v, EMA and the bf16 copy lives in an arena of its own, pre-filled with a NaN bit pattern; every tensor sits at a
chosen element offset inside it with at least 8 sentinel elements on either side, so every pointer the kernels see points
into a live allocation, and every arena byte outside the tensors is compared bitwise afterwards.

Bars (all the project's own): p and EMA rtol 2e-5 / atol 1e-6 (test_fused_lamb_matches_independent_restatement); m, v and
the consumed gradient u 2e-5 of the tensor's largest magnitude in the reference; gradient norm 1e-5 relative; the bf16
copy bitwise the round-to-nearest-even cast of the kernel's own f32 parameter.  tests/test_lamb_oracle.py shows an
independent f32 implementation on the same cases staying within 1 % / 3e-6 / 1e-6 of these; the kernels measured, on the
size matrix: p 1.5 % of its bar, m 1.4e-7, v 2.0e-7 and u 3.6e-6 of scale, gradient norm 5.9e-8 (each test prints its own).
u's share is the f32 rounding of 1 - b2^t at t = 2 and 3 (an ulp of 0.998 against 0.002: 6.7e-6 of it, half of that on u)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import lamb_cases as C
from oracle.lamb_ref import LambRef, ema_update

pytestmark = pytest.mark.gpu

GUARD = 8                        # sentinel elements on either side of every tensor, at least
ALIGN = 8                        # undisplaced tensors start at a multiple of 8 elements: 32 B in f32, 16 B in bf16
SENTINEL = {torch.float32: (torch.int32, 0x7FC5A5A5), torch.bfloat16: (torch.int16, 0x7FC5)}   # quiet NaNs
EPS, DECAY = 1e-8, 0.9
DEV = "cuda"                     # where the arenas and tables live
OPERANDS = ("p", "g", "m", "v", "ema", "bf16")


def _f32(x):
    """The value the kernel receives for a hyper-parameter passed as float: the reference computes with the same one."""
    return float(np.float32(x))


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Arena:
    """One device tensor full of sentinels; tensor i occupies elements [start[i], start[i] + numel[i]) of it (None: absent)."""

    def __init__(self, numels, shift, dtype, present=None):
        self.dtype, (self.itype, self.sentinel) = dtype, SENTINEL[dtype]
        self.numels, self.start, off = list(numels), [], GUARD
        for i, n in enumerate(numels):
            if present is not None and not present[i]:
                self.start.append(None)
                continue
            self.start.append(off + shift)
            off = (off + shift + n + GUARD + ALIGN - 1) // ALIGN * ALIGN
        self.bits = torch.full((off + GUARD,), self.sentinel, dtype=self.itype, device=DEV)
        self.t = self.bits.view(dtype)
        assert self.t.data_ptr() % 16 == 0
        guard = np.ones(off + GUARD, dtype=bool)
        for s, n in zip(self.start, numels):
            if s is not None:
                assert s >= GUARD and guard[s - GUARD:s + n + GUARD].all() and s + n + GUARD <= guard.size
                guard[s:s + n] = False
        self.guard = guard

    def ptr(self, i):
        return 0 if self.start[i] is None else self.t.data_ptr() + self.start[i] * self.t.element_size()

    def put(self, values):
        for s, n, val in zip(self.start, self.numels, values):
            if s is not None:
                self.t[s:s + n].copy_(val.reshape(-1).to(self.dtype))

    def host_bits(self):
        return self.bits.cpu()

    def split(self, host_bits):
        """The tensors' values out of a host copy of the arena (None where absent)."""
        h = host_bits.view(self.dtype)
        return [None if s is None else h[s:s + n] for s, n in zip(self.start, self.numels)]

    def guards_intact(self, host_bits):
        return bool((host_bits.numpy()[self.guard] == self.sentinel).all())


class Problem:
    """Tables, chunk list, workspace and arenas for a list of (numel, wd, lr) entries.  ``shifts``: operand -> displacement in
    elements of that operand's type.  ``shadow``: "some" (the bf16 table has null entries), "all", or None (no table)."""

    def __init__(self, entries, params, shifts=None, ema=True, shadow="some"):
        from octic_vits_amd import _lib
        from octic_vits_amd.train import FusedLamb
        assert FusedLamb.CHUNK == C.CHUNK
        self.L = _lib.lib()
        self.entries, self.n = entries, len(entries)
        numels = [e[0] for e in entries]
        shifts = dict(shifts or {})
        i32, i64, f32 = torch.int32, torch.int64, torch.float32
        self.arena = {k: Arena(numels, shifts.get(k, 0), f32) for k in ("p", "g", "m", "v")}
        if ema:
            self.arena["ema"] = Arena(numels, shifts.get("ema", 0), f32)
        if shadow:
            present = [shadow == "all" or i % 4 != 1 for i in range(self.n)]
            self.arena["bf16"] = Arena(numels, shifts.get("bf16", 0), torch.bfloat16, present)
        dev = DEV
        self.ptrs = {k: torch.tensor([a.ptr(i) for i in range(self.n)], dtype=i64, device=dev) for k, a in self.arena.items()}
        ct, co, cl, tb = [], [], [], [0]
        for i, n in enumerate(numels):
            for o in range(0, n, C.CHUNK):
                ct.append(i); co.append(o); cl.append(min(C.CHUNK, n - o))
            tb.append(len(ct))
        self.nchunks = len(ct)
        self.chunk_tensor = torch.tensor(ct, dtype=i32, device=dev)
        self.chunk_off = torch.tensor(co, dtype=i64, device=dev)
        self.chunk_len = torch.tensor(cl, dtype=i32, device=dev)
        self.tensor_chunk_begin = torch.tensor(tb, dtype=i32, device=dev)
        self.wd = torch.tensor([e[1] for e in entries], dtype=f32, device=dev)
        self.lr_t = torch.tensor([e[2] for e in entries], dtype=f32, device=dev)
        self.decay_t = torch.tensor([DECAY], dtype=f32, device=dev)
        self.ws = torch.zeros(int(self.L.octic_lamb_workspace_floats(self.n, self.nchunks)), dtype=f32, device=dev)
        zeros = [torch.zeros(n) for n in numels]
        self.arena["p"].put(params)
        self.arena["m"].put(zeros)
        self.arena["v"].put(zeros)
        if ema:
            self.arena["ema"].put(params)
        if shadow:
            self.arena["bf16"].put(zeros)

    def step(self, grads, mode="lamb", hp=False, max_norm=1.0, step=0):
        """One call of the entry point.  grads=None leaves the gradient arena as it is."""
        if grads is not None:
            self.arena["g"].put(grads)
        a = self.ptrs
        common = [_vp(a["p"]), _vp(a["g"]), _vp(a["m"]), _vp(a["v"]), _vp(a.get("ema")), _vp(self.wd), _vp(self.chunk_tensor),
                  _vp(self.chunk_off), _vp(self.chunk_len), _vp(self.tensor_chunk_begin), self.n, self.nchunks, _vp(self.ws)]
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        if hp:
            fn = self.L.octic_adamw_step_hp if mode == "adamw" else self.L.octic_lamb_step_hp
            rc = fn(*common, _vp(self.lr_t), 0.9, 0.999, EPS, float(max_norm), step, _vp(self.decay_t) if "ema" in a else None,
                    _vp(a.get("bf16")), stream)
        else:
            assert len({e[2] for e in self.entries}) == 1, "the scalar entry points take one lr"
            fn = self.L.octic_adamw_step if mode == "adamw" else self.L.octic_lamb_step
            rc = fn(*common, self.entries[0][2], 0.9, 0.999, EPS, float(max_norm), step, DECAY, _vp(a.get("bf16")), stream)
        assert rc == 0
        torch.cuda.synchronize()

    def snapshot(self):
        """Host copies of every arena (as bits) and of the workspace."""
        snap = {k: a.host_bits() for k, a in self.arena.items()}
        snap["ws"] = self.ws.cpu()
        return snap

    def values(self, snap):
        return {k: a.split(snap[k]) for k, a in self.arena.items()}

    def assert_guards(self, snap, label=""):
        for k, a in self.arena.items():
            assert a.guards_intact(snap[k]), f"{label}: the step wrote outside a tensor's extent in the {k} arena"


def reference(entries, params, grad_steps, mode, max_norm, t_before=None):
    """LambRef + ema_update in f64 on the same f32 values -> per step dict(p, m, v, u, ema: lists of arrays; gn).
    t_before: per step, the value to give ``ref.t`` before it (None: leave the counter alone)."""
    ref = LambRef([(e[0],) for e in entries], [_f32(e[1]) for e in entries], lr=[_f32(e[2]) for e in entries],
                  betas=(_f32(0.9), _f32(0.999)), eps=_f32(EPS), max_grad_norm=max_norm, trust_ratio=(mode == "lamb"))
    cur = [p.double().numpy().copy() for p in params]
    ema = [c.copy() for c in cur]
    out = []
    for s, grads in enumerate(grad_steps):
        if t_before is not None and t_before[s] is not None:
            ref.t = t_before[s]
        cur = ref.step(cur, [g.double().numpy() for g in grads])
        ema = ema_update(ema, cur, _f32(DECAY))
        out.append(dict(p=cur, m=list(ref.m), v=list(ref.v), u=list(ref.last_updates), ema=ema, gn=ref.last_grad_norm, t=ref.t))
    return out


def assert_step(prob, snap, want, label, report=None):
    """The state after one applied step against the reference, tensor by tensor, at the bars of the module docstring."""
    got = prob.values(snap)
    ws = snap["ws"].numpy()
    assert ws[2] == 0.0 and ws[3] == want["t"], f"{label}: skipped flag {ws[2]}, step counter {ws[3]} (want {want['t']})"
    gn_err = abs(float(ws[1]) - want["gn"]) / want["gn"] if want["gn"] > 0 else float(ws[1] != 0.0)
    assert gn_err <= 1e-5, f"{label}: gradient norm {ws[1]} vs {want['gn']}"
    worst = {"gn": gn_err, "p": 0.0, "ema": 0.0, "m": 0.0, "v": 0.0, "u": 0.0}
    for i, (n, wd, lr) in enumerate(prob.entries):
        where = f"{label}, tensor {i} (numel {n}, wd {wd})"
        for key in ("p", "ema"):
            if key not in got:
                continue
            have, ref = got[key][i].double().numpy(), want[key][i]
            assert np.isfinite(have).all(), f"{where}: non-finite {key}"
            rel = float((np.abs(have - ref) / (1e-6 + 2e-5 * np.abs(ref))).max())
            worst[key] = max(worst[key], rel)
            assert rel <= 1.0, f"{where}: {key} off by {rel:.3g} of rtol 2e-5 / atol 1e-6 at element {int(np.argmax(np.abs(have - ref)))}"
        for key, src in (("m", "m"), ("v", "v"), ("u", "g")):
            have, ref = got[src][i].double().numpy(), want[key][i]
            scale = float(np.abs(ref).max())
            err = float(np.abs(have - ref).max())
            if scale > 0:
                worst[key] = max(worst[key], err / scale)
            assert err <= 2e-5 * scale, f"{where}: {key} off by {err:.3g}, scale {scale:.3g}"
        if "bf16" in got and got["bf16"][i] is not None:
            cast = got["p"][i].to(torch.bfloat16)
            assert torch.equal(got["bf16"][i].view(torch.int16), cast.view(torch.int16)), f"{where}: bf16 copy is not the cast of p"
    if report is not None:
        for k, x in worst.items():
            report[k] = max(report.get(k, 0.0), x)
    return worst


def _show(name, report):
    print(f"{name}: worst error in units of its bar - p {report['p']:.2e}, ema {report['ema']:.2e}; relative to scale - "
          f"m {report['m']:.2e}, v {report['v']:.2e}, u {report['u']:.2e}; gradient norm {report['gn']:.2e}")


# ---- a. size and alignment matrix ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _matrix_case(mode):
    ps, gs = C.matrix_inputs()
    return ps, gs, reference(C.matrix_entries(), ps, gs, mode, 1.0)


def _matrix_params():
    out = []
    for tables in ("ema+bf16", "ema", "bf16", "neither"):
        ops = [("none", 0)] + [(op, s) for op in OPERANDS + ("all",) if op in ("p", "g", "m", "v", "all") or op in tables
                               for s in (1, 2, 3)]
        out += [pytest.param(mode, op, s, tables, id=f"{mode}-{tables}-{op}{s or ''}") for op, s in ops for mode in ("lamb", "adamw")]
    return out


@pytest.mark.parametrize("mode,operand,shift,tables", _matrix_params())
def test_size_and_alignment_matrix(mode, operand, shift, tables):
    """Lengths 1..8, 255..257, 1023..1025, 65535..65537, 131072, 131073 and 196613 (three chunks and a tail of 5) in one call,
    wd alternating, three steps of the scalar entry points with the first one clipped.  One operand - or all of them - is
    displaced by 1, 2 or 3 elements of its type from a 16-byte boundary (bf16: 2, 4, 6 bytes, across the 8-byte test of
    stage 2), with the complete set of tables (the bf16 table has null entries), without the EMA table, without the bf16
    table and without both."""
    ent = C.matrix_entries()
    ps, gs, want = _matrix_case(mode)
    shifts = {k: shift for k in OPERANDS if operand in (k, "all")}
    prob = Problem(ent, ps, shifts, ema="ema" in tables, shadow="some" if "bf16" in tables else None)
    for k, a in prob.arena.items():      # the displacement is what the kernels will see
        assert all(p % 16 == (shifts.get(k, 0) * a.t.element_size()) % 16 for p in prob.ptrs[k].tolist() if p)
    report = {}
    for s in range(3):
        prob.step(gs[s], mode=mode, max_norm=1.0)
        snap = prob.snapshot()
        assert snap["ws"][0] < (0.01 if s == 0 else 1.0)       # clipped, the first step 50 times harder
        assert_step(prob, snap, want[s], f"step {s}", report)
    prob.assert_guards(snap)
    _show(f"matrix {mode} {tables} {operand} {shift}", report)


# ---- b. more tensors than one workgroup of the ratio kernel -----------------------------------------------------------------

def _assert_many_tensors_premise(ent, ps, first, mode):
    """What makes the many-tensor case bite, from the inputs and the f64 reference's first step alone.  The learning rates
    are pairwise distinct as f32, and those 1, 2, 8 and 256 slots apart (the neighbour, the next tensor of the same decay
    class, a short period, the same thread of the next workgroup) differ by more than 2.5 % - over a thousand times the
    2e-5 of the p bar; taking the lr from 1, 2 or 256 slots away moves more than half of the tensors past ten times their p
    bar (the rest are those of the largest |p| without a trust ratio, where 2e-5 |p| outweighs lr).  Under LAMB the trust
    ratios of decayed tensors 2 and 256 slots apart differ by more than a factor of 1.4."""
    n = len(ent)
    lr = np.array([np.float32(e[2]) for e in ent], dtype=np.float64)
    srt = np.sort(lr)
    assert ((srt[1:] - srt[:-1]) > 1e-4 * srt[1:]).all(), "two tensors share a learning rate"
    for d in (1, 2, 8, 256):
        if d < n:
            assert (np.abs(lr[d:] - lr[:-d]) > 0.025 * np.maximum(lr[d:], lr[:-d])).all(), f"lr aliases at distance {d}"
    un = [np.linalg.norm(u) for u in first["u"]]
    ratio = [np.linalg.norm(p.double().numpy()) / u if (mode == "lamb" and e[1]) else 1.0 for p, u, e in zip(ps, un, ent)]
    for d in (d for d in (1, 2, 256) if d < n):
        past =[bool((abs(lr[i] - lr[i - d]) * ratio[i] * np.abs(first["u"][i])
                      > 10.0 * (1e-6 + 2e-5 * np.abs(first["p"][i]))).any()) for i in range(d, n)]
        assert sum(past) > 0.5 * len(past), f"an lr from {d} slots away would go unnoticed in most tensors"
    if mode == "lamb":
        decayed = [i for i in range(n) if ent[i][1]]
        assert all(abs(np.log2(ratio[i] / ratio[i - 2])) > 0.5 for i in decayed[1:])
        assert all(abs(np.log2(ratio[i] / ratio[i - 256])) > 0.5 for i in decayed if i >= 256)


@pytest.mark.parametrize("mode", ["lamb", "adamw"])
@pytest.mark.parametrize("ntensors", [255, 256, 257, 600])
def test_many_tensors_each_with_its_own_lr_and_ratio(ntensors, mode):
    """lamb_ratio_kernel runs one thread per tensor, 256 per block: 255 / 256 / 257 tensors sit on its edge, 600 fill three
    blocks.  Through the _hp entry points, every tensor with its own lr (no two equal, none aliasing at a distance of 1, 2, 8
    or 256 slots) and - by magnitudes stepped in powers of two - its own trust ratio, so a ratio or lr taken from another
    tensor's slot misses the bar many times over; the premise is asserted before the kernel runs.  Two steps; the
    second gradient is the first one times a positive factor per element, so that no m = b1 m + (1 - b1) g cancels: in a
    tensor of one or two elements a cancelled m would put the rounding of the f32 clip factor at the tensor's whole scale,
    and this case is about indices, not conditioning."""
    ent = C.many_entries(ntensors)
    ps, g0 = C.many_inputs(ntensors)
    gen = torch.Generator().manual_seed(37)
    gs = [g0, [g * (0.25 + torch.rand(g.shape, generator=gen)) for g in g0]]
    want = reference(ent, ps, gs, mode, 1.0)
    _assert_many_tensors_premise(ent, ps, want[0], mode)
    prob = Problem(ent, ps, {"g": 1, "ema": 2}, shadow="some")
    report = {}
    for s in range(2):
        prob.step(gs[s], mode=mode, hp=True, max_norm=1.0)
        snap = prob.snapshot()
        assert_step(prob, snap, want[s], f"step {s}", report)
    prob.assert_guards(snap)
    _show(f"many {ntensors} {mode}", report)


# ---- c. trust-ratio gates ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["lamb", "adamw"])
def test_trust_ratio_gates(mode):
    """One unclipped step (max_grad_norm = 0) of lamb_cases.gate_entries(): |p| = 0 with weight decay (ratio 1, finite), zero
    gradient with weight decay (LAMB: u = wd p, ratio 1 / wd, p (1 - lr) - a gate on the gradient would give p (1 - lr wd)),
    zero gradient without (nothing moves, bitwise), wd = 0 with |p| / |u| ~ 1e3 (ratio 1), and a three-chunk tensor that is
    non-zero in its last chunk only between neighbours whose norms are orders of magnitude away (a chunk range off by one
    at either end changes its ratio 100-fold).  In AdamW mode the ratio is 1 everywhere."""
    ent = C.gate_entries()
    ps, gs = C.gate_inputs()
    want = reference(ent, ps, [gs], mode, 0.0)
    prob = Problem(ent, ps, shadow="all")
    prob.step(gs, mode=mode, hp=True, max_norm=0.0)
    snap = prob.snapshot()
    assert snap["ws"][0] == 1.0 and snap["ws"][1] > 0
    _show(f"gates {mode}", assert_step(prob, snap, want[0], mode))
    got = prob.values(snap)
    lr, wd = _f32(C.LR), _f32(C.WD)
    i = C.GATE_ZERO_G_WD
    moved = ps[i].double().numpy() * ((1.0 - lr) if mode == "lamb" else (1.0 - lr * wd))
    assert np.allclose(got["p"][i].double().numpy(), moved, rtol=2e-5, atol=1e-6)
    i = C.GATE_ZERO_G
    assert torch.equal(got["p"][i].view(torch.int32), ps[i].view(torch.int32))
    assert not got["m"][i].view(torch.int32).any() and not got["v"][i].view(torch.int32).any()
    for i in (C.GATE_ZERO_P, C.GATE_FAR):    # ratio 1: the step is lr * u with u = +-1 at the first step
        assert np.allclose(np.abs((got["p"][i] - ps[i]).double().numpy()), lr, rtol=1e-3 if i == C.GATE_ZERO_P else 0.1)
    i = C.GATE_LAST_CHUNK
    assert not got["p"][i][:2 * C.CHUNK].view(torch.int32).any() and not got["g"][i][:2 * C.CHUNK].view(torch.int32).any()
    if mode == "lamb":
        p64 = ps[i].double().numpy()[2 * C.CHUNK:]
        u = np.sign(gs[i].double().numpy()[2 * C.CHUNK:]) + wd * p64
        ratio = np.linalg.norm(p64) / np.linalg.norm(u)
        assert 0.005 < ratio < 0.02
        assert np.allclose(got["p"][i].double().numpy()[2 * C.CHUNK:], p64 - lr * ratio * u, rtol=2e-5, atol=1e-6)
    prob.assert_guards(snap)


@pytest.mark.parametrize("mode", ["lamb", "adamw"])
def test_all_gradients_zero(mode):
    """gn = 0: the clip factor is 1, nothing is NaN (0 / (0 + eps) = 0), the step counts (ws[3] advances, ws[2] = 0), moments
    stay bitwise zero and the parameters move by weight decay alone: p (1 - lr) under LAMB (ratio 1 / wd), p (1 - lr wd) under
    AdamW, not at all where wd = 0."""
    ent = C.gate_entries()
    ps, gs = C.gate_inputs(all_grads_zero=True)
    want = reference(ent, ps, [gs], mode, 0.0)
    prob = Problem(ent, ps, shadow="all")
    prob.step(gs, mode=mode, hp=True, max_norm=0.0)
    snap = prob.snapshot()
    ws = snap["ws"].numpy()
    assert ws[0] == 1.0 and ws[1] == 0.0 and ws[2] == 0.0 and ws[3] == 1.0 and ws[6] == 0.0
    assert_step(prob, snap, want[0], mode)
    got = prob.values(snap)
    lr, wd = _f32(C.LR), _f32(C.WD)
    for i, e in enumerate(ent):
        assert not got["m"][i].view(torch.int32).any() and not got["v"][i].view(torch.int32).any()
        if e[1] == 0.0:
            assert torch.equal(got["p"][i].view(torch.int32), ps[i].view(torch.int32))
        else:
            moved = ps[i].double().numpy() * ((1.0 - lr) if mode == "lamb" else (1.0 - lr * wd))
            assert np.allclose(got["p"][i].double().numpy(), moved, rtol=2e-5, atol=1e-6)
    prob.assert_guards(snap)


# ---- d. clip edges -----------------------------------------------------------------------------------------------------------

EDGE_ENTRIES = [(1025, C.WD, C.LR), (7, 0.0, C.LR), (C.CHUNK + 1030, C.WD, C.LR), (6, 0.0, C.LR)]


def _edge_params():
    gen = torch.Generator().manual_seed(29)
    return [torch.randn(n, generator=gen) for n, _, _ in EDGE_ENTRIES]


def _edge_grads(seed, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=gen) * scale for n, _, _ in EDGE_ENTRIES]


@pytest.mark.parametrize("max_norm,clip", [(5.0, 1.0), (4.0, 0.8)])
def test_clip_at_and_just_above_the_norm(max_norm, clip):
    """g = (3, 4) and zeros elsewhere: sum g^2 = 25 and the norm 5 are exact in f32.  max_grad_norm = 5: gn > max_norm is
    false, so ws[0] = 1 and ws[1] = 5 exactly.  max_grad_norm = 4: ws[0] = 4 / 5 to f32 rounding (one ulp of 0.8 = 2^-24)."""
    ps = _edge_params()
    gs = [torch.zeros(n) for n, _, _ in EDGE_ENTRIES]
    gs[2][C.CHUNK + 1] = 3.0
    gs[2][C.CHUNK + 2] = 4.0
    want = reference(EDGE_ENTRIES, ps, [gs], "lamb", max_norm)
    prob = Problem(EDGE_ENTRIES, ps, {"g": 1})
    prob.step(gs, max_norm=max_norm)
    snap = prob.snapshot()
    ws = snap["ws"].numpy()
    assert ws[1] == 5.0
    assert ws[0] == 1.0 if clip == 1.0 else abs(float(ws[0]) - 0.8) <= 2.0 ** -24
    assert_step(prob, snap, want[0], f"max_norm {max_norm}")
    prob.assert_guards(snap)


def test_no_clipping_at_max_grad_norm_zero():
    """max_grad_norm = 0 means no clipping, however large the norm (here ~2.6e4): ws[0] = 1, ws[1] the norm, results as the
    reference without clipping - which differ from the clipped ones in m and v by eight orders of magnitude."""
    ps, gs = _edge_params(), _edge_grads(31, 100.0)
    want = reference(EDGE_ENTRIES, ps, [gs], "lamb", 0.0)
    assert want[0]["gn"] > 2000
    prob = Problem(EDGE_ENTRIES, ps, {"p": 2})
    prob.step(gs, max_norm=0.0)
    snap = prob.snapshot()
    assert snap["ws"][0] == 1.0
    assert_step(prob, snap, want[0], "no clip")
    prob.assert_guards(snap)


# ---- e. step counter and bias correction -------------------------------------------------------------------------------------

def test_host_step_argument_equals_the_device_counter_bitwise():
    """Three steps with step = 0 (the device counter ws[3]) and three with step = 1, 2, 3: every arena and the whole workspace,
    ws[3] included, bitwise equal."""
    ps = _edge_params()
    snaps = []
    for host in (False, True):
        prob = Problem(EDGE_ENTRIES, ps, {"v": 3}, shadow="all")
        for s in range(3):
            prob.step(_edge_grads(40 + s, 5.0 if s == 0 else 0.1), hp=True, step=s + 1 if host else 0)
        snaps.append(prob.snapshot())
    assert snaps[0]["ws"][3] == 3.0
    for k in snaps[0]:
        assert torch.equal(snaps[0][k].view(torch.int32 if k == "ws" else snaps[0][k].dtype),
                           snaps[1][k].view(torch.int32 if k == "ws" else snaps[1][k].dtype)), k


@pytest.mark.parametrize("mode", ["lamb", "adamw"])
@pytest.mark.parametrize("resumed,host", [(999, False), (99999, False), (999, True), (99999, True)])
def test_bias_correction_far_into_a_run(resumed, host, mode):
    """What a resumed checkpoint does (load_state_dict -> ws[3]): one ordinary step, then the counter is set to 999 / 99999 -
    on the device, or the next number is passed as the host step - and the next step must be LambRef's with t set to match:
    1 - b2^1000 = 0.632 (AdamW steps are 26 % larger than with 1), 1 - b2^100000 = 1."""
    ps = _edge_params()
    gs = [_edge_grads(50, 5.0), _edge_grads(51, 0.1)]
    want = reference(EDGE_ENTRIES, ps, gs, mode, 1.0, t_before=[None, resumed])
    prob = Problem(EDGE_ENTRIES, ps, {"m": 1})
    prob.step(gs[0], mode=mode)
    assert_step(prob, prob.snapshot(), want[0], "first step")
    if not host:
        prob.ws[3] = float(resumed)
    prob.step(gs[1], mode=mode, step=resumed + 1 if host else 0)
    snap = prob.snapshot()
    assert snap["ws"][3] == resumed + 1
    assert_step(prob, snap, want[1], f"step {resumed + 1}")
    prob.assert_guards(snap)


# ---- f. non-finite values ----------------------------------------------------------------------------------------------------

def _poison(kind):
    """(shifts, tensor, element, value)"""
    if kind == "inf in the last element of a displaced tensor":
        return {"g": 3, "p": 3, "m": 3, "v": 3, "ema": 3, "bf16": 3}, 0, EDGE_ENTRIES[0][0] - 1, float("inf")
    if kind == "nan in the vector body of the second chunk":
        return {}, 2, C.CHUNK + 512, float("nan")
    return {}, 2, 17, 1e20       # finite, but its square is not


@pytest.mark.parametrize("kind", ["inf in the last element of a displaced tensor", "nan in the vector body of the second chunk",
                                  "1e20: the f32 sum of squares overflows"])
def test_non_finite_norm_skips_the_step_and_touches_nothing(kind):
    """A non-finite gradient norm skips the step: ws[2] = 1, ws[6] counts it, ws[3] does not advance, and p, m, v, EMA, the bf16
    copies and the gradient itself are bitwise what they were, as is everything around them.  A finite gradient of 1e20 is
    treated the same BY DESIGN: the norm is accumulated in f32, 1e40 is not representable, and a step whose clip factor
    cannot be formed is refused rather than guessed (the f64 reference would clip it to 1)."""
    shifts, ti, el, value = _poison(kind)
    ps = _edge_params()
    prob = Problem(EDGE_ENTRIES, ps, shifts, shadow="all")
    prob.step(_edge_grads(60, 5.0))
    bad = _edge_grads(61, 0.1)
    bad[ti][el] = value
    prob.arena["g"].put(bad)
    before = prob.snapshot()
    assert before["ws"][3] == 1.0 and before["ws"][6] == 0.0
    prob.step(None)
    after = prob.snapshot()
    ws = after["ws"].numpy()
    assert ws[2] == 1.0 and ws[6] == 1.0 and ws[3] == 1.0 and not np.isfinite(ws[1])
    for k in prob.arena:
        assert torch.equal(before[k], after[k]), f"a skipped step changed the {k} arena"
    # ... and the next finite step is applied as step 2
    good = _edge_grads(62, 0.1)
    want = reference(EDGE_ENTRIES, ps, [_edge_grads(60, 5.0), good], "lamb", 1.0)
    prob.step(good)
    snap = prob.snapshot()
    assert snap["ws"][6] == 1.0
    assert_step(prob, snap, want[1], "the step after the skipped one")
    prob.assert_guards(snap)


# ---- g. through FusedLamb, gradients packed like DDP's bucket views ----------------------------------------------------------

FUSED_SHAPES = [(7,), (33, 17), (3,), (129, 5), (70001,), (4,), (256, 256), (131073,), (5, 5)]


@pytest.mark.parametrize("adam", [False, True])
def test_fused_lamb_on_packed_gradient_views(adam):
    """Gradients are views of one flat f32 buffer, back to back without padding, as DistributedDataParallel's
    gradient_as_bucket_view=True hands them over: after an odd-sized tensor they are 4-byte aligned only.  step() must keep
    those views (same address, no copy), leave u in them, match LambRef over three steps, and leave the pad elements of
    its flat m / v / EMA (beyond each tensor's numel, up to the next multiple of 4) exactly zero.  adam=True: AdamW with the
    EMA kept in external tensors."""
    from octic_vits_amd.train import FusedLamb
    gen = torch.Generator().manual_seed(5)
    ps = [torch.randn(*s, generator=gen).cuda().requires_grad_(True) for s in FUSED_SHAPES]
    host = [p.detach().cpu().reshape(-1) for p in ps]
    groups = [{"params": [p for p in ps if p.ndim <= 1], "weight_decay": 0.0},
              {"params": [p for p in ps if p.ndim > 1], "weight_decay": C.WD}]
    ext = {id(p): p.detach().clone() for p in ps} if adam else None
    opt = FusedLamb(groups, lr=C.LR, eps=EPS, ema_decay=DECAY, adam=adam, ema_tensors=ext)
    order = opt.params
    index = [next(j for j, q in enumerate(ps) if q is p) for p in order]
    ent = [(p.numel(), 0.0 if p.ndim <= 1 else C.WD, C.LR) for p in order]
    gen = torch.Generator().manual_seed(11)
    gs = [[torch.randn(e[0], generator=gen) * (5.0 if s == 0 else 0.1) for e in ent] for s in range(3)]
    want = reference(ent, [host[j] for j in index], gs, "adamw" if adam else "lamb", 1.0)
    flat = torch.zeros(sum(e[0] for e in ent) + 2 * GUARD, dtype=torch.float32, device=DEV)
    views, off = [], GUARD
    for p in order:
        views.append(flat[off:off + p.numel()].view_as(p))
        off += p.numel()
    assert sum(v.data_ptr() % 16 != 0 for v in views) >= len(views) // 2
    pad = torch.ones(opt.m.numel(), dtype=torch.bool)
    for p, o in zip(order, opt._offs):
        pad[o:o + p.numel()] = False
    assert int(pad.sum()) > 0
    for s in range(3):
        for p, v, g in zip(order, views, gs[s]):
            v.copy_(g.view_as(v))
            p.grad = v
        opt.step()
        torch.cuda.synchronize()
        assert all(p.grad.data_ptr() == v.data_ptr() for p, v in zip(order, views)), "step() replaced a gradient view"
        assert abs(float(opt.last_grad_norm) - want[s]["gn"]) <= 1e-5 * want[s]["gn"]
        emas = opt.ema_state()
        for i, p in enumerate(order):
            for have, ref in ((p, want[s]["p"][i]), (emas[i], want[s]["ema"][i])):
                assert np.allclose(have.detach().cpu().reshape(-1).double().numpy(), ref, rtol=2e-5, atol=1e-6), f"step {s}, tensor {i}"
            ref = want[s]["u"][i]
            err = np.abs(views[i].cpu().reshape(-1).double().numpy() - ref).max()
            assert err <= 2e-5 * np.abs(ref).max(), f"step {s}, tensor {i}: the gradient view does not hold u"
            o = opt._offs[i]
            for name, state in (("m", opt.m), ("v", opt.v)):
                ref = want[s][name][i]
                err = np.abs(state[o:o + p.numel()].cpu().double().numpy() - ref).max()
                assert err <= 2e-5 * np.abs(ref).max(), f"step {s}, tensor {i}: {name}"
        for name, state in (("m", opt.m), ("v", opt.v), ("ema", opt.ema)):
            if state is not None:
                assert not state.cpu()[pad].view(torch.int32).any(), f"step {s}: pad elements of opt.{name} were written"
        assert not flat[:GUARD].view(torch.int32).any() and not flat[-GUARD:].view(torch.int32).any()
    assert opt.skipped_steps == 0
