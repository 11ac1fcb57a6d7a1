"""TEST INFRASTRUCTURE — the inputs of the optimizer-step edge tests, shared by tests/test_lamb_oracle.py (train.Lamb on the
CPU) and tests/test_lamb_kernels_gpu.py (csrc/lamb.hip through the C ABI), so that both run the very same cases against
oracle/lamb_ref.py.  Everything is a list of f32 CPU tensors, one per optimizer tensor; nothing here computes an update."""
import torch

CHUNK = 65536        # train.FusedLamb.CHUNK (the GPU harness asserts that they agree)
LR, WD = 3e-3, 0.02

# every length at which csrc/lamb.hip changes path: the scalar tails n % 4 = 0..3 without and with a vector body, the
# block-stride edges of 256 threads (x 4 elements), one chunk -1 / exact / +1, two chunks exact / +1, three chunks + 5
SIZES = [1, 2, 3, 4, 5, 6, 7, 8, 255, 256, 257, 1023, 1024, 1025, 65535, 65536, 65537, 131072, 131073, 196613]


def matrix_entries():
    """(numel, wd, lr) of the size matrix: wd alternates between 0 and 0.02."""
    return [(n, 0.0 if i % 2 == 0 else WD, LR) for i, n in enumerate(SIZES)]


def matrix_inputs(steps=3):
    """Parameters and ``steps`` gradient lists: 5 * randn at the first step (clipped at max_grad_norm = 1), 0.1 * randn after."""
    gen = torch.Generator().manual_seed(5)
    ps = [torch.randn(n, generator=gen) for n in SIZES]
    gen = torch.Generator().manual_seed(11)
    gs = [[torch.randn(n, generator=gen) * (5.0 if s == 0 else 0.1) for n in SIZES] for s in range(steps)]
    return ps, gs


# the trust-ratio gate cases: index -> what the tensor is.  Ordinary tensors around them keep the global norm positive.
GATE_ZERO_P, GATE_ZERO_G_WD, GATE_ZERO_G, GATE_FAR, GATE_BEFORE, GATE_LAST_CHUNK, GATE_AFTER = 1, 3, 4, 5, 7, 8, 9
GATE_LAST_LEN = 300          # the non-zero part of the three-chunk tensor: the 300 elements of its last chunk


def gate_entries():
    return [(300, WD, LR),                          # 0  ordinary
            (261, WD, LR),                          # 1  p = 0, g != 0: |p| = 0 -> ratio 1
            (5, 0.0, LR),                           # 2  ordinary
            (1027, WD, LR),                         # 3  g = 0, p != 0: u = wd p, ratio 1 / wd -> p (1 - lr)
            (130, 0.0, LR),                         # 4  g = 0, wd = 0: nothing moves, m = v = 0
            (515, 0.0, LR),                         # 5  wd = 0, |p| / |u| ~ 1e3: ratio 1
            (7, WD, LR),                            # 6  ordinary
            (CHUNK + 4464, WD, LR),                 # 7  neighbour in front, |p| ~ 4 per element
            (2 * CHUNK + GATE_LAST_LEN, WD, LR),    # 8  three chunks, p (~ 1e-2 per element) and g non-zero in the last one only
            (1000, WD, LR),                         # 9  neighbour behind, |p| ~ 4 per element
            (7, 0.0, LR)]                           # 10 ordinary


def gate_inputs(all_grads_zero=False):
    """(parameters, gradients) of gate_entries().  The three-chunk tensor (8) has |p|^2 = |u|^2 = 0 in its first two chunks and
    |p|^2 ~ 0.03, |u|^2 ~ 300 in the last: ratio ~ 0.01.  The last chunk of the tensor in front of it carries |p|^2 ~ 7e4 and
    the only chunk of the one behind |p|^2 ~ 1.6e4, so a chunk range that starts one chunk early or ends one late makes the
    ratio ~ 3.5, and one that ends one early makes it 1 (|p| = 0).  The scales stay below 10 where weight decay is on: a
    LAMB step is ~ lr * rms(p) per element, and its f32 rounding has to stay small against the 1e-6 of the p bar."""
    gen = torch.Generator().manual_seed(17)
    ent = gate_entries()
    ps = [torch.randn(n, generator=gen) for n, _, _ in ent]
    gs = [torch.randn(n, generator=gen) for n, _, _ in ent]
    ps[GATE_ZERO_P].zero_()
    gs[GATE_ZERO_G_WD].zero_()
    gs[GATE_ZERO_G].zero_()
    ps[GATE_FAR] *= 1e3
    ps[GATE_BEFORE] *= 4.0
    ps[GATE_AFTER] *= 4.0
    ps[GATE_LAST_CHUNK] *= 1e-2
    ps[GATE_LAST_CHUNK][:2 * CHUNK] = 0
    gs[GATE_LAST_CHUNK][:2 * CHUNK] = 0
    if all_grads_zero:
        for g in gs:
            g.zero_()
    return ps, gs


def many_entries(ntensors):
    """Lengths cycle through 1..9, wd alternates starting with 0.02 (so tensor 256, the first one of the ratio kernel's second
    workgroup, has a trust ratio), every tensor its own lr: 3e-3 * (1 + frac(i * phi)) with phi the golden ratio's
    fractional part.  i * phi mod 1 never repeats and has no period: tensors 1, 2, 8 and 256 slots apart differ by 0.38,
    0.24, 0.056 and 0.22 of 3e-3 (frac(d * phi) or 1 minus it), and no two of 600 are closer than 1e-3 of it.  Without
    weight decay and in AdamW mode lr is the only per-tensor factor of the step, so it must not alias at any distance."""
    phi = (5.0 ** 0.5 - 1.0) / 2.0
    return [(1 + i % 9, WD if i % 2 == 0 else 0.0, LR * (1.0 + (i * phi) % 1.0)) for i in range(ntensors)]


def many_inputs(ntensors):
    """g is randn * 2^(3 - i % 7); every element of p of tensor i has a magnitude in [1, 1.25) * 2^(i % 11 - 5) and the sign of
    its gradient, so that the Adam term and wd * p never cancel in u (in a tensor of one or two elements a cancelled u
    would put f32 rounding at the tensor's whole scale; this case is about indices, not conditioning).  With weight decay
    the trust ratio |p| / |u| at the first step (Adam term ~ 1 per element) follows rms(p), so it differs from that of the
    decayed tensors next to it (i +- 2: a factor of 4 or 512 in scale) and from that of tensor i +- 256 (256 % 11 = 3: a
    factor of 8 or 256) by a factor of two or more, and so does lr * ratio."""
    gen = torch.Generator().manual_seed(23)
    ent = many_entries(ntensors)
    gs = [torch.randn(n, generator=gen) * 2.0 ** (3 - i % 7) for i, (n, _, _) in enumerate(ent)]
    ps = [torch.sign(g) * (1.0 + 0.25 * torch.rand(g.shape, generator=gen)) * 2.0 ** (i % 11 - 5) for i, g in enumerate(gs)]
    return ps, gs
