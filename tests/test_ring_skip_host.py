"""Host side of the ring kernel's stochastic-depth mask (no GPU): the item order of a masked launch through the kernel's own
mapping function (csrc/gemm.hip ring_item_masked, asked through octic_linear_d8_ring_order_dropped), the refusals of
octic_linear_d8_fwd_dropped that need no device, the OCTIC_RING_SKIP switch and the prototypes."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("octic_linear_d8_fwd_dropped", "octic_linear_d8_ring_order_dropped")
ESHAPE = -1


def _order(m_tiles, n_chunks, dead_long, dead_short):
    """[(group, item, dead)] per workgroup in blockIdx order."""
    from octic_vits_amd import _lib
    raw = _lib.lib()
    n = sum(m * c for m, c in zip(m_tiles, n_chunks))
    arr = lambda v: (ctypes.c_int * len(v))(*v)
    flags = lambda v: (ctypes.c_ubyte * len(v))(*[int(bool(f)) for f in v])
    og, oi, od = (ctypes.c_int * n)(), (ctypes.c_int * n)(), (ctypes.c_int * n)()
    ksteps = [20] + [10] * (len(m_tiles) - 1)
    got = raw.octic_linear_d8_ring_order_dropped(len(m_tiles), arr(m_tiles), arr(ksteps), 64, arr(n_chunks), flags(dead_long),
                                                 flags(dead_short), og, oi, od)
    assert got == n, got
    return list(zip(og, oi, od))


# (m-tiles per group, n-chunks per group): ViT-H's long-K launch (514 + 4 x 129 items, 64 slots per XCD), the narrow tile of a
# ViT-L-like layer (three and two chunks per m-tile), a launch under 16 items (no dispatch plan; too few rounds to keep a long
# m-tile's chunks on one XCD: the plain list), one m-tile per group, and a long group that is a multiple of eight
SHAPES = [([257, 129, 129, 129, 129], [2, 1, 1, 1, 1]),
          ([197, 99, 99, 99, 99], [3, 2, 2, 2, 2]),
          ([2, 1, 1, 1, 1], [3, 2, 2, 2, 2]),
          ([1, 1, 1, 1, 1], [1, 1, 1, 1, 1]),
          ([64, 32, 32], [2, 1, 1])]


def _masks(rng, n_long, n_short):
    yield [0] * n_long, [0] * n_short                                  # all live
    yield [1] * n_long, [1] * n_short                                  # all dead
    yield [1] * n_long, [0] * n_short                                  # (flags are per group: the mapping does not couple them)
    yield [i & 1 for i in range(n_long)], [(i + 1) & 1 for i in range(n_short)]
    for _ in range(6):
        p = rng.uniform(0.1, 0.9)
        yield list(rng.random(n_long) < p), list(rng.random(n_short) < p)


@pytest.mark.parametrize("m_tiles,n_chunks", SHAPES)
def test_masked_order(m_tiles, n_chunks):
    rng = np.random.default_rng(sum(m_tiles))
    n = sum(m * c for m, c in zip(m_tiles, n_chunks))
    want = {(g, i) for g, (m, c) in enumerate(zip(m_tiles, n_chunks)) for i in range(m * c)}
    nc0, ncs = n_chunks[0], n_chunks[1]
    colocated = -(-m_tiles[0] // 8) * nc0 <= n // 8
    for dead_long, dead_short in _masks(rng, m_tiles[0], m_tiles[1]):
        order = _order(m_tiles, n_chunks, dead_long, dead_short)
        # every item runs exactly once, and the mapping's idea of dead is the flags'
        assert len(order) == n and {(g, i) for g, i, _ in order} == want
        for g, i, d in order:
            assert d == int(bool(dead_long[i // nc0] if g == 0 else dead_short[i // ncs])), (g, i)
        live_long, live_short, live_all = [], [], []
        for x in range(8):
            mine = order[x::8]
            # live before dead, long before short among the live
            rank = [2 if d else (0 if g == 0 else 1) for g, _, d in mine]
            assert rank == sorted(rank), x
            live_long.append(rank.count(0))
            live_short.append(rank.count(1))
            live_all.append(rank.count(0) + rank.count(1))
            if colocated:
                # the n-chunks of a long m-tile are consecutive workgroups of this XCD
                longs = [i for g, i, d in mine if g == 0 and not d]
                assert len(longs) % nc0 == 0
                for k in range(0, len(longs), nc0):
                    assert longs[k:k + nc0] == list(range(longs[k], longs[k] + nc0)) and longs[k] % nc0 == 0
        # shared evenly: within one m-tile of each other (a long m-tile is nc0 items; an XCD with one long m-tile fewer takes
        # that many short items more, so the totals differ by one item)
        assert max(live_long) - min(live_long) <= nc0
        assert max(live_short) - min(live_short) <= max(nc0, 1) + 1
        assert max(live_all) - min(live_all) <= max(nc0, 1)


def test_vit_h_counts():
    """ViT-H: 1030 workgroups; with every other sample-sized run of tiles dead each XCD gets an eighth of the live work."""
    m_tiles, n_chunks = [257, 129, 129, 129, 129], [2, 1, 1, 1, 1]
    dead_long = [(i // 4) & 1 for i in range(257)]
    dead_short = [(i // 2) & 1 for i in range(129)]
    order = _order(m_tiles, n_chunks, dead_long, dead_short)
    assert len(order) == 1030
    ll = 2 * dead_long.count(0)
    ls = 4 * dead_short.count(0)
    for x in range(8):
        mine = order[x::8]
        assert abs(sum(1 for g, _, d in mine if g == 0 and not d) - ll / 8) <= 2
        assert abs(sum(1 for g, _, d in mine if not d) - (ll + ls) / 8) <= 1


def test_order_refuses_what_the_masked_kernel_does_not_take():
    from octic_vits_amd import _lib
    raw = _lib.lib()
    arr = lambda v: (ctypes.c_int * len(v))(*v)
    z = (ctypes.c_ubyte * 4096)()
    out = (ctypes.c_int * 8192)()
    call = lambda items: raw.octic_linear_d8_ring_order_dropped(len(items), arr(items), arr([2] * len(items)), 64, None, z, z, out,
                                                                out, None)
    assert call([100, 30, 20]) == ESHAPE                               # unequal short groups
    assert call([64]) == ESHAPE                                        # no short group
    assert call([1025, 513]) == ESHAPE                                 # past the bitmap cap
    assert call([1024, 512, 512]) == 2048


def _view(c):
    from octic_vits_amd import _lib
    v = _lib.OcticView()
    for i in range(5):
        v.ptr[i] = 4096                                                # never dereferenced: every call below is refused first
        v.ld[i] = c if i < 4 else 4 * c
    return v


def test_entry_point_refusals():
    """octic_linear_d8_fwd_dropped returns OCTIC_ESHAPE before it looks at a pointer."""
    from octic_vits_amd import _lib
    raw = _lib.lib()
    M, cin, cout = 6 * 37, 64, 32
    x, y = _view(cin), _view(cout)
    p = ctypes.c_void_p(4096)
    w = (ctypes.c_void_p * 5)(*[4096] * 5)

    def call(bias=None, resid=None, rs=None, rps=0, cs=None, dropped=p, drps=37, m=M):
        return raw.octic_linear_d8_fwd_dropped(ctypes.byref(x), w, bias, ctypes.byref(y), ctypes.byref(resid) if resid else None, rs,
                                               rps, cs, m, cin, cout, _lib.BF16, _lib.BF16, dropped, drps, None)

    assert call(bias=p) == ESHAPE                                      # plain launch with a bias
    assert call(drps=0) == ESHAPE
    assert call(drps=36) == ESHAPE                                     # M % dropped_rows_per_sample != 0
    assert call(resid=y, rs=None) == ESHAPE                            # fused without rs
    assert call(rs=p, rps=37) == ESHAPE                                # ... without a residual
    assert call(cs=w) == ESHAPE
    assert call(resid=y, rs=p, rps=74, drps=37) == ESHAPE              # the two masks count different rows per sample


def test_switch_reads_the_environment(monkeypatch):
    import octic_vits_amd.functional as OF
    monkeypatch.delenv("OCTIC_RING_SKIP", raising=False)
    assert OF._skip_from_env("OCTIC_RING_SKIP") is True
    monkeypatch.setenv("OCTIC_RING_SKIP", "0")
    assert OF._skip_from_env("OCTIC_RING_SKIP") is False
    assert isinstance(OF.RING_SKIP_DROPPED, bool)

    class Factors:
        is_cuda, dtype = True, torch.float32
        dim = lambda self: 1
        numel = lambda self: 3
        is_contiguous = lambda self: True
        detach = lambda self: self

    f = Factors()
    monkeypatch.setattr(OF, "LINEAR_SKIP_DROPPED", True)
    monkeypatch.setattr(OF, "RING_SKIP_DROPPED", True)
    assert OF.ring_skip_scale(f, 17, 51) is f
    assert OF.ring_skip_scale(f, 17, 52) is None
    monkeypatch.setattr(OF, "RING_SKIP_DROPPED", False)
    assert OF.ring_skip_scale(f, 17, 51) is None and OF.linear_skip_scale(f, 17, 51) is f    # a switch of its own
    monkeypatch.setattr(OF, "RING_SKIP_DROPPED", True)
    monkeypatch.setattr(OF, "LINEAR_SKIP_DROPPED", False)
    assert OF.ring_skip_scale(f, 17, 51) is None                       # effective only while the linear skip is on


def test_prototypes_abi_and_exports():
    from octic_vits_amd import _lib
    header = open(os.path.join(ROOT, "include", "octic_hip.h")).read()
    assert f"#define OCTIC_ABI_VERSION {_lib.ABI_VERSION}" in header      # additions only: the number stays
    so = os.path.join(ROOT, "octic_vits_amd", "liboctic_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (octic_\w+)", out))
    for name in NEW:
        assert name in _lib._PROTOS and name in exported
        assert re.search(r"\bint " + name + r"\(", header), name
    assert _lib._PROTOS[NEW[0]][1] == _lib._PROTOS["octic_linear_d8_fwd_skip"][1]
