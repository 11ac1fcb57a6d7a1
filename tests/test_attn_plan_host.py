"""Which kernel an attention shape runs: octic_attn_plan - the library's one routing function (attn_plan, csrc/attention.hip),
the one the entry points launch from - against the table below, written out for every T in 1 .. 320 at each of the eight
head_dims (bf16, contiguous heads), under the default routing and under each attention route knob.  No GPU needed.

The table is the record of what each shape runs; tests/test_attn_resident_gpu.py takes its test ids and its coverage check
from it.  Importing this module does not need the built library."""
import pytest

HDS = (16, 32, 48, 64, 80, 96, 112, 128)
# kernel ids of include/octic_hip.h (OCTIC_ATTN_FWD_* / OCTIC_ATTN_BWD_*)
PERSIST, A80_ONESHOT, A80_ONLINE, RESIDENT, FWD_STREAM, FWD_F32 = range(6)
SINGLE, PAIR, BWD_STREAM, BWD_F32 = range(4)
F32, BF16 = 0, 1
STREAM_WAVES = 4

# head_dims -> rows (first T, last T, kernel, waves per workgroup), the first row that holds T counts.  nt = ceil(T / 32) tiles;
# waves: a number, "nt", "min8" = min(nt, 8), "max4" = max(4, nt).
_FWD_TAIL = [(259, 288, RESIDENT, 9), (289, 320, RESIDENT, 10)]
FWD = {
    (16, 32, 48, 64): [(1, 258, PERSIST, "min8")] + _FWD_TAIL,
    (80,): [(1, 256, A80_ONESHOT, "max4"), (257, 258, A80_ONESHOT, 8)] + _FWD_TAIL,
    (96,): [(1, 256, PERSIST, "min8"), (257, 288, RESIDENT, 9), (289, 320, RESIDENT, 10)],
    (112,): [(1, 27, PERSIST, "min8"), (33, 54, PERSIST, "min8"), (65, 82, PERSIST, "min8"), (97, 109, PERSIST, "min8"),
             (129, 137, PERSIST, "min8"), (161, 164, PERSIST, "min8"), (1, 256, RESIDENT, "nt"), (257, 288, RESIDENT, 9),
             (289, 320, FWD_STREAM, STREAM_WAVES)],
    (128,): [(1, 256, RESIDENT, "nt"), (257, 320, FWD_STREAM, STREAM_WAVES)],
}
_BWD_64 = [(1, 256, PAIR, "nt"), (257, 288, PAIR, 8), (289, 320, PAIR, 10)]          # 257 .. 288: eight waves share the ninth tile
BWD = {
    (16, 32, 48, 64, 96): _BWD_64,
    (80,): [(1, 32, SINGLE, 1), (33, 64, SINGLE, 2), (65, 192, PAIR, "nt"), (193, 257, SINGLE, 8), (258, 288, PAIR, 8),
            (289, 320, PAIR, 10)],
    (112, 128): [(1, 256, PAIR, "nt"), (257, 320, BWD_STREAM, STREAM_WAVES)],
}
# the route knobs (octic_route_override = 1); what a knob does not name stays as above
KNOBS = ("STREAM", "LEGACY", "BWD_PAIR", "ONLINE")
FWD_KNOB = {
    "LEGACY": {(80,): [(1, 257, PERSIST, "min8"), (258, 288, RESIDENT, 9), (289, 320, RESIDENT, 10)]},
    "ONLINE": {(80,): [(1, 258, A80_ONLINE, "min8")] + _FWD_TAIL},
}
BWD_KNOB = {"LEGACY": {(80,): _BWD_64}, "BWD_PAIR": {(80,): _BWD_64}}


def _lookup(table, T, hd):
    nt = (T + 31) // 32
    (rows,) = [r for hds, r in table.items() if hd in hds]
    lo, hi, kernel, waves = next(r for r in rows if r[0] <= T <= r[1])
    return kernel, {"nt": nt, "min8": min(nt, 8), "max4": max(4, nt)}.get(waves, waves)


def expected(T, hd, knob=None):
    """(forward kernel, forward waves, phase-3 backward choice, backward waves) of a bf16 shape with contiguous heads."""
    if T > 320 or knob == "STREAM":
        return FWD_STREAM, STREAM_WAVES, BWD_STREAM, STREAM_WAVES
    fwd = {**FWD, **FWD_KNOB.get(knob, {})}
    bwd = {**BWD, **BWD_KNOB.get(knob, {})}
    return _lookup(fwd, T, hd) + _lookup(bwd, T, hd)


def labels(T, hd, knob=None):
    """Short names of the two choices (the ids of the sweep of tests/test_attn_resident_gpu.py): the kernel, and the
    instantiation where a kernel has more than one."""
    fwd, fw, bwd, bw = expected(T, hd, knob)
    nt = (T + 31) // 32
    f = {PERSIST: "persist", A80_ONESHOT: "attn80", A80_ONLINE: "attn80", FWD_STREAM: "stream",
         RESIDENT: "fwd512" if fw <= 8 else "fwd640w%d" % fw}[fwd]
    b = {SINGLE: "attn80_bwd", BWD_STREAM: "stream", PAIR: "pair512" if nt <= 8 else "pair512tile9" if nt == 9 else "pair640"}[bwd]
    return f, b


def _knob_id(lib, knob):
    return getattr(lib, "ROUTE_ATTN_" + knob)


def _plan(T, hd, dtype=BF16, ld=0):
    from octic_vits_amd import _lib
    return _lib.attn_plan(T, hd, dtype, ld, ld, ld)


def test_ids_match_the_header():
    import re
    from octic_vits_amd import _lib
    text = open(_lib.HEADER_PATH).read()
    for name, value in (("FWD_PERSIST", PERSIST), ("FWD_A80_ONESHOT", A80_ONESHOT), ("FWD_A80_ONLINE", A80_ONLINE),
                        ("FWD_RESIDENT", RESIDENT), ("FWD_STREAM", FWD_STREAM), ("FWD_F32", FWD_F32), ("BWD_SINGLE", SINGLE),
                        ("BWD_PAIR", PAIR), ("BWD_STREAM", BWD_STREAM), ("BWD_F32", BWD_F32)):
        assert int(re.search(r"OCTIC_ATTN_%s = (\d+)" % name, text).group(1)) == value == getattr(_lib, "ATTN_" + name), name
    assert (_lib.F32, _lib.BF16) == (F32, BF16)


@pytest.mark.parametrize("hd", HDS)
def test_plan_matches_the_table_at_every_token_count(hd):
    bad = [(T, _plan(T, hd), expected(T, hd)) for T in range(1, 321) if _plan(T, hd) != expected(T, hd)]
    assert not bad, bad[:8]


@pytest.mark.parametrize("knob", KNOBS)
def test_plan_matches_the_table_under_each_knob(knob):
    from octic_vits_amd import _lib
    try:
        assert _lib.route_override(_knob_id(_lib, knob), 1) == 0
        bad = [(T, hd, _plan(T, hd), expected(T, hd, knob)) for hd in HDS for T in range(1, 321)
               if _plan(T, hd) != expected(T, hd, knob)]
        f32 = {_plan(T, hd, F32) for hd in HDS for T in (1, 257, 320, 321)}
    finally:
        _lib.route_override(_knob_id(_lib, knob), 0)
    assert not bad, bad[:8]
    assert f32 == {(FWD_F32, 4, BWD_F32, 4)}
    assert _plan(257, 80) == expected(257, 80)                      # the knob is back at 0


def test_knobs_change_what_the_table_says_they_change():
    """The knob rows differ from the default ones where the issue says so (a table whose knob rows were copies of the default
    would let a dead knob pass)."""
    assert labels(257, 80, "LEGACY") == ("persist", "pair512tile9") and labels(258, 80, "LEGACY")[0] == "fwd640w9"
    assert labels(257, 80, "BWD_PAIR") == ("attn80", "pair512tile9") and labels(37, 80, "BWD_PAIR")[1] == "pair512"
    assert expected(257, 80, "ONLINE")[:2] == (A80_ONLINE, 8) and expected(37, 80, "ONLINE")[:2] == (A80_ONLINE, 2)
    assert expected(257, 80)[:2] == (A80_ONESHOT, 8) and expected(37, 80)[:2] == (A80_ONESHOT, 4)
    assert expected(64, 80)[2:] == (SINGLE, 2) and expected(32, 80)[2:] == (SINGLE, 1)


def test_long_sequences_stream_and_bad_shapes_are_rejected():
    from octic_vits_amd import _lib
    for hd in HDS:
        for T in (321, 16384):
            assert _plan(T, hd) == (FWD_STREAM, STREAM_WAVES, BWD_STREAM, STREAM_WAVES), (T, hd)
            assert _plan(T, hd, F32) == (FWD_F32, 4, BWD_F32, 4), (T, hd)
        assert _plan(257, hd, F32) == (FWD_F32, 4, BWD_F32, 4)
    out = (_lib.c_int * 4)()
    for dtype in (BF16, F32):
        for T, hd in ((16385, 64), (257, 72), (257, 144), (0, 64), (257, 0)):
            assert _lib.lib().octic_attn_plan(dtype, T, hd, 0, 0, 0, out) == -1, (dtype, T, hd)     # OCTIC_ESHAPE
    assert _lib.lib().octic_attn_plan(BF16, 257, 80, 0, 0, 0, None) == -4                           # OCTIC_ENULL


def test_entry_points_reject_the_shapes_the_plan_rejects():
    """One validation: a (T, hd) is OCTIC_ESHAPE for octic_attn_plan exactly where it is for the entry points (checked before
    any launch, so no GPU is touched)."""
    from octic_vits_amd import _lib
    L = _lib.lib()
    out = (_lib.c_int * 4)()
    p = 4096
    for T, hd in ((16385, 64), (257, 72), (257, 144), (0, 64), (257, 64), (16384, 128), (1, 16)):
        want = L.octic_attn_plan(BF16, T, hd, 0, 0, 0, out)
        # misaligned q: a shape the plan takes gets as far as the alignment check (-2), a rejected one stops before it (-1)
        got = L.octic_attn_fwd(p + 2, p, p, p, None, 1, 1, T, hd, T * hd, T * hd, hd, T * hd, T * hd, hd, 0.125, None)
        assert (want, got) in ((0, -2), (-1, -1)), (T, hd, want, got)
        got = L.octic_attn_bwd(p + 2, p, p, p, p, p, p, p, p, p, 1, 1, T, hd, *([T * hd, T * hd, hd] * 3), 0.125, 3, None)
        assert (want, got) in ((0, -2), (-1, -1)), (T, hd, want, got)
        got = L.octic_attn_fwd_f32(p + 2, p, p, p, None, 1, 1, T, hd, T * hd, T * hd, hd, T * hd, T * hd, hd, 0.125, None)
        assert (L.octic_attn_plan(F32, T, hd, 0, 0, 0, out), got) in ((0, -2), (-1, -1)), (T, hd, got)


def test_strides_beyond_32_bit_offsets_leave_the_dma_kernels():
    """head_dim 80, 257 tokens, token stride 4 200 000 elements: 257 x 4.2 M x 2 B is past the 32-bit buffer offsets of
    the head_dim-80 kernels and of the persistent forward's K DMA - nine waves of attn_fwd_kernel, the dq + dkv pair."""
    assert 257 * 4_200_000 * 2 >= 0x7FFFFFF0 > 256 * 4_100_000 * 2
    assert _plan(257, 80, ld=4_200_000) == (RESIDENT, 9, PAIR, 8)
    assert _plan(257, 80, ld=4_100_000) == expected(257, 80)        # (just inside: the default plan)
    assert _plan(257, 80, ld=80) == _plan(257, 80, ld=0)            # 0 = contiguous heads
