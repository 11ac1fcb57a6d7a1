"""CPU-only: the row kernels of csrc/dense.hip refuse bad arguments before any launch, their slab plans have the edges
tests/test_dense_rows_matrix_gpu.py runs rows around, and that file's shape tables reach every template instance of every
routing branch.  Every pointer is a dummy that is never dereferenced, and every call here carries exactly one reason to
refuse it (or no rows): no call reaches a launch.  So that the fused LayerNorm-backward tail ACCEPTS a width cannot be
seen here (its pointer checks come first and a call with good pointers and a good width would launch): the refusals are
asserted for every other width of the tables, and the GPU file launches every accepted one.
"""
import ctypes
import os
import re

import pytest
import torch

from octic_vits_amd import _lib

P = 4096                                   # a 16-byte aligned, never dereferenced address
F32, BF16 = _lib.F32, _lib.BF16


def _codes():
    """OCTIC_* error codes by name, from include/octic_hip.h."""
    with open(_lib.HEADER_PATH) as f:
        return {k: int(v) for k, v in re.findall(r"\b(OCTIC_(?:OK|E[A-Z]+))\s*=\s*(-?\d+)", f.read())}


C = _codes()
OK, ESHAPE, EALIGN, EDTYPE, ENULL = (C[k] for k in ("OCTIC_OK", "OCTIC_ESHAPE", "OCTIC_EALIGN", "OCTIC_EDTYPE", "OCTIC_ENULL"))

# entry point -> ordered arguments with a well-formed default (d = 256 is a width every one of them takes)
_LN_FWD = dict(x=P, y=P, y_dtype=BF16, w=P, b=P, stats=P, rows=8, d=256, eps=1e-6)
_RESID = dict(x=P, yb=P, yb_dtype=BF16, gamma=P, rs=None, rows_per_scale=1, xout=P, y=P, y_dtype=BF16, w=P, b=P, stats=P,
              rows=8, d=256, eps=1e-6)
_LN_BWD = dict(gy=P, g_dtype=BF16, x=P, w=P, stats=P, dres=P, dx=P, partials=P, rows=8, d=256)
_TAIL = dict(gy=P, x=P, w=P, stats=P, dres=P, dx=P, partials=P, yb=P, gamma=P, rs=None, rows_per_scale=1, gyb=P, partials2=P,
             rows=8, d=256)
_SR_FWD = dict(x=P, y=P, y_dtype=BF16, gamma=P, rs=None, rows_per_scale=1, out=P, rows=8, d=256)
_SR_BWD = dict(gout=P, y=P, y_dtype=BF16, gamma=P, rs=None, rows_per_scale=1, gy=P, partials=P, rows=8, d=256)
SPECS = {
    "octic_dense_layernorm_fwd": dict(_LN_FWD, stream=None),
    "octic_dense_layernorm_fwd_rows": dict(_LN_FWD, rowmap=P, xcopy=P, stream=None),
    "octic_dense_resid_layernorm_fwd": dict(_RESID, stream=None),
    "octic_dense_layernorm_bwd": dict(_LN_BWD, stream=None),
    "octic_dense_layernorm_bwd_rows": dict(_LN_BWD, rowmap=P, stream=None),
    "octic_dense_layernorm_bwd_tail": dict(_TAIL, stream=None),
    "octic_dense_layernorm_bwd_tail_skip": dict(_TAIL, sample_scale=None, rows_per_sample=0, stream=None),
    "octic_scale_residual_fwd": dict(_SR_FWD, stream=None),
    "octic_scale_residual_fwd_rows": dict(_SR_FWD, rowmap=P, stream=None),
    "octic_scale_residual_bwd": dict(_SR_BWD, stream=None),
    "octic_scale_residual_bwd_rows": dict(_SR_BWD, rowmap=P, stream=None),
}
REQUIRED = {
    "octic_dense_layernorm_fwd": ("x", "y", "stats"),
    "octic_dense_layernorm_fwd_rows": ("x", "y", "stats"),
    "octic_dense_resid_layernorm_fwd": ("x", "yb", "xout", "y", "stats"),
    "octic_dense_layernorm_bwd": ("gy", "x", "stats", "dx"),
    "octic_dense_layernorm_bwd_rows": ("gy", "x", "stats", "dx"),
    "octic_dense_layernorm_bwd_tail": ("gy", "x", "stats", "dx", "yb", "gyb"),
    "octic_dense_layernorm_bwd_tail_skip": ("gy", "x", "stats", "dx", "yb", "gyb"),
    "octic_scale_residual_fwd": ("x", "y", "out"),
    "octic_scale_residual_fwd_rows": ("x", "y", "out"),
    "octic_scale_residual_bwd": ("gout", "gy", "y"),              # y: required with partials
    "octic_scale_residual_bwd_rows": ("gout", "gy", "y"),
}
POINTERS = {"x", "y", "w", "b", "stats", "yb", "gamma", "rs", "xout", "gy", "dres", "dx", "partials", "gyb", "partials2", "out",
            "gout", "rowmap", "xcopy", "sample_scale"}
ROW_KERNELS = sorted(SPECS)
COLUMN_SPECS = {
    "octic_dense_colsum": dict(g=P, rows=8, d=64, ld=72, partials=P, stream=None),
    "octic_dense_colsum_skip": dict(g=P, rows=8, d=64, ld=72, partials=P, sample_scale=None, rows_per_sample=0, stream=None),
    "octic_dense_gelu_bwd": dict(h=P, g=P, dh=P, partials=P, rows=8, d=64, stream=None),
}


def call(name, **kw):
    spec = SPECS.get(name) or COLUMN_SPECS[name]
    assert not set(kw) - set(spec), (name, kw)
    assert kw, "a well-formed call would launch"
    args = dict(spec, **kw)
    return getattr(_lib.lib(), name)(*args.values())


def test_every_entry_point_is_declared_and_bound():
    declared = _lib.header_symbols()
    L = _lib.lib()
    for name in list(SPECS) + list(COLUMN_SPECS) + ["octic_dense_blocks", "octic_dense_gelu_blocks", "octic_dense_finish",
                                                   "octic_dense_finish_batch"]:
        assert name in declared and name in _lib._PROTOS and hasattr(L, name), name
    for name, spec in {**SPECS, **COLUMN_SPECS}.items():
        assert len(spec) == len(_lib._PROTOS[name][1]), name


def test_slab_plans():
    L = _lib.lib()
    assert [L.octic_dense_blocks(r) for r in (0, 1, 16, 17, 4096, 4097, 1 << 40)] == [1, 1, 1, 2, 256, 256, 256]
    assert L.octic_dense_gelu_blocks() == 256          # the colsum / gelu_bwd row tables of the GPU file rest on it


@pytest.mark.parametrize("name", ROW_KERNELS)
def test_row_kernels_refuse_bad_arguments(name):
    for d in (0, -4, 6, 2052):
        assert call(name, d=d) == ESHAPE, d
    assert call(name, rows=-1) == ESHAPE
    for k in SPECS[name]:
        if k.endswith("_dtype"):
            assert call(name, **{k: 7}) == EDTYPE, k
    for k in REQUIRED[name]:
        assert call(name, **{k: None}) == ENULL, k
    if "rs" in SPECS[name]:
        assert call(name, rs=P, rows_per_scale=0) == ESHAPE
        assert call(name, rs=P, rows_per_scale=-3) == ESHAPE
    if "bwd" in name and "scale_residual" in name:     # y is nullable without partials only
        assert call(name, y=None, partials=None, d=6) == ESHAPE


@pytest.mark.parametrize("name", ROW_KERNELS)
def test_row_kernels_accept_no_rows_before_their_pointer_checks(name):
    null = {k: None for k in SPECS[name] if k in POINTERS}
    assert call(name, rows=0, **null) == OK


def test_tail_kernel_checks_its_mask_first_and_takes_whole_chunks_only():
    name = "octic_dense_layernorm_bwd_tail_skip"
    assert call(name, rows=0, sample_scale=P, rows_per_sample=0) == ESHAPE          # the mask's shape: before rows == 0
    assert call(name, rows=0, sample_scale=P, rows_per_sample=-1) == ESHAPE
    assert call(name, rows=0, sample_scale=P, rows_per_sample=3) == OK
    assert call(name, rows=6, sample_scale=P, rows_per_sample=4, gy=None) == ESHAPE   # 6 % 4: refused before the pointers
    assert call(name, rows=6, sample_scale=P, rows_per_sample=3, gy=None) == ENULL    # accepted: on to the pointers
    assert call(name, rows=6, sample_scale=None, rows_per_sample=4, gy=None) == ENULL # no mask, no shape to check
    for entry in ("octic_dense_layernorm_bwd_tail", name):
        for d in (260, 1536, 2048):
            assert call(entry, d=d) == ESHAPE, d


def test_ops_predicate_agrees_with_the_tail_kernel():
    from octic_vits_amd import ops
    import test_dense_rows_matrix_gpu as M
    bf, f32 = torch.empty(0, dtype=torch.bfloat16), torch.empty(0)
    for d in M.WIDTHS:
        takes = d in M.TAIL_WIDTHS
        assert ops.dense_ln_bwd_tail_ok(bf, bf, d) == takes, d
        assert not ops.dense_ln_bwd_tail_ok(f32, bf, d) and not ops.dense_ln_bwd_tail_ok(bf, f32, d), d
        if not takes:
            assert call("octic_dense_layernorm_bwd_tail", d=d) == ESHAPE, d


def test_column_kernels_refuse_bad_arguments():
    for name in ("octic_dense_colsum", "octic_dense_colsum_skip"):
        assert call(name, d=12, ld=16) == ESHAPE               # d % 8
        assert call(name, d=0) == ESHAPE
        assert call(name, ld=68) == ESHAPE                     # ld % 8
        assert call(name, ld=56) == ESHAPE                     # ld < d
        assert call(name, rows=0) == ESHAPE
        assert call(name, rows=-1) == ESHAPE
        assert call(name, g=P + 8) == EALIGN
        assert call(name, g=None) == ENULL
        assert call(name, partials=None) == ENULL
        assert call(name, rows=0, g=None, partials=None) == ENULL   # no rows is a refusal here, and comes after the pointers
    assert call("octic_dense_colsum_skip", sample_scale=P, rows_per_sample=0) == ESHAPE
    assert call("octic_dense_colsum_skip", sample_scale=P, rows_per_sample=3) == ESHAPE          # 8 % 3
    name = "octic_dense_gelu_bwd"
    assert call(name, d=12) == ESHAPE
    assert call(name, d=0) == ESHAPE
    assert call(name, d=-8) == ESHAPE
    assert call(name, rows=-1) == ESHAPE
    for k in ("h", "g", "dh"):
        assert call(name, **{k: P + 8}) == EALIGN, k
        assert call(name, **{k: None}) == ENULL, k
    assert call(name, rows=0, h=None, g=None, dh=None, partials=None) == OK


def test_finish_refuses_bad_arguments():
    from octic_vits_amd import ops
    L = _lib.lib()
    assert L.octic_dense_finish(None, 4, 8, P, P, None, None) == ENULL
    for nblocks, d in ((0, 8), (-1, 8), (4, 0), (4, -8)):
        assert L.octic_dense_finish(P, nblocks, d, P, P, None, None) == ESHAPE, (nblocks, d)
    assert L.octic_dense_finish_batch(None, 1, None) == ENULL
    jobs = (ops._FinishJob * 3)()
    for j in jobs:
        j.partials, j.out0, j.out1, j.scale1, j.nblocks, j.d = P, P, P, None, 4, 8
    arr = ctypes.cast(jobs, ctypes.c_void_p)
    assert L.octic_dense_finish_batch(arr, -1, None) == ESHAPE
    for i in range(3):                                                               # a bad job anywhere refuses the batch
        for field, bad, want in (("partials", None, ENULL), ("nblocks", 0, ESHAPE), ("d", 0, ESHAPE), ("d", -4, ESHAPE)):
            keep = getattr(jobs[i], field)
            setattr(jobs[i], field, bad)
            assert L.octic_dense_finish_batch(arr, 3, None) == want, (i, field)
            setattr(jobs[i], field, keep)


# ------------------------------------------------------------------------------------- the GPU file's shape tables
# The routing rules of csrc/dense.hip, copied: a change of routing fails here and not on the GPU.
def nv(d):
    return (d + 255) // 256


def ln_bwd_route(d):
    return "wide" if d == 256 * nv(d) and nv(d) <= 6 else "predicated"


def resid_ln_fast(d):
    return nv(d) <= 6 and d == 256 * nv(d)


def scale_residual_bwd_fast(d):                      # (with partials; without them the predicated loop)
    return nv(d) <= 5 and d == 256 * nv(d)


def tail_takes(d):
    return d == 256 * nv(d) and nv(d) <= 5


def test_shape_tables_reach_every_instance():
    import test_dense_rows_matrix_gpu as M
    assert M.WHOLE == (256, 512, 768, 1024, 1280, 1536, 1792, 2048)
    assert sorted(M.EDGE) == [4, 252, 260, 508, 516, 764, 772, 1020, 1028, 1276, 1284, 1532, 1540, 1788, 1796, 2044]
    assert set(M.WIDTHS) == set(M.WHOLE) | set(M.EDGE) | {384} and all(d % 4 == 0 and 0 < d <= 2048 for d in M.WIDTHS)
    every = set(range(1, 9))
    # width sweep: each instance with every lane live, with one lane and with all lanes but one in the last chunk
    for widths in (M.WHOLE, [d for d in M.EDGE if d % 256 == 4], [d for d in M.EDGE if d % 256 == 252]):
        assert {nv(d) for d in widths} == every
    sweep = {d for r, d in M.LN_CASES if r == M.SWEEP_ROWS}
    assert sweep == set(M.WIDTHS)
    assert {nv(d) for d in sweep if ln_bwd_route(d) == "predicated"} == every        # LayerNorm fwd (one kernel) and bwd
    assert {nv(d) for d in sweep if ln_bwd_route(d) == "wide"} == set(range(1, 7))
    assert {d for d in sweep if ln_bwd_route(d) == "predicated" and d % 256 == 0} == {1792, 2048}
    sweep = {d for r, d in M.RESID_LN_CASES if r == M.SWEEP_ROWS}
    assert {nv(d) for d in sweep if resid_ln_fast(d)} == set(range(1, 7)) and {nv(d) for d in sweep if not resid_ln_fast(d)} == every
    sweep = {d for r, k, d in M.SCALE_RESIDUAL_CASES if r == M.SWEEP_ROWS}
    assert {nv(d) for d in sweep if scale_residual_bwd_fast(d)} == set(range(1, 6))
    assert {nv(d) for d in sweep if not scale_residual_bwd_fast(d)} == every
    assert [d for d in M.WIDTHS if tail_takes(d)] == list(M.TAIL_WIDTHS) and {nv(d) for d in M.TAIL_WIDTHS} == set(range(1, 6))
    assert {d for r, d in M.TAIL_CASES if r == M.SWEEP_ROWS} == set(M.TAIL_WIDTHS) == {d for r, d in M.TAIL_CASES if r == 4115}
    # row sweep: one EDGE and one WHOLE width per path, at every row count
    routes = {"ln_fwd": lambda d: "predicated", "ln_bwd": ln_bwd_route, "resid_ln_fwd": resid_ln_fast,
              "scale_residual": scale_residual_bwd_fast, "ln_bwd_tail": tail_takes}
    want = {"ln_fwd": 1, "ln_bwd": 2, "resid_ln_fwd": 2, "scale_residual": 2, "ln_bwd_tail": 1}
    cases = {"ln_fwd": M.LN_CASES, "ln_bwd": M.LN_CASES, "resid_ln_fwd": M.RESID_LN_CASES,
             "scale_residual": [(r, d) for r, k, d in M.SCALE_RESIDUAL_CASES], "ln_bwd_tail": M.TAIL_CASES}
    for path, widths in M.ROW_SWEEP_WIDTHS.items():
        assert len({routes[path](d) for d in widths}) == want[path], path
        assert any(d in M.WHOLE for d in widths) and (path == "ln_bwd_tail" or any(d in M.EDGE for d in widths)), path
        for d in widths:
            assert {r for r, dd in cases[path] if dd == d} >= set(M.ROW_SWEEP), (path, d)
    assert M.ROW_SWEEP == (1, 3, 5, 16, 17, 67, 257, 4115) and M.SWEEP_ROWS == 67
    L = _lib.lib()
    assert L.octic_dense_blocks(67) == 5 and L.octic_dense_blocks(4115) == 256 and 4115 == 256 * 16 + 19
    # grid caps: past 4096 workgroups of 16 rows and past 8192 of 8
    assert (M.CAP_ROWS + 15) // 16 > 4096 and (M.CAP_ROWS + 7) // 8 > 8192 and M.CAP_WIDTHS == (4, 256)
    assert not resid_ln_fast(4) and resid_ln_fast(256)
    # samples: one row a sample, three (no divisor of a workgroup's 16 rows) and one sample
    assert M.rps_of(67) == 1 and M.rps_of(4115) == 5 and all(r % M.rps_of(r) == 0 for r in M.ROW_SWEEP + (M.CAP_ROWS,))
    assert {k for r, k in M.SAMPLE_CASES} >= {3} and all(r % k == 0 for r, k in M.SAMPLE_CASES)
    assert any(r == k for r, k in M.SAMPLE_CASES)
    # relations
    assert set(M.RELATION_WIDTHS) == {d for d in M.WHOLE if d <= 1280} | {4, 508, 1796} and M.RELATION_ROWS == (67, 4115)
    assert sum(d in M.EDGE for d in M.RELATION_WIDTHS) == 3
    assert {(r, d) for r, d in M.RESID_LN_CASES} >= {(r, d) for d in M.RELATION_WIDTHS for r in M.RELATION_ROWS}
    assert {k for r, d, k in M.ROWMAP_CASES} == {"subset", "identity", "one"}
    for rows, kind in ((67, "subset"), (4115, "subset"), (67, "identity"), (1, "one")):
        S, m = M.make_map(rows, kind, 1)
        assert 2 * rows <= S <= 3 * rows and m.numel() == rows and int(m.max()) < S
        if kind == "subset":
            assert 0 in m.tolist() and S - 1 in m.tolist()
    # column kernels: the strip of a slab, ceil(rows / 256)
    strips = [-(-r // 256) for r, k in M.COLSUM_ROWS]
    assert strips == [1, 3, 16, 17, 29] and all(r % k == 0 for r, k in M.COLSUM_ROWS)
    assert M.COLSUM_WIDTHS == (8, 504, 512, 520, 3840) and M.GELU_WIDTHS == (8, 504, 512, 520, 5120)
    assert M.GELU_ROWS == (1, 3, 1030, 2309) and -(-2309 // 256) == 10
    assert M.FINISH_NBLOCKS == (1, 15, 16, 17, 48, 49, 63, 64, 65, 112, 113, 255, 256) and M.FINISH_WIDTHS == (4, 8, 12, 260)
