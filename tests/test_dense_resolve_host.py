"""CPU-only: every plan and order query of csrc/dense_gemm.hip answers what it answered before the host layer was rebuilt around
one resolved launch (dense_resolve).  The module calls nothing but the exported queries, over a sweep of shapes, modes, masks,
route overrides and refusals, and compares one SHA-256 per (query family, route setting) against DIGESTS below.

DIGESTS were generated from a build of the commit BEFORE dense_resolve existed (the parent of the change that added this file),
never from the code under test:

    OCTIC_LIB=<parent build>/liboctic_hip.so python tests/test_dense_resolve_host.py --digests

Run as a script with a path, the module writes the full table as JSON; a digest that moved is located by diffing the dump of the
older build against the newer one's (order records carry the return value and a short hash of their arrays):

    python tests/test_dense_resolve_host.py table.json

256 workgroup slots (no device: the library plans for 256 CUs)."""
import ctypes
import functools
import hashlib
import itertools
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from octic_vits_amd import _lib

TOK = 257
MS = tuple(dict.fromkeys([B * TOK for B in (1, 2, 3, 16, 64, 65, 128)] + [256, 300, 4096, 16448]))
NS = (256, 320, 640, 1280, 3840, 5120)
KS = (128, 640, 1280, 3840, 5120)
MODES = tuple(range(7))
TOKENS = (0, TOK)
DROPS = (0.0, 0.1, 0.5, 0.9)
# the eight dense_nt launches of a ViT-H standard block (N, K, mode): qkv, proj + residual, fc1 + factor, fc2 + residual and the
# input gradients of fc2, fc1, proj, qkv
VITH = ((3840, 1280, 0), (1280, 1280, 2), (5120, 1280, 4), (1280, 5120, 2), (5120, 1280, 5), (1280, 5120, 0), (1280, 1280, 0),
        (1280, 3840, 0))
ROUTES = {"default": None}
for _knob, _values in (("DENSE_TILE", (0, 4, 5, 16, 32)), ("DENSE_SPLIT", (0, 1, 2, 8)), ("DENSE_IMAGE", (0, 1, 2, 3, 4, 8, 12, 16)),
                       ("DENSE_CLS2", (0, 1, 2))):
    for _v in _values:
        ROUTES[f"{_knob}={_v}"] = (getattr(_lib, "ROUTE_" + _knob), _v)
FAMILIES = ("plan", "plan_dropped", "plan_adaptive", "plan_adaptive_cls", "plan_image", "tile", "colsum_rows", "workspace_bytes",
            "order_dropped", "order_adaptive", "order_adaptive_cls", "order_image", "refusals")


def shapes(route):
    """(M, N, K, mode) of a route setting: the whole cross product at default routes, the ViT-H launches otherwise."""
    if route == "default":
        return list(itertools.product(MS, NS, KS, MODES))
    return [(B * TOK, N, K, mode) for B in (3, 64) for N, K, mode in VITH]


def rps_values(M):
    return tuple(dict.fromkeys((TOK, 1, M)))


def q(name, n, *args):
    """[return code, the n ints the query wrote]"""
    out = (ctypes.c_int * n)(*([-7] * n))
    return [getattr(_lib.lib(), "octic_dense_gemm_" + name)(*args, out)] + list(out)


def masks(S):
    """Kept (True) / dropped samples: every mask of up to three samples; else all kept, all dropped, alternating, two seeded draws."""
    if S <= 3:
        return [list(m) for m in itertools.product((True, False), repeat=S)]
    return [[True] * S, [False] * S, [bool(i & 1) for i in range(S)]] + [
        (np.random.RandomState(seed).rand(S) < 0.5).tolist() for seed in (1, 2)]


def scale(keep):
    return np.ascontiguousarray([2.0 if k else 0.0 for k in keep], dtype=np.float32)


def order(name, head, cap, n_arrays, cls_cap=None, width=False):
    """[return code, hash of everything the order query wrote] with arrays of exactly `cap` / `cls_cap` entries."""
    arrs = [np.full(max(cap, 0) + 1, -7, dtype=np.int32) for _ in range(n_arrays)]
    w = ctypes.c_int(-7)
    args = list(head) + [cap] + [a.ctypes.data for a in arrs] + ([ctypes.addressof(w)] if width else [])
    cls = []
    if cls_cap is not None:
        cls = [np.full(max(cls_cap, 0) + 1, -7, dtype=np.int32) for _ in range(2)]
        args += [cls_cap] + [a.ctypes.data for a in cls]
    rc = getattr(_lib.lib(), "octic_dense_gemm_" + name)(*args)
    assert all(int(a[-1]) == -7 for a in arrs + cls), (name, head)                    # nothing past the caps
    h = hashlib.sha256()
    for a in arrs + cls:
        h.update(a.tobytes())
    return [rc, w.value, h.hexdigest()[:16]]


def order_records(family, route):
    recs = []
    refused = 0
    for M, N, K, mode in shapes(route):
        for tokens in TOKENS:
            for rps in rps_values(M):
                if M % rps or (rps == 1 and M > 3 * TOK and not (N == 1280 and K == 1280)):
                    continue                                                           # (per-row masks of a large M: one problem)
                drops = DROPS[1:] if family == "order_image" else (0.0,)
                for drop in drops:
                    if family == "order_dropped":
                        plan = q("plan_dropped", 4, M, N, K, mode, tokens, rps)
                        taken, cap, cls_cap = mode != 2, plan[4], None
                    elif family == "order_adaptive":
                        plan = q("plan_adaptive", 5, M, N, K, mode, tokens, rps)
                        taken, cap, cls_cap = plan[1] == 1, plan[2], None
                    elif family == "order_adaptive_cls":
                        plan = q("plan_adaptive_cls", 5, M, N, K, mode, tokens, rps)
                        taken, cap, cls_cap = plan[1] == 1, plan[2], plan[3] * plan[4]
                    else:
                        plan = q("plan_image", 8, M, N, K, mode, tokens, rps, 1, drop)
                        taken, cap, cls_cap = plan[1] == 1, plan[2], plan[3] * plan[4]
                    if not taken:
                        refused += 1
                        if refused % 97 != 1:
                            continue                                                   # a few of the launches not taken: the refusal
                    S = M // rps
                    for keep in (masks(S) if taken else masks(S)[:1]):
                        sc = scale(keep)
                        head = [M, N, K, mode, tokens, sc.ctypes.data, rps] + ([drop] if family == "order_image" else [])
                        n, width = {"order_dropped": (5, False), "order_adaptive": (3, True), "order_adaptive_cls": (3, True),
                                    "order_image": (3, False)}[family]
                        recs.append([M, N, K, mode, tokens, rps, drop, "".join("01"[k] for k in keep[:64])] +
                                    order(family, head, cap, n, cls_cap, width))
    return recs


def refusal_records():
    """A null `out`, M = 0, K = 64, a rows_per_sample that does not divide M, a cap one short, a cls_cap one short."""
    recs = []
    L = _lib.lib()
    for B, N, K, mode in ((64, 1280, 1280, 0), (64, 5120, 1280, 5), (3, 1280, 640, 4), (64, 3840, 1280, 0)):
        M = B * TOK
        for M_, K_, rps in ((M, K, TOK), (0, K, TOK), (M, 64, TOK), (M, K, 7), (M, K, 0)):
            recs.append([B, N, K, mode, M_, K_, rps,
                         L.octic_dense_gemm_plan(M_, N, K_, mode, TOK, None), q("plan", 4, M_, N, K_, mode, TOK),
                         L.octic_dense_gemm_plan_dropped(M_, N, K_, mode, TOK, rps, None), q("plan_dropped", 4, M_, N, K_, mode, TOK, rps),
                         L.octic_dense_gemm_plan_adaptive(M_, N, K_, mode, TOK, rps, None), q("plan_adaptive", 5, M_, N, K_, mode, TOK, rps),
                         L.octic_dense_gemm_plan_adaptive_cls(M_, N, K_, mode, TOK, rps, None),
                         q("plan_adaptive_cls", 5, M_, N, K_, mode, TOK, rps),
                         L.octic_dense_gemm_plan_image(M_, N, K_, mode, TOK, rps, 1, 0.5, None),
                         q("plan_image", 8, M_, N, K_, mode, TOK, rps, 1, 0.5), q("plan_image", 8, M_, N, K_, mode, TOK, rps, 0, 0.5),
                         L.octic_dense_gemm_tile(M_, N, K_, mode), L.octic_dense_gemm_colsum_rows(M_, N, K_),
                         L.octic_dense_gemm_workspace_bytes(M_, N, K_)])
            sc = scale([True, False] * (B // 2) + [True] * (B % 2))
            for null in (False, True):
                p = None if null else sc.ctypes.data
                recs.append([B, N, K, mode, M_, K_, rps, null,
                             order("order_dropped", [M_, N, K_, mode, TOK, p, rps], 4096, 5),
                             order("order_adaptive", [M_, N, K_, mode, TOK, p, rps], 4096, 3, width=True),
                             order("order_adaptive_cls", [M_, N, K_, mode, TOK, p, rps], 4096, 3, 8192, width=True),
                             order("order_image", [M_, N, K_, mode, TOK, p, rps, 0.5], 4096, 3, 8192)])
        # caps: exactly enough, one short
        sc = scale([True, False] * (B // 2) + [True] * (B % 2))
        grid = q("plan_dropped", 4, M, N, K, mode, TOK, TOK)[4]
        ad, fold, img = q("plan_adaptive", 5, M, N, K, mode, TOK, TOK), q("plan_adaptive_cls", 5, M, N, K, mode, TOK, TOK), \
            q("plan_image", 8, M, N, K, mode, TOK, TOK, 1, 0.5)
        for short in (0, 1):
            recs.append([B, N, K, mode, short, order("order_dropped", [M, N, K, mode, TOK, sc.ctypes.data, TOK], grid - short, 5),
                         order("order_adaptive", [M, N, K, mode, TOK, sc.ctypes.data, TOK], ad[2] - short, 3, width=True),
                         order("order_adaptive_cls", [M, N, K, mode, TOK, sc.ctypes.data, TOK], fold[2] - short, 3, fold[3] * fold[4],
                               width=True),
                         order("order_adaptive_cls", [M, N, K, mode, TOK, sc.ctypes.data, TOK], fold[2], 3, fold[3] * fold[4] - short,
                               width=True),
                         order("order_image", [M, N, K, mode, TOK, sc.ctypes.data, TOK, 0.5], img[2] - short, 3, img[3] * img[4]),
                         order("order_image", [M, N, K, mode, TOK, sc.ctypes.data, TOK, 0.5], img[2], 3, img[3] * img[4] - short)])
    return recs


def plan_records(family, route):
    L = _lib.lib()
    recs = []
    for M, N, K, mode in shapes(route):
        if family == "tile":
            recs.append([M, N, K, mode, L.octic_dense_gemm_tile(M, N, K, mode)])
        elif family in ("colsum_rows", "workspace_bytes"):
            if mode == 0:
                recs.append([M, N, K, getattr(L, "octic_dense_gemm_" + family)(M, N, K)])
        else:
            for tokens in TOKENS:
                if family == "plan":
                    recs.append([M, N, K, mode, tokens] + q("plan", 4, M, N, K, mode, tokens))
                    continue
                for rps in rps_values(M):
                    if family == "plan_dropped":
                        recs.append([M, N, K, mode, tokens, rps] + q("plan_dropped", 4, M, N, K, mode, tokens, rps))
                    elif family in ("plan_adaptive", "plan_adaptive_cls"):
                        recs.append([M, N, K, mode, tokens, rps] + q(family, 5, M, N, K, mode, tokens, rps))
                    else:
                        for drop, masked in itertools.product(DROPS, (0, 1)):
                            recs.append([M, N, K, mode, tokens, rps, drop, masked] + q("plan_image", 8, M, N, K, mode, tokens, rps, masked, drop))
    return recs


def records(family, route):
    knob = ROUTES[route]
    try:
        if knob is not None:
            _lib.route_override(*knob)
        if family == "refusals":
            return refusal_records()
        return order_records(family, route) if family.startswith("order_") else plan_records(family, route)
    finally:
        if knob is not None:
            _lib.route_override(knob[0], 0)


def digest(recs):
    return hashlib.sha256(json.dumps(recs, separators=(",", ":")).encode()).hexdigest()


@functools.lru_cache(maxsize=None)
def digests(route):
    return {family: digest(records(family, route)) for family in FAMILIES}


@pytest.mark.parametrize("route", list(ROUTES))
def test_every_query_answers_what_it_answered_before_the_resolved_launch(route):
    got = digests(route)
    assert {f: got[f] for f in FAMILIES if got[f] != DIGESTS[route][f]} == {}, route


def test_the_sweep_reaches_every_launch_family():
    """The digests would hold for a sweep that never left the classic plan: each family of dense_resolve is taken somewhere."""
    M = 64 * TOK
    assert q("plan", 4, M, 1280, 1280, 0, TOK)[1:4] == [320, 2 * 64 + 4, 1]             # per-image panels, the 320-wide tile
    assert q("plan", 4, M, 5120, 1280, 5, TOK)[3] == 0                                  # classic panels
    assert q("plan_adaptive", 5, M, 1280, 1280, 0, TOK, TOK)[1] == 1
    assert q("plan_adaptive_cls", 5, M, 1280, 1280, 0, TOK, TOK)[1] == 1
    assert q("plan_image", 8, M, 5120, 1280, 5, TOK, TOK, 1, 0.5)[1] == 1
    assert any(r[-3] > 0 for r in order_records("order_image", "DENSE_IMAGE=4"))        # ... and their order query walks launches


# generated from a build of the parent commit (see the module docstring)
DIGESTS = {
 "default": {
  "plan": "9dba261413cc95dc6a9f47fab2eb962155c451c9aa31022e16ffd87ddaef7624",
  "plan_dropped": "2b7cf0d5d46900ec7f6fbf3cb7da0ef58cb9ced9caf4bbeffdc266aa87877d7f",
  "plan_adaptive": "695a1040b13b0547c0b6aad048c059f8c6fc0c98a3be22db14e27a3524c353f1",
  "plan_adaptive_cls": "24095ba0943ea1ec07e7dff3765ef847168a679227f1366e15b34de1a21de42c",
  "plan_image": "955b2bf6188696691178b4c59423667a92e8045f1e5bcb92cfcacc54a4405404",
  "tile": "2fc6326c5078b01d126b5d4d8ddfcec6e230c55368286607fa1d64c1ebeb5d2a",
  "colsum_rows": "3e701ab8e0fd88e059465eb4f28ed37687edce118f8ef9a1d3bc711aecb9de46",
  "workspace_bytes": "d0b2b5178f1e268428ac818633180ca907f30c05f7d3722dd2b75d65dcab8307",
  "order_dropped": "f089cb6b38d92e997ae285e7cda2f9ca7a533e8b2b9750e8f311c7f81fd29512",
  "order_adaptive": "7a98bfe404c4427aeb484d04b7c23160555e5c18aae5cff9c6d230ffb2f7a08a",
  "order_adaptive_cls": "6cd60bbdda5c1f86b10d2c2458542c040069a1fda86acc70abbd73677d3fcb23",
  "order_image": "8a9ba77e0e920a085fd079d00eb31ece8d861ced0f090a18befeef4b1154e0a5",
  "refusals": "51713da040c6c0db4b25fd89b4d7b31e45826a9abaf7c2f6a5a4091ce2ba0f5a"
 },
 "DENSE_TILE=0": {
  "plan": "058377c40dba20e1a8581e4714a19774c765d5c93593217610b18e9aa80035f0",
  "plan_dropped": "2610c865fe72aa495e054eff429bd5432c8308a8ada7c2bbd99e5a54c21b7e39",
  "plan_adaptive": "2597824eddd4a8c1f9205060923dbdbb41f6ac1fe01beec89a1a916d3226cc7c",
  "plan_adaptive_cls": "96e7b1ba4bc37446bcbfdb131eb5490c72ab773a4afe2257899bbf95888f08a0",
  "plan_image": "de0c9f643a09221d074ed68d6c8fc9b5dbd2a20a9a691fe4e537b4dfa111eb3d",
  "tile": "c9aa4f0d1a8891da07c135ca1b488cb668119972c43b1334b296200f03cdc42f",
  "colsum_rows": "dffcbf8fc1edb566a753ee06b09dae09c5a3bbb168ef3dcc8d59389e2acd9b6f",
  "workspace_bytes": "d83c9fa02e544ab9caeb2a0f56684d34567f50b0733e73a4cf14870faed82526",
  "order_dropped": "e4ea0bd2f7b2f9fe9403abb5bb41922c5f065715c9a9702a785303c061631b9c",
  "order_adaptive": "d869c2e4a8954f2269150a16773a9d4650bd264fec815ed62a186fc02410d9fa",
  "order_adaptive_cls": "717a30422268710dcd8b5497df39ec37cab52258d066c75cd180dfacc148871b",
  "order_image": "d45f05c130cdb57eb98eec0d8398e0e53951a6fbd752c59b5a461e2bb716b30f",
  "refusals": "51713da040c6c0db4b25fd89b4d7b31e45826a9abaf7c2f6a5a4091ce2ba0f5a"
 },
 "DENSE_TILE=4": {
  "plan": "24a3a68dc79bc920985eadfb0ee3425f306e1fe571826b2198acfb5f44cc64cc",
  "plan_dropped": "720c75d37a8c53608416bedc5b5c1cd46b01676296fa1b7bbb2b53c953e73886",
  "plan_adaptive": "2648bd654a3a8a1b739634fff37329332085517f441a2ee9952b23c048f20483",
  "plan_adaptive_cls": "5dce59c11ca3c08ae16555e98be03941750998163a5b76c30b1f02d9ce55a4cc",
  "plan_image": "ba1c0a9be9346c43fdca0a991a79ee5f911ca6033b97e6f8d00a43da7dca69cd",
  "tile": "04c8d30d535537776e9e6c89707dd91b2466b4b4612d8741a198318397ec84a8",
  "colsum_rows": "dffcbf8fc1edb566a753ee06b09dae09c5a3bbb168ef3dcc8d59389e2acd9b6f",
  "workspace_bytes": "d83c9fa02e544ab9caeb2a0f56684d34567f50b0733e73a4cf14870faed82526",
  "order_dropped": "ddbb174a56c81aca1907f2f686a3fc1ccc51ef91d0285855b6ed73f52483ee90",
  "order_adaptive": "d403c59197660a7abbca574bcace1db16551f2fe3fc1f4117fd3b39488400796",
  "order_adaptive_cls": "eb2d914d7ed19e0f6f4cc1799620605cb191022bbd536f5f22f052292a6692bb",
  "order_image": "d45f05c130cdb57eb98eec0d8398e0e53951a6fbd752c59b5a461e2bb716b30f",
  "refusals": "eb11826f357fcee888780e57ad79e48b6f936ff90c4b6023c178eb0d40145b10"
 },
 "DENSE_TILE=5": {
  "plan": "c2dbbb92f59db60bda627acdbbc2c8032837ba67bf682d0eeeb7b7436951c873",
  "plan_dropped": "0103ac35ea694f095bbb797c33d6b54020847716b861c4ed0328cf4d3d32d707",
  "plan_adaptive": "d74f8091ac047d61e912fdeb57eb8d18632f254060ce1ccde864e7083ca3fab7",
  "plan_adaptive_cls": "f37c8229af908c2400493ee9b73103e9e667693c4d875be19c83336d9401d4b2",
  "plan_image": "c1f5c822774d3ccd3b4c6669a38b6213960d1c782f3421ff80f927b08bb6e5c6",
  "tile": "146877e707dbd65a8fe2c46e3abde39d0a0f772defc790dba35da84d5e3991d2",
  "colsum_rows": "dffcbf8fc1edb566a753ee06b09dae09c5a3bbb168ef3dcc8d59389e2acd9b6f",
  "workspace_bytes": "d83c9fa02e544ab9caeb2a0f56684d34567f50b0733e73a4cf14870faed82526",
  "order_dropped": "fc8413085326c558300dbc72af9966777209c51101a939bdb9b9b0d481ef8081",
  "order_adaptive": "a24ccc7f953f0b4f56a6a039ee1f8833d12cec79ba17d1f3be9930321ddf601a",
  "order_adaptive_cls": "baa8f345fa5f81630ce92863ccb9b66b609c464e761b9b57ad4a141537a1af0d",
  "order_image": "f19bcc58d57fa6f079275b7c6b35a65499b59b48d07893139c46ab4c56ffd4c0",
  "refusals": "e1bc77c65aee8103fabbe24ab62a0b9165daac14006843a95b42643972ce6b12"
 },
 "DENSE_TILE=16": {
  "plan": "058377c40dba20e1a8581e4714a19774c765d5c93593217610b18e9aa80035f0",
  "plan_dropped": "2610c865fe72aa495e054eff429bd5432c8308a8ada7c2bbd99e5a54c21b7e39",
  "plan_adaptive": "2597824eddd4a8c1f9205060923dbdbb41f6ac1fe01beec89a1a916d3226cc7c",
  "plan_adaptive_cls": "96e7b1ba4bc37446bcbfdb131eb5490c72ab773a4afe2257899bbf95888f08a0",
  "plan_image": "de0c9f643a09221d074ed68d6c8fc9b5dbd2a20a9a691fe4e537b4dfa111eb3d",
  "tile": "c9aa4f0d1a8891da07c135ca1b488cb668119972c43b1334b296200f03cdc42f",
  "colsum_rows": "dffcbf8fc1edb566a753ee06b09dae09c5a3bbb168ef3dcc8d59389e2acd9b6f",
  "workspace_bytes": "d83c9fa02e544ab9caeb2a0f56684d34567f50b0733e73a4cf14870faed82526",
  "order_dropped": "e4ea0bd2f7b2f9fe9403abb5bb41922c5f065715c9a9702a785303c061631b9c",
  "order_adaptive": "8dba5717d7511e1a94a3d507f5c0df08917c15e3ee11a64894ddd0b86970f457",
  "order_adaptive_cls": "b64b11744e1886120e52d9a972a1c52eb1be8a12511a9869ed52d315d5c9afc7",
  "order_image": "d45f05c130cdb57eb98eec0d8398e0e53951a6fbd752c59b5a461e2bb716b30f",
  "refusals": "a934993733566271efcdd1912042cee028c52b49fa4f65be3fd6540b1e53b1d3"
 },
 "DENSE_TILE=32": {
  "plan": "058377c40dba20e1a8581e4714a19774c765d5c93593217610b18e9aa80035f0",
  "plan_dropped": "2610c865fe72aa495e054eff429bd5432c8308a8ada7c2bbd99e5a54c21b7e39",
  "plan_adaptive": "2597824eddd4a8c1f9205060923dbdbb41f6ac1fe01beec89a1a916d3226cc7c",
  "plan_adaptive_cls": "96e7b1ba4bc37446bcbfdb131eb5490c72ab773a4afe2257899bbf95888f08a0",
  "plan_image": "de0c9f643a09221d074ed68d6c8fc9b5dbd2a20a9a691fe4e537b4dfa111eb3d",
  "tile": "c9aa4f0d1a8891da07c135ca1b488cb668119972c43b1334b296200f03cdc42f",
  "colsum_rows": "dffcbf8fc1edb566a753ee06b09dae09c5a3bbb168ef3dcc8d59389e2acd9b6f",
  "workspace_bytes": "d83c9fa02e544ab9caeb2a0f56684d34567f50b0733e73a4cf14870faed82526",
  "order_dropped": "e4ea0bd2f7b2f9fe9403abb5bb41922c5f065715c9a9702a785303c061631b9c",
  "order_adaptive": "a6b4b9c6300f52d7bcea94881507c5562dd3380a23f12aad7950a9f4f4252390",
  "order_adaptive_cls": "4e4a1442dd38f68abbc74e9c076d03b5cec5e23309937f6da50f7094469b9275",
  "order_image": "d45f05c130cdb57eb98eec0d8398e0e53951a6fbd752c59b5a461e2bb716b30f",
  "refusals": "51713da040c6c0db4b25fd89b4d7b31e45826a9abaf7c2f6a5a4091ce2ba0f5a"
 },
 "DENSE_SPLIT=0": {
  "plan": "058377c40dba20e1a8581e4714a19774c765d5c93593217610b18e9aa80035f0",
  "plan_dropped": "2610c865fe72aa495e054eff429bd5432c8308a8ada7c2bbd99e5a54c21b7e39",
  "plan_adaptive": "2597824eddd4a8c1f9205060923dbdbb41f6ac1fe01beec89a1a916d3226cc7c",
  "plan_adaptive_cls": "96e7b1ba4bc37446bcbfdb131eb5490c72ab773a4afe2257899bbf95888f08a0",
  "plan_image": "de0c9f643a09221d074ed68d6c8fc9b5dbd2a20a9a691fe4e537b4dfa111eb3d",
  "tile": "c9aa4f0d1a8891da07c135ca1b488cb668119972c43b1334b296200f03cdc42f",
  "colsum_rows": "dffcbf8fc1edb566a753ee06b09dae09c5a3bbb168ef3dcc8d59389e2acd9b6f",
  "workspace_bytes": "d83c9fa02e544ab9caeb2a0f56684d34567f50b0733e73a4cf14870faed82526",
  "order_dropped": "e4ea0bd2f7b2f9fe9403abb5bb41922c5f065715c9a9702a785303c061631b9c",
  "order_adaptive": "d869c2e4a8954f2269150a16773a9d4650bd264fec815ed62a186fc02410d9fa",
  "order_adaptive_cls": "717a30422268710dcd8b5497df39ec37cab52258d066c75cd180dfacc148871b",
  "order_image": "d45f05c130cdb57eb98eec0d8398e0e53951a6fbd752c59b5a461e2bb716b30f",
  "refusals": "51713da040c6c0db4b25fd89b4d7b31e45826a9abaf7c2f6a5a4091ce2ba0f5a"
 },
 "DENSE_SPLIT=1": {
  "plan": "ef1bdca91a5557710712b2d77f82c5930f3b33df22cde83619ccca0b0b41a621",
  "plan_dropped": "87e6c8c18438a8e4ebbdd74e26175030d83aee229d7f71ed2a3db5eb60904312",
  "plan_adaptive": "1b0b9da2562ed35f4947af89ed65b119318fb5d583c5c411017688824a4dfbb8",
  "plan_adaptive_cls": "923e7d6ce5db84894b38a914029396ca9375965178324ec8eb44a9d80a17c10f",
  "plan_image": "a583dafef9f7c4133fda0b5e399609321836fc050acc8cd9fb2cb3013f90f0f2",
  "tile": "890a6cc12b07c3e8079058b649f6a79c3585db5258a353cb7c62e41d1558ab6a",
  "colsum_rows": "dffcbf8fc1edb566a753ee06b09dae09c5a3bbb168ef3dcc8d59389e2acd9b6f",
  "workspace_bytes": "d83c9fa02e544ab9caeb2a0f56684d34567f50b0733e73a4cf14870faed82526",
  "order_dropped": "b684a277cc004394ed37f1523aad1e12e9250226e4ed3842c4518edd91399eed",
  "order_adaptive": "9f5210c17ac72725b27da6a98549a1de69ad4601629a7721e15618a02bb70761",
  "order_adaptive_cls": "b31dabf2261fc30297cffb6dbb6f1a15d1e149a96c8b6fdf719dbfa0cfae4ea7",
  "order_image": "562aed93f104e174ea17b0ba34531fb70f906316ac376cf1b174db49dd2f666b",
  "refusals": "a0be5014912ff830245be42cbb4278c399a9a4269d94214c48b4a389ac141976"
 },
 "DENSE_SPLIT=2": {
  "plan": "b1f98e66a43a9d5f4bd96658df5b152184554499c060dc52ac9ba9b903e099b5",
  "plan_dropped": "8f6543de50656fa0c4ca2bf891ecdf6e2844bfd16b5d54fbe8c38bc33db287ba",
  "plan_adaptive": "256efd3c2df7c8de9a2003484be91a96f9577dc06dc1fd79874402fdea47ce8e",
  "plan_adaptive_cls": "56a29444d14a691632dc583c6160d81abc15ee13d373dab2791f15491c97c1d8",
  "plan_image": "f8874db5f76b9e91cf72f07c35ebc4ce1648555c0edddab087641fd74fddc104",
  "tile": "c9aa4f0d1a8891da07c135ca1b488cb668119972c43b1334b296200f03cdc42f",
  "colsum_rows": "dffcbf8fc1edb566a753ee06b09dae09c5a3bbb168ef3dcc8d59389e2acd9b6f",
  "workspace_bytes": "75403737d919908bfa3cf9f7649ac80d4c33a9a9acbbc4a57824b2f694f602a8",
  "order_dropped": "95635716481910f6455d73caa36949516af73958e09013e8eb40674eed4bf299",
  "order_adaptive": "19cde19b694261212d17efa748cbbeb025880f83277122e97518b451d8ce1245",
  "order_adaptive_cls": "918c7d2d983ca5b856631817053bd0fe9b488f996ddd70e3ac61412c8eb79fae",
  "order_image": "6ed4b4e60cb5af5d792565b52b3a40523147654a4c62adc1ae3952a4c780bce6",
  "refusals": "76eee1edceb92a6723d98b240ad070ee8875624ffe8b1f15654890995d59131b"
 },
 "DENSE_SPLIT=8": {
  "plan": "9af986d39fcc47c0f54ec73ce05f47ebfd0680875d5b5892c4b9afbc2c8a413b",
  "plan_dropped": "4dc80f8f7164e1ddf6619489d66f87324c41d15868f2ac361982543d6c0fa4d1",
  "plan_adaptive": "488762691125ec3cfa73ccb29ec04f64775144fefcd9e281ea9b20165f905d24",
  "plan_adaptive_cls": "9fd855118bc4b9e8c380a14e613abd8595e8ba50f77478d229f2157f0fc2382e",
  "plan_image": "c717486a53edb55e11114d41a647324d1176ece000ada339f76a193b58e7301a",
  "tile": "e12809fa94b07eb0a89fe1febf405cf63765f6880bff51e925fd83275a0fdb6a",
  "colsum_rows": "dffcbf8fc1edb566a753ee06b09dae09c5a3bbb168ef3dcc8d59389e2acd9b6f",
  "workspace_bytes": "75403737d919908bfa3cf9f7649ac80d4c33a9a9acbbc4a57824b2f694f602a8",
  "order_dropped": "0991e4d96a9ec1d7ab306a61753241a12397a48abc237e4331b7608703b00ab5",
  "order_adaptive": "f88b82b1b53e5984ece008ea0521884bf5133456b7ff3d73391d687c6664aada",
  "order_adaptive_cls": "f7f3ff163861517dab78049c98093f2ad60cc5c9a16b79f364909ef4b9df267b",
  "order_image": "35e4215c42e8b999c480734887ccff81c9a4756990ec58c9e845d0e8da77ab95",
  "refusals": "85aa0111badc6933127a46682c4c6623eb63ccee52c552621eeecef1e0e3cffd"
 },
 "DENSE_IMAGE=0": {
  "plan": "058377c40dba20e1a8581e4714a19774c765d5c93593217610b18e9aa80035f0",
  "plan_dropped": "2610c865fe72aa495e054eff429bd5432c8308a8ada7c2bbd99e5a54c21b7e39",
  "plan_adaptive": "2597824eddd4a8c1f9205060923dbdbb41f6ac1fe01beec89a1a916d3226cc7c",
  "plan_adaptive_cls": "96e7b1ba4bc37446bcbfdb131eb5490c72ab773a4afe2257899bbf95888f08a0",
  "plan_image": "de0c9f643a09221d074ed68d6c8fc9b5dbd2a20a9a691fe4e537b4dfa111eb3d",
  "tile": "c9aa4f0d1a8891da07c135ca1b488cb668119972c43b1334b296200f03cdc42f",
  "colsum_rows": "dffcbf8fc1edb566a753ee06b09dae09c5a3bbb168ef3dcc8d59389e2acd9b6f",
  "workspace_bytes": "d83c9fa02e544ab9caeb2a0f56684d34567f50b0733e73a4cf14870faed82526",
  "order_dropped": "e4ea0bd2f7b2f9fe9403abb5bb41922c5f065715c9a9702a785303c061631b9c",
  "order_adaptive": "d869c2e4a8954f2269150a16773a9d4650bd264fec815ed62a186fc02410d9fa",
  "order_adaptive_cls": "717a30422268710dcd8b5497df39ec37cab52258d066c75cd180dfacc148871b",
  "order_image": "d45f05c130cdb57eb98eec0d8398e0e53951a6fbd752c59b5a461e2bb716b30f",
  "refusals": "51713da040c6c0db4b25fd89b4d7b31e45826a9abaf7c2f6a5a4091ce2ba0f5a"
 },
 "DENSE_IMAGE=1": {
  "plan": "0a2a24de15934ba245c16dd02b2ddc3610193fc67972e0c45766b5215a3d58f7",
  "plan_dropped": "4754575a87267f69c75d3ac30f9c2e1a15419ee8f4b31a261f3ea15ed1317859",
  "plan_adaptive": "57c5a53ffde743868e06b03770c406cd525bf118a5227bce60e64d03f4c504be",
  "plan_adaptive_cls": "355f179799c37633d57e8d7ad1bac9db3b3a738a2a8181b606c7979c704af67b",
  "plan_image": "ab6eb00202b428dad8259ea52da579607130c90b2742decb2b246e66587a7014",
  "tile": "c9aa4f0d1a8891da07c135ca1b488cb668119972c43b1334b296200f03cdc42f",
  "colsum_rows": "dffcbf8fc1edb566a753ee06b09dae09c5a3bbb168ef3dcc8d59389e2acd9b6f",
  "workspace_bytes": "d83c9fa02e544ab9caeb2a0f56684d34567f50b0733e73a4cf14870faed82526",
  "order_dropped": "2af7087c05a266dfc4b3c86ae6d92a31f28d30a20bddc0f5f5cb64154c47c2aa",
  "order_adaptive": "d869c2e4a8954f2269150a16773a9d4650bd264fec815ed62a186fc02410d9fa",
  "order_adaptive_cls": "717a30422268710dcd8b5497df39ec37cab52258d066c75cd180dfacc148871b",
  "order_image": "37c28abb19c5a51ed77ef783c1b0b6c5569c28dc857f080a048451c5eb0c7797",
  "refusals": "847f22f49d212cf48387785d9ac36c5ea116886f8903415a9b476af275f08b96"
 },
 "DENSE_IMAGE=2": {
  "plan": "78495a2eb037789b75a684fd8f8c3d87b0daa0231f98938c2141d5d1aa7a23b2",
  "plan_dropped": "b28a0ebfb7cfbe9532999cb8ffbaec5a10de3a1cf74b6c74f582126913304be6",
  "plan_adaptive": "fef3e42786876e328d67fc70540d3c0e56a48502eee8fac56b4589284988ca2e",
  "plan_adaptive_cls": "31bc8201ea7158595ae662dd0667eddddd0797afd6a0add6b3f19b7bdec49cd1",
  "plan_image": "a36ee7eeccc64dc2b666cee08f27525662ef9ad877c1d3a45234b2461e7a4c65",
  "tile": "c9aa4f0d1a8891da07c135ca1b488cb668119972c43b1334b296200f03cdc42f",
  "colsum_rows": "dffcbf8fc1edb566a753ee06b09dae09c5a3bbb168ef3dcc8d59389e2acd9b6f",
  "workspace_bytes": "d83c9fa02e544ab9caeb2a0f56684d34567f50b0733e73a4cf14870faed82526",
  "order_dropped": "40ef423f1f64cbf840ac6ae990456b8e4719a5fb8d79bfcef428dd9c6ffdc645",
  "order_adaptive": "d403c59197660a7abbca574bcace1db16551f2fe3fc1f4117fd3b39488400796",
  "order_adaptive_cls": "eb2d914d7ed19e0f6f4cc1799620605cb191022bbd536f5f22f052292a6692bb",
  "order_image": "37c28abb19c5a51ed77ef783c1b0b6c5569c28dc857f080a048451c5eb0c7797",
  "refusals": "67b2f6f077fbef292856e3a2a7c4d3a432df827636ea41624e6af435c089b560"
 },
 "DENSE_IMAGE=3": {
  "plan": "058377c40dba20e1a8581e4714a19774c765d5c93593217610b18e9aa80035f0",
  "plan_dropped": "2610c865fe72aa495e054eff429bd5432c8308a8ada7c2bbd99e5a54c21b7e39",
  "plan_adaptive": "2597824eddd4a8c1f9205060923dbdbb41f6ac1fe01beec89a1a916d3226cc7c",
  "plan_adaptive_cls": "96e7b1ba4bc37446bcbfdb131eb5490c72ab773a4afe2257899bbf95888f08a0",
  "plan_image": "de0c9f643a09221d074ed68d6c8fc9b5dbd2a20a9a691fe4e537b4dfa111eb3d",
  "tile": "c9aa4f0d1a8891da07c135ca1b488cb668119972c43b1334b296200f03cdc42f",
  "colsum_rows": "dffcbf8fc1edb566a753ee06b09dae09c5a3bbb168ef3dcc8d59389e2acd9b6f",
  "workspace_bytes": "d83c9fa02e544ab9caeb2a0f56684d34567f50b0733e73a4cf14870faed82526",
  "order_dropped": "e4ea0bd2f7b2f9fe9403abb5bb41922c5f065715c9a9702a785303c061631b9c",
  "order_adaptive": "d869c2e4a8954f2269150a16773a9d4650bd264fec815ed62a186fc02410d9fa",
  "order_adaptive_cls": "717a30422268710dcd8b5497df39ec37cab52258d066c75cd180dfacc148871b",
  "order_image": "d45f05c130cdb57eb98eec0d8398e0e53951a6fbd752c59b5a461e2bb716b30f",
  "refusals": "51713da040c6c0db4b25fd89b4d7b31e45826a9abaf7c2f6a5a4091ce2ba0f5a"
 },
 "DENSE_IMAGE=4": {
  "plan": "058377c40dba20e1a8581e4714a19774c765d5c93593217610b18e9aa80035f0",
  "plan_dropped": "2610c865fe72aa495e054eff429bd5432c8308a8ada7c2bbd99e5a54c21b7e39",
  "plan_adaptive": "2597824eddd4a8c1f9205060923dbdbb41f6ac1fe01beec89a1a916d3226cc7c",
  "plan_adaptive_cls": "96e7b1ba4bc37446bcbfdb131eb5490c72ab773a4afe2257899bbf95888f08a0",
  "plan_image": "e997ab0d4b32a19cdf1fa65386b15edca6ae26a284a1d1eeae13406d795dd7e3",
  "tile": "c9aa4f0d1a8891da07c135ca1b488cb668119972c43b1334b296200f03cdc42f",
  "colsum_rows": "dffcbf8fc1edb566a753ee06b09dae09c5a3bbb168ef3dcc8d59389e2acd9b6f",
  "workspace_bytes": "d83c9fa02e544ab9caeb2a0f56684d34567f50b0733e73a4cf14870faed82526",
  "order_dropped": "e4ea0bd2f7b2f9fe9403abb5bb41922c5f065715c9a9702a785303c061631b9c",
  "order_adaptive": "d869c2e4a8954f2269150a16773a9d4650bd264fec815ed62a186fc02410d9fa",
  "order_adaptive_cls": "717a30422268710dcd8b5497df39ec37cab52258d066c75cd180dfacc148871b",
  "order_image": "082e96556316cee8300c45194e0c2bd2e7d47c3b712c94a17f92aa82bb0201ac",
  "refusals": "9c2edaf353fa09b04989c2a030d447862b58e63a8f6364a2468613180cff54be"
 },
 "DENSE_IMAGE=8": {
  "plan": "058377c40dba20e1a8581e4714a19774c765d5c93593217610b18e9aa80035f0",
  "plan_dropped": "2610c865fe72aa495e054eff429bd5432c8308a8ada7c2bbd99e5a54c21b7e39",
  "plan_adaptive": "2597824eddd4a8c1f9205060923dbdbb41f6ac1fe01beec89a1a916d3226cc7c",
  "plan_adaptive_cls": "96e7b1ba4bc37446bcbfdb131eb5490c72ab773a4afe2257899bbf95888f08a0",
  "plan_image": "1aae0f33a9b966a718f7d01f1eb291d29e64753df031be744975e339be7da375",
  "tile": "c9aa4f0d1a8891da07c135ca1b488cb668119972c43b1334b296200f03cdc42f",
  "colsum_rows": "dffcbf8fc1edb566a753ee06b09dae09c5a3bbb168ef3dcc8d59389e2acd9b6f",
  "workspace_bytes": "d83c9fa02e544ab9caeb2a0f56684d34567f50b0733e73a4cf14870faed82526",
  "order_dropped": "e4ea0bd2f7b2f9fe9403abb5bb41922c5f065715c9a9702a785303c061631b9c",
  "order_adaptive": "d869c2e4a8954f2269150a16773a9d4650bd264fec815ed62a186fc02410d9fa",
  "order_adaptive_cls": "717a30422268710dcd8b5497df39ec37cab52258d066c75cd180dfacc148871b",
  "order_image": "85fadaabcf5ee6a330b05e39fd8d116129f976b9321f888534b4fa8f41424e41",
  "refusals": "f02dbd03760f5339ea2c8da8e4961a28a7411a9beb475d04dae45b99959ccfc1"
 },
 "DENSE_IMAGE=12": {
  "plan": "058377c40dba20e1a8581e4714a19774c765d5c93593217610b18e9aa80035f0",
  "plan_dropped": "2610c865fe72aa495e054eff429bd5432c8308a8ada7c2bbd99e5a54c21b7e39",
  "plan_adaptive": "2597824eddd4a8c1f9205060923dbdbb41f6ac1fe01beec89a1a916d3226cc7c",
  "plan_adaptive_cls": "96e7b1ba4bc37446bcbfdb131eb5490c72ab773a4afe2257899bbf95888f08a0",
  "plan_image": "5f3c09b48e3b7c4933bf4267efb8d031d905a8adbaa0e29ac0a43ab1739cdb66",
  "tile": "c9aa4f0d1a8891da07c135ca1b488cb668119972c43b1334b296200f03cdc42f",
  "colsum_rows": "dffcbf8fc1edb566a753ee06b09dae09c5a3bbb168ef3dcc8d59389e2acd9b6f",
  "workspace_bytes": "d83c9fa02e544ab9caeb2a0f56684d34567f50b0733e73a4cf14870faed82526",
  "order_dropped": "e4ea0bd2f7b2f9fe9403abb5bb41922c5f065715c9a9702a785303c061631b9c",
  "order_adaptive": "d869c2e4a8954f2269150a16773a9d4650bd264fec815ed62a186fc02410d9fa",
  "order_adaptive_cls": "717a30422268710dcd8b5497df39ec37cab52258d066c75cd180dfacc148871b",
  "order_image": "71f11634ea849bedeebc7f28cd82431898a5d83edbd67f64ab22b04e322ee4c2",
  "refusals": "827f543333f2cb70d1d3beeddd66768c8dd2b01d0b455c137fe0319e7fa240d3"
 },
 "DENSE_IMAGE=16": {
  "plan": "058377c40dba20e1a8581e4714a19774c765d5c93593217610b18e9aa80035f0",
  "plan_dropped": "2610c865fe72aa495e054eff429bd5432c8308a8ada7c2bbd99e5a54c21b7e39",
  "plan_adaptive": "2597824eddd4a8c1f9205060923dbdbb41f6ac1fe01beec89a1a916d3226cc7c",
  "plan_adaptive_cls": "96e7b1ba4bc37446bcbfdb131eb5490c72ab773a4afe2257899bbf95888f08a0",
  "plan_image": "d421ddb5332586ed6f34af05ffdea4c63ced74a2c1221ed3026f618b7bd7a1c2",
  "tile": "c9aa4f0d1a8891da07c135ca1b488cb668119972c43b1334b296200f03cdc42f",
  "colsum_rows": "dffcbf8fc1edb566a753ee06b09dae09c5a3bbb168ef3dcc8d59389e2acd9b6f",
  "workspace_bytes": "d83c9fa02e544ab9caeb2a0f56684d34567f50b0733e73a4cf14870faed82526",
  "order_dropped": "e4ea0bd2f7b2f9fe9403abb5bb41922c5f065715c9a9702a785303c061631b9c",
  "order_adaptive": "d869c2e4a8954f2269150a16773a9d4650bd264fec815ed62a186fc02410d9fa",
  "order_adaptive_cls": "717a30422268710dcd8b5497df39ec37cab52258d066c75cd180dfacc148871b",
  "order_image": "37c28abb19c5a51ed77ef783c1b0b6c5569c28dc857f080a048451c5eb0c7797",
  "refusals": "38345825c42cdbd44b979df3c8cbe7597305a4ed4ab77d2a05ed438ed673d5e4"
 },
 "DENSE_CLS2=0": {
  "plan": "058377c40dba20e1a8581e4714a19774c765d5c93593217610b18e9aa80035f0",
  "plan_dropped": "2610c865fe72aa495e054eff429bd5432c8308a8ada7c2bbd99e5a54c21b7e39",
  "plan_adaptive": "2597824eddd4a8c1f9205060923dbdbb41f6ac1fe01beec89a1a916d3226cc7c",
  "plan_adaptive_cls": "96e7b1ba4bc37446bcbfdb131eb5490c72ab773a4afe2257899bbf95888f08a0",
  "plan_image": "de0c9f643a09221d074ed68d6c8fc9b5dbd2a20a9a691fe4e537b4dfa111eb3d",
  "tile": "c9aa4f0d1a8891da07c135ca1b488cb668119972c43b1334b296200f03cdc42f",
  "colsum_rows": "dffcbf8fc1edb566a753ee06b09dae09c5a3bbb168ef3dcc8d59389e2acd9b6f",
  "workspace_bytes": "d83c9fa02e544ab9caeb2a0f56684d34567f50b0733e73a4cf14870faed82526",
  "order_dropped": "e4ea0bd2f7b2f9fe9403abb5bb41922c5f065715c9a9702a785303c061631b9c",
  "order_adaptive": "d869c2e4a8954f2269150a16773a9d4650bd264fec815ed62a186fc02410d9fa",
  "order_adaptive_cls": "717a30422268710dcd8b5497df39ec37cab52258d066c75cd180dfacc148871b",
  "order_image": "d45f05c130cdb57eb98eec0d8398e0e53951a6fbd752c59b5a461e2bb716b30f",
  "refusals": "51713da040c6c0db4b25fd89b4d7b31e45826a9abaf7c2f6a5a4091ce2ba0f5a"
 },
 "DENSE_CLS2=1": {
  "plan": "0d7a082fcd83c2b26f66bd574bf94a1a0412f666843b2b065833298c2e09a3a8",
  "plan_dropped": "9612e620eacda1f3f432977d26dedf81a64cfb585839d2937da02b3529072142",
  "plan_adaptive": "ab0d6517d7831221c2a64930b6c9e9ba66826dd33d2a0a684eb6e9d87bdba7ae",
  "plan_adaptive_cls": "12cbc52555bcd07aaebce47582b691568f338fa1f87e7d7b511238b7eb790f4b",
  "plan_image": "0b8b4ab18788e0ac11ebc72933f277cd8b8d42fccc75984e29f0e7524e2b352d",
  "tile": "c9aa4f0d1a8891da07c135ca1b488cb668119972c43b1334b296200f03cdc42f",
  "colsum_rows": "dffcbf8fc1edb566a753ee06b09dae09c5a3bbb168ef3dcc8d59389e2acd9b6f",
  "workspace_bytes": "d83c9fa02e544ab9caeb2a0f56684d34567f50b0733e73a4cf14870faed82526",
  "order_dropped": "fa814358988265305dd090db962fa6574fa7c18bf2fe54afce26921e7e820376",
  "order_adaptive": "bc4e747cc5125b530a6c3c5ca2e54f1ab43d868c056835eeb55a9d3e751dab8c",
  "order_adaptive_cls": "473d822a8c4b1bc7593bb49ba791fcb59878405e2549a79c56faee054beab2c2",
  "order_image": "11345131fa555f1edc16f5346ecd766a379eaeefe5efc7bdab1e1f223d83d33b",
  "refusals": "51713da040c6c0db4b25fd89b4d7b31e45826a9abaf7c2f6a5a4091ce2ba0f5a"
 },
 "DENSE_CLS2=2": {
  "plan": "058377c40dba20e1a8581e4714a19774c765d5c93593217610b18e9aa80035f0",
  "plan_dropped": "2610c865fe72aa495e054eff429bd5432c8308a8ada7c2bbd99e5a54c21b7e39",
  "plan_adaptive": "2597824eddd4a8c1f9205060923dbdbb41f6ac1fe01beec89a1a916d3226cc7c",
  "plan_adaptive_cls": "96e7b1ba4bc37446bcbfdb131eb5490c72ab773a4afe2257899bbf95888f08a0",
  "plan_image": "de0c9f643a09221d074ed68d6c8fc9b5dbd2a20a9a691fe4e537b4dfa111eb3d",
  "tile": "c9aa4f0d1a8891da07c135ca1b488cb668119972c43b1334b296200f03cdc42f",
  "colsum_rows": "dffcbf8fc1edb566a753ee06b09dae09c5a3bbb168ef3dcc8d59389e2acd9b6f",
  "workspace_bytes": "d83c9fa02e544ab9caeb2a0f56684d34567f50b0733e73a4cf14870faed82526",
  "order_dropped": "e4ea0bd2f7b2f9fe9403abb5bb41922c5f065715c9a9702a785303c061631b9c",
  "order_adaptive": "d869c2e4a8954f2269150a16773a9d4650bd264fec815ed62a186fc02410d9fa",
  "order_adaptive_cls": "717a30422268710dcd8b5497df39ec37cab52258d066c75cd180dfacc148871b",
  "order_image": "d45f05c130cdb57eb98eec0d8398e0e53951a6fbd752c59b5a461e2bb716b30f",
  "refusals": "51713da040c6c0db4b25fd89b4d7b31e45826a9abaf7c2f6a5a4091ce2ba0f5a"
 }
}


if __name__ == "__main__":
    if sys.argv[1:] == ["--digests"]:
        print("DIGESTS = " + json.dumps({route: digests(route) for route in ROUTES}, indent=1))
    else:
        with open(sys.argv[1], "w") as f:
            json.dump({f"{family}@{route}": records(family, route) for route in ROUTES for family in FAMILIES}, f, indent=0)
