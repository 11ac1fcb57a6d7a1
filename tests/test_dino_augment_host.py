"""CPU-only: the host side of octic_vits_amd.dino_augment - the new C symbols, draw parity with the reference's
DataAugmentationDINO (tests/golden/dino_augment_case.py holds its order), the blur quirk, the coefficient tables against the
numpy restatement of the contract (tests/golden/dino_augment_numpy.py), that restatement against Pillow's recorded results
(tests/golden/dino_augment.npz), the packed rows, and the refusals.  Everything is bit for bit."""
import os

import numpy as np
import pytest
import torch

import dino_augment_case as C
import dino_augment_numpy as N
from octic_vits_amd import _lib, ops
from octic_vits_amd import dino_augment as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "dino_augment.npz"))
SYMBOLS = ("octic_dino_resize_coeffs", "octic_dino_resize_max_taps", "octic_dino_resize_u8", "octic_dino_color_workspace_bytes", "octic_dino_color_u8")
SMALL = dict(local_crops_number=2, global_crops_size=32, local_crops_size=16)


def test_symbols_are_declared_exported_documented_and_the_abi_version_is_unchanged():
    L = _lib.lib()
    declared = _lib.header_symbols()
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in SYMBOLS:
        assert s in declared and s in _lib._PROTOS and hasattr(L, s) and s in text, s
    assert L.octic_abi_version() == 20 == _lib.ABI_VERSION
    from octic_vits_amd.build import SOURCES
    assert "dino_augment.hip" in SOURCES
    header = open(_lib.HEADER_PATH).read()
    assert "octic_dino_row" in header and "fmaf(blur_w[j]" in header and "(int)(w_j 2^22 +- 0.5)" in header
    assert ops.DINO_ROW_WORDS * 4 == 160 and "/* 160 bytes */" in header


def test_abi_argument_validation_without_gpu():
    L = _lib.lib()
    ESHAPE, EALIGN, EDTYPE, ENULL = -1, -2, -3, -4
    assert L.octic_dino_resize_max_taps(224) == 49152 // (224 * 3) and L.octic_dino_resize_max_taps(96) == 170
    assert L.octic_dino_resize_max_taps(4) == ESHAPE and L.octic_dino_resize_max_taps(4097) == ESHAPE
    assert L.octic_dino_color_workspace_bytes(2, 16, 16) == 256 + 2 * 16 * 16 * 3
    assert L.octic_dino_color_workspace_bytes(64, 224, 224) == 64 * 25 * 4 + 64 * 224 * 224 * 3
    for bad in ((0, 16, 16), (1, 4, 16), (1, 16, 4), (1, 1 << 15, 1 << 15)):
        assert L.octic_dino_color_workspace_bytes(*bad) == ESHAPE
    b, k = np.zeros((16, 2), np.int32), np.zeros((16, 15), np.int32)      # room for the most taps asked below
    co = lambda n, S, taps, bp=b.ctypes.data, kp=k.ctypes.data: L.octic_dino_resize_coeffs(n, S, taps, bp, kp)
    assert co(53, 16, 15) == 0 and co(53, 16, 9) == ESHAPE and co(16, 16, 9) == ESHAPE and co(0, 16, 9) == ESHAPE
    assert co(20, 16, 7, bp=None) == ENULL and co(20, 16, 7, kp=None) == ENULL and co(20, 16, 7) == 0 and b[:, 1].min() >= 1
    data, rows, coef, crops, dst, ws = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20, 6 << 20
    rz = lambda **k: L.octic_dino_resize_u8(*[k.get(n, v) for n, v in (
        ("data", data), ("bytes", 4096), ("rows", rows), ("coef", coef), ("len", 1024), ("N", 2), ("S", 16), ("crops", crops),
        ("stream", None))])
    assert rz(data=None) == ENULL and rz(rows=None) == ENULL and rz(coef=None) == ENULL and rz(crops=None) == ENULL
    assert rz(N=0) == ESHAPE and rz(S=4) == ESHAPE and rz(S=4097) == ESHAPE and rz(bytes=0) == ESHAPE and rz(len=0) == ESHAPE
    assert rz(rows=rows + 4) == EALIGN and rz(coef=coef + 2) == EALIGN
    assert rz(crops=data + 100) == ESHAPE                                                    # crops inside the sources
    cl = lambda **k: L.octic_dino_color_u8(*[k.get(n, v) for n, v in (
        ("crops", crops), ("dst", dst), ("dtype", _lib.F32), ("rows", rows), ("m0", 0.5), ("m1", 0.5), ("m2", 0.5), ("s0", 0.25),
        ("s1", 0.25), ("s2", 0.25), ("N", 2), ("H", 8), ("W", 8), ("ws", ws), ("stream", None))])
    assert cl(crops=None) == ENULL and cl(dst=None) == ENULL and cl(rows=None) == ENULL and cl(ws=None) == ENULL
    assert cl(N=0) == ESHAPE and cl(H=4) == ESHAPE and cl(W=4) == ESHAPE and cl(H=1 << 15, W=1 << 15) == ESHAPE
    assert cl(dtype=_lib.BF16) == EDTYPE and cl(dtype=7) == EDTYPE
    assert cl(dst=dst + 2) == EALIGN and cl(rows=rows + 4) == EALIGN and cl(ws=ws + 1) == EALIGN
    assert cl(dst=crops) == ESHAPE and cl(dst=crops + 4) == ESHAPE and cl(ws=crops) == ESHAPE and cl(ws=dst) == ESHAPE


# ------------------------------------------------------------------------------------------------ the draw
SOURCES = [[(375, 500), (500, 375), (64, 48)], [(8, 200), (200, 8), (31, 33), (1, 1)], [(1024, 3), (5, 5), (480, 640)]]


@pytest.mark.parametrize("geometry", [{}, SMALL, dict(local_crops_number=0, global_crops_scale=(0.5, 0.9))])
def test_draws_match_the_reference_order_variate_for_variate(geometry):
    ours, ref = torch.Generator().manual_seed(43), torch.Generator().manual_seed(43)
    aug = D.DinoAugment(generator=ours, **geometry)
    fallback = 0
    for sizes in SOURCES * 2:
        hs, ws = [s[0] for s in sizes], [s[1] for s in sizes]
        got = aug.draw(hs, ws)
        assert len(got) == len(sizes) and got.n_crops == 2 + aug.local_crops_number
        for b, (H, W) in enumerate(sizes):
            want = C.draw_image(H, W, generator=ref, **geometry)
            assert len(want) == got.n_crops
            for c, w in enumerate(want):
                have = got.crop(c, b)
                w = dict(w, **{k: float(np.float32(w[k])) for k in ("brightness", "contrast", "saturation")})
                assert have == w, (b, c, have, w)
                top, left, h, ww = have["box"]
                assert 0 <= top and 0 <= left and 1 <= h and 1 <= ww and top + h <= H and left + ww <= W
                if (H, W) in ((8, 200), (200, 8), (1024, 3)):
                    # no try fits such a strip at any global scale: torchvision's central crop
                    fallback += c < 2 and have["box"] in ((0, 94, 8, 11), (94, 0, 11, 8), (510, 0, 4, 3))
        assert torch.equal(ours.get_state(), ref.get_state())
    assert fallback > 0


def test_the_default_generator_is_torchs_own():
    torch.manual_seed(6)
    a = D.DinoAugment(**SMALL).draw([40, 31], [56, 33])
    b = D.DinoAugment(generator=torch.Generator().manual_seed(6), **SMALL).draw([40, 31], [56, 33])
    assert a == b


def test_the_draw_reproduces_the_golden_pipeline_parameters():
    g = torch.Generator().manual_seed(5)
    aug = D.DinoAugment(generator=g, **SMALL)
    sizes = [GOLDEN[f"pipe_src_{b}"].shape[:2] for b in range(3)]
    got = aug.draw([s[0] for s in sizes], [s[1] for s in sizes])
    for b in range(3):
        for c, want in enumerate(C.unpack(GOLDEN, f"pipe_{b}_")):
            have = got.crop(c, b)
            want = dict(want, **{k: float(np.float32(want[k])) for k in ("brightness", "contrast", "saturation")})
            assert have == want, (b, c)
    assert np.array_equal(g.get_state().numpy(), GOLDEN["pipe_generator_state"])


def test_the_blur_quirk_is_reproduced():
    """dinov2/data/transforms.py hands RandomApply 1 - p: global 1 (p = 1.0) is never blurred, global 2 (p = 0.1) nearly always."""
    aug = D.DinoAugment(generator=torch.Generator().manual_seed(1), local_crops_number=1, global_crops_size=8, local_crops_size=8)
    p = aug.draw([64] * 2000, [64] * 2000)
    assert not p.blur[0].any()
    assert 0.85 <= p.blur[1].mean() <= 0.95 and 0.45 <= p.blur[2].mean() <= 0.55
    assert ((p.sigma >= 0.1) & (p.sigma <= 2.0))[p.blur].all() and not p.sigma[~p.blur].any()
    assert not p.solarize[0].any() and not p.solarize[2].any() and 0.15 <= p.solarize[1].mean() <= 0.25
    assert 0.75 <= p.jitter.mean() <= 0.85 and 0.15 <= p.gray.mean() <= 0.25 and 0.45 <= p.flip.mean() <= 0.55


# ------------------------------------------------------------------------------------------------ the tables
@pytest.mark.parametrize("n,S", [(53, 16), (5, 16), (7, 12), (200, 12), (1, 16), (17, 16), (15, 16), (1024, 96), (1024, 224),
                                 (500, 224), (3, 5)])
def test_coefficient_tables_match_the_numpy_restatement(n, S):
    xmin, cnt, kk = N.resize_coeffs(n, S)
    bounds, k = D.resize_coeffs(n, S)
    assert bounds.dtype == k.dtype == np.int32 and k.shape == (S, D.resize_taps(n, S)) == kk.shape
    assert np.array_equal(bounds[:, 0], xmin) and np.array_equal(bounds[:, 1], cnt) and np.array_equal(k, kk)
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds.sum(1) <= n).all()
    assert (np.abs(k.astype(np.int64).sum(1) - (1 << 22)) <= k.shape[1]).all()


def test_a_skipped_pass_is_one_tap_of_unity():
    bounds, k = D.resize_coeffs(16, 16)
    assert np.array_equal(bounds, np.stack([np.arange(16), np.ones(16)], 1)) and np.array_equal(k, np.full((16, 1), 1 << 22))
    xmin, cnt, kk = N.resize_coeffs(16, 16)                # what Pillow would compute had it not skipped: the identity, too
    assert all(kk[x, xx - xmin[x]] == 1 << 22 and np.count_nonzero(kk[x]) == 1 for x, xx in enumerate(range(16)))


def test_rows_and_pool_packing():
    g = torch.Generator().manual_seed(5)
    aug = D.DinoAugment(generator=g, **SMALL)
    hs, ws = [40, 64, 31], [56, 48, 33]
    p = aug.draw(hs, ws)
    t = p.tables()
    rg, rl, coef = t["rows_global"], t["rows_local"], t["coef"]
    assert rg.shape == (6, 40) and rl.shape == (6, 40) and rg.dtype == rl.dtype == coef.dtype == np.int32
    offsets = np.concatenate([[0], np.cumsum(np.array(hs) * np.array(ws) * 3)[:-1]])
    rows = np.concatenate([rg, rl])
    at = 0
    for i, row in enumerate(rows):
        c, b = divmod(i, 3)
        S = 32 if c < 2 else 16
        q = p.crop(c, b)
        assert row[:2].copy().view(np.int64)[0] == offsets[b] and tuple(row[2:4]) == (hs[b], ws[b])
        assert tuple(row[4:8]) == q["box"] and row[8] == q["flip"]
        for word, n in ((9, q["box"][3]), (11, q["box"][2])):
            bounds, k = D.resize_coeffs(n, S)
            assert row[word] == at and row[word + 1] == k.shape[1]
            assert np.array_equal(coef[at:at + 2 * S].reshape(S, 2), bounds)
            assert np.array_equal(coef[at + 2 * S:at + 2 * S + k.size].reshape(k.shape), k)
            at += 2 * S + k.size
        assert row[13:17].tolist() == (q["order"] if q["jitter"] else [-1] * 4)
        assert row[17:20].copy().view(np.float32).tolist() == [np.float32(q[k]) for k in ("brightness", "contrast", "saturation")]
        assert row[20] == N.hue_shift(q["hue"]) == D.hue_shift(q["hue"]) and 0 <= row[20] < 256
        assert (row[21], row[22], row[23]) == (q["gray"], q["blur"], q["solarize"])
        w = row[24:33].copy().view(np.float32)
        assert np.array_equal(w, N.blur_weights(q["sigma"]) if q["blur"] else np.zeros(9, np.float32))
        assert not row[33:].any()
    assert at == coef.size <= aug.coef_capacity(3)
    assert np.array_equal(p.color_rows([(1, 2)])[0, 13:33], rows[1 * 3 + 2, 13:33])
    assert [D.hue_shift(f) for f in (0.005, 0.1, -0.1, 0.0, -0.003, -0.5, 0.5)] == [1, 25, 231, 0, 0, 129, 127]


@pytest.mark.parametrize("geometry", [dict(max_side=96), dict(max_side=224), dict(max_side=224, local_crops_number=0),
                                      dict(max_side=32, **SMALL), dict(max_side=16, **SMALL), dict(max_side=5, **SMALL)])
def test_the_pool_capacity_bounds_every_batch_also_where_max_side_is_a_crop_size(geometry):
    """A crop length equal to the output size is the skipped pass of one tap; every shorter one needs five.  The capacity must
    come from the largest count over all lengths up to max_side, not from the count AT max_side."""
    aug = D.DinoAugment(generator=torch.Generator().manual_seed(2), **geometry)
    m = aug.max_side
    for S in (aug.global_crops_size, aug.local_crops_size):
        assert D.max_resize_taps(m, S) == max(D.resize_taps(n, S) for n in range(1, m + 1)) <= ops.dino_resize_max_taps(S)
    B = 4
    worst = 0
    for sizes in ([(m, m)] * B, [(m, m - 1), (m - 1, m), (m, 1), (max(m // 2, 1), m)]):
        p = aug.draw([s[0] for s in sizes], [s[1] for s in sizes])
        assert p.tables()["coef"].size <= aug.coef_capacity(B)
        for b, (H, W) in enumerate(sizes):                   # the costliest boxes these sources allow: one short of a crop size
            p.box[:, b] = (0, 0, max(H - 1, 1), max(W - 1, 1))
        worst = max(worst, p.tables()["coef"].size)
        assert p.tables()["coef"].size <= aug.coef_capacity(B)
    assert worst > aug.coef_capacity(B) // 4


def test_blur_weights_are_torchvisions():
    for sigma in (0.1, 0.5, 1.0, 2.0, 1.2345):
        w = D.blur_weights(sigma)
        assert w.dtype == np.float32 and np.array_equal(w, N.blur_weights(sigma)) and np.array_equal(w, w[::-1])
        assert abs(float(w.astype(np.float64).sum()) - 1) < 1e-6
    assert D.blur_weights(0.1)[4] == 1.0 and 0 < D.blur_weights(0.1)[3] < 1e-20


# ------------------------------------------------------------------------------------------------ the restatement and the golden
def test_numpy_resize_equals_the_golden_pil_pixels():
    seen = {16: 0, 12: 0}
    for case in GOLDEN["resize_cases"]:
        i, top, left, h, w, S, flip = (int(v) for v in case)
        p = dict(C.identity((top, left, h, w), S), flip=bool(flip))
        want, alt = N.apply_u8(GOLDEN[f"resize_src_{i}"], p)
        assert np.array_equal(want, GOLDEN[f"resize_out_{S}"][seen[S]]) and np.array_equal(want, alt), case
        seen[S] += 1
    assert seen[16] == len(GOLDEN["resize_out_16"]) and seen[12] == len(GOLDEN["resize_out_12"]) and min(seen.values()) > 40


def test_numpy_hue_and_jitter_chain_equal_the_golden_pil_pixels():
    for f, want in zip(GOLDEN["hue_factors"], GOLDEN["hue_out"]):
        p = dict(C.identity((0, 0, 64, 64), 64), jitter=True, order=[3, -1, -1, -1], hue=float(f))
        assert np.array_equal(N.color_chain(GOLDEN["hue_src"], p)[0], want), f
    for key in ("16x16", "7x30"):
        ps = C.unpack(GOLDEN, f"jit_{key}_")
        orders = {tuple(p["order"]) for p in ps if p["jitter"]}
        assert len(orders) == 24 and len(ps) == len(GOLDEN[f"jit_src_{key}"]) == 31
        for px, p, want in zip(GOLDEN[f"jit_src_{key}"], ps, GOLDEN[f"jit_out_{key}"]):
            got, alt = N.color_chain(px, p)
            assert np.array_equal(got, want) and np.array_equal(got, alt), (key, p)


def test_numpy_pipeline_equals_the_golden_oracle_up_to_the_blur_rule():
    blurred = 0
    for b in range(3):
        src, ps = GOLDEN[f"pipe_src_{b}"], C.unpack(GOLDEN, f"pipe_{b}_")
        outs = list(GOLDEN[f"pipe_out_{b}_g"]) + list(GOLDEN[f"pipe_out_{b}_l"])
        for p, out in zip(ps, outs):
            want, alt = N.apply_u8(src, p)
            assert ((out == want) | (out == alt)).all() and (want != alt).mean() <= 0.01
            assert p["blur"] or np.array_equal(out, want)
            blurred += p["blur"]
    assert 0 < blurred < 12


def test_numpy_restatement_equals_live_pil():
    pytest.importorskip("PIL")
    rs = np.random.RandomState(3)
    g = torch.Generator().manual_seed(9)
    for H, W in [(37, 53), (120, 90), (9, 200), (5, 5)]:
        src = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
        for p in C.draw_image(H, W, generator=g, local_crops_number=3, global_crops_size=24, local_crops_size=11):
            out = C.apply_u8(src, p)
            want, alt = N.apply_u8(src, p)
            assert ((out == want) | (out == alt)).all() and (p["blur"] or np.array_equal(want, alt)), ((H, W), p)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_name_the_option():
    with pytest.raises(ValueError, match="global_crops_size"):
        D.DinoAugment(global_crops_size=4)
    with pytest.raises(ValueError, match="local_crops_size"):
        D.DinoAugment(local_crops_size=4)
    with pytest.raises(ValueError, match="max_side"):
        D.DinoAugment(max_side=1 << 16)                    # more taps than the resize kernel holds
    with pytest.raises(ValueError, match="mean"):
        D.DinoAugment(mean=(0.5, 0.5))
    aug = D.DinoAugment(max_side=256, **SMALL)
    with pytest.raises(ValueError, match="max_side"):
        aug.draw([257, 10], [10, 10])
    with pytest.raises(ValueError, match="max_side"):
        aug.draw([10], [300])
    with pytest.raises(ValueError, match="below 1"):
        aug.draw([0], [10])
    with pytest.raises(TypeError, match="uint8"):
        D.pack_images([np.zeros((4, 4, 3), np.float32)], "cuda")
    with pytest.raises(ValueError, match="below 1"):
        D.pack_images([np.zeros((0, 4, 3), np.uint8)], "cuda")
    with pytest.raises(ValueError, match=r"\[H, W, 3\]"):
        D.pack_images([np.zeros((4, 4), np.uint8)], "cuda")
    with pytest.raises(TypeError, match="device"):
        D.pack_images([np.zeros((4, 4, 3), np.uint8)], "cpu")
    cpu = D.PackedImages(torch.zeros(48, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64), torch.full((1,), 4, dtype=torch.int32),
                         torch.full((1,), 4, dtype=torch.int32))
    with pytest.raises(TypeError, match="GPU"):
        aug.apply(cpu)
    with pytest.raises(TypeError, match="GPU"):
        aug.collate(cpu, (0.1, 0.5), 0.5, 4, None)
    with pytest.raises(TypeError, match="PackedImages"):
        aug.apply(torch.zeros(48, dtype=torch.uint8))
    with pytest.raises(TypeError, match="GPU"):
        aug.apply_crops(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), np.zeros((1, 40), np.int32))
    with pytest.raises(TypeError, match="uint8"):
        aug.apply_crops(torch.zeros(1, 8, 8, 3), np.zeros((1, 40), np.int32))
    with pytest.raises(TypeError, match="GPU"):
        aug.launch(torch.zeros(48, dtype=torch.uint8), torch.zeros(2, 40, dtype=torch.int32), torch.zeros(2, 40, dtype=torch.int32),
                   torch.zeros(8, dtype=torch.int32))
    p = aug.draw([16], [16])
    p.box[0, 0] = (0, 0, 17, 16)
    with pytest.raises(ValueError, match="leaves its"):
        p.tables()
    p = aug.draw([16], [16])
    old, D._POOL_MAX = D._POOL_MAX, 100                    # the rows hold 32-bit pool offsets
    try:
        with pytest.raises(ValueError, match="coefficient pool"):
            p.tables()
    finally:
        D._POOL_MAX = old
    with pytest.raises(ValueError, match="crop-major"):
        D.DinoAugParams([16], [16], 2, 32, 16, flip=np.zeros((1, 4), bool))
