"""CPU checks of tests/golden/elementwise_cases.py: the tables reach what tests/test_elementwise_matrix_gpu.py says they reach,
and the helpers the GPU module leans on agree with the oracle and with torch."""
import numpy as np
import torch
import torch.nn.functional as F

import elementwise_cases as E


def test_heads_tables_reach_every_instantiation_a_shape_can_select():
    reach = E.heads_reachable()
    assert sorted(reach) == sorted(E.heads_all_instances())                      # all 84: none is dead code
    cases, big = E.heads_cases(), E.heads_big_lds_cases()
    got = E.heads_reached(cases)
    only_big = sorted(k for k in reach if k not in got)
    assert only_big == [("bf16", 1, 1, 16), ("f32", 1, 1, 16)]                   # (the module docstring of the GPU suite names them)
    assert not [k for k in reach if k not in E.heads_reached(cases + big)]
    for case in big:
        r = E.heads_route(case[0], case[4], case[3], case[5], 1)
        assert r[2] == 1 and 64 * 1024 < r[3] <= E.HEADS_MAX_LDS
    assert all(E.heads_route(c[0], c[4], c[3], c[5], 1)[0] != "refused" for c in cases + big)
    assert all(c[1] <= 2 for c in cases + big)
    assert {c[2] for c in cases} == {1, 3, 4, 5, 7, 257}
    assert {c[4] // c[3] for c in cases} >= {5, 10, 12, 8, 16, 9, 15, 17}
    for dtype, B, T, H, c, n_s, direction, why in E.HEADS_REFUSED:
        assert E.heads_route(dtype, c, H, n_s, direction) == ("refused", why)


def test_named_heads_shapes_land_where_they_are_meant_to():
    r = lambda dt, c, H, n_s, d: E.heads_route(dt, c, H, n_s, d)[:3]
    assert r("bf16", 72, 8, 3, 0) == (1, 5, 4) and r("bf16", 120, 8, 1, 0) == (1, 8, 4) and r("bf16", 136, 8, 3, 0) == (1, 16, 4)
    assert r("f32", 192, 12, 3, 0) == (4, 1, 2) and r("f32", 384, 12, 3, 0) == (4, 1, 1)
    assert E.heads_route("f32", 704, 8, 3, 0) == (4, 4, 1, 67584)
    assert [r(dt, 160, 16, 3, 0)[0] for dt in E.DTYPES] == [2, 2] and r("bf16", 64, 8, 3, 0)[0] == 8 and r("f32", 40, 8, 3, 0)[0] == 1


def test_heads_data_is_a_pair_under_the_oracle():
    for n_s in (1, 3):
        x, heads = E.heads_case_data("bf16", 2, 5, 8, 40, n_s)
        assert x.shape == (10, 8 * n_s * 40) and len(heads) == n_s and heads[0].shape == (2, 8, 5, 40)
        if n_s == 3:
            back = torch.cat([E.heads_unpack_ref(h) for h in heads], 1)          # [A1 q|..|E q | A1 k|..]: regroup by irrep
            c = 40
            cols = torch.cat([torch.arange(s * 8 * c + i * c, s * 8 * c + (i + 1) * c) for i in range(4) for s in range(3)]
                             + [torch.arange(s * 8 * c + 4 * c + r * 2 * c, s * 8 * c + 4 * c + (r + 1) * 2 * c) for r in range(2) for s in range(3)])
            assert torch.equal(back[:, cols], x)


def test_large_shapes_are_the_smallest_with_a_second_item():
    for dtype, c, rps, B in E.GELU_LARGE:
        per = 4 if dtype == "bf16" else 8
        assert E.second_item(B * rps * c // per) and not E.second_item((B - 1) * rps * c // per)
    c, M = E.CAST_LARGE
    assert E.second_item(M * c) and M % 257 == 0
    assert all((E.CAST_M * c) % 256 for c in E.SMALL_C)


def test_the_eight_components_of_a_channel_are_the_columns_j_plus_kc():
    c, j = 8, 3
    x = torch.zeros(1, 8 * c)
    x[0, [j + k * c for k in range(8)]] = torch.arange(1.0, 9.0)
    y, gin = E.gelu_oracle(x, torch.ones(1, 8 * c), c)
    group = np.zeros(8 * c, bool)
    group[[j + k * c for k in range(8)]] = True
    assert (y.numpy()[0][~group] == 0).all() and (y.numpy()[0][group] != 0).all()
    s = E.group_scale(y.numpy(), c)
    assert (s[0][group] == np.abs(y.numpy()).max()).all() and (s[0][~group] == 0).all()


def test_spectrum_inputs_hold_the_zeros_and_autograd_returns_zero_there():
    c, M = 8, 19
    ref = E.spectrum_case(M, c)
    x = ref["x"].numpy()
    assert (x[:, c:4 * c] == 0).any() and np.signbit(x[:, c:4 * c][x[:, c:4 * c] == 0]).any()
    pair0 = (x[:, 4 * c:6 * c] == 0) & (x[:, 6 * c:] == 0)
    assert pair0.any() and ((x[:, 4 * c:6 * c] == 0) & ~pair0).any()
    assert not np.isnan(ref["dx"]).any()
    assert (ref["dx"][:, c:4 * c][x[:, c:4 * c] == 0] == 0).all()
    assert (ref["dx"][:, 4 * c:6 * c][pair0] == 0).all() and (ref["dx"][:, 6 * c:][pair0] == 0).all()


def test_im2col_reference_is_unfold():
    for Himg, Wimg, p in E.IM2COL:
        img = torch.randn(3, 3, Himg, Wimg, generator=E.gen("host.img"))
        K = 3 * p * p
        want = F.unfold(img, p, stride=p).transpose(1, 2).reshape(-1, K)
        got = E.im2col_ref(img, p, K + 8)
        assert torch.equal(got[:, :K], want) and not got[:, K:].any()


def test_prep_table_and_references():
    assert E.PREP_ITEM_DTYPE.itemsize == 112                                      # octic_prep_item: 12 pointers and four ints
    assert E.prep_tiles(40, 120) == 4 * 2 * 1 + 4 * 2 and E.prep_tiles(8, 8) == 5 and E.PREP_MANY * 5 > 256 * 5
    w5, cs5 = E.prep_inputs("host", 8, 24)
    wb, wt = E.prep_ref(w5, cs5, torch.bfloat16)
    assert wb.numel() == wt.numel() == 8 * 8 * 24
    assert torch.equal(wt[:8 * 24].reshape(8, 24), (w5[0] * cs5[0][:, None]).t().to(torch.bfloat16))
    assert torch.equal(E.prep_ref(w5, None, torch.float32)[1][4 * 8 * 24:].reshape(16, 48), w5[4].t())
