"""tests/pack_numpy.py (the numpy restatement of the weight packs that test_gpu_pack.py holds the pack kernels to)
against a plain dense W @ x through the slot maps: the packs are decoded the way the matrix instructions read them --
written out as loops, lane by lane -- and applied to a slot vector."""
import numpy as np
import torch

import pack_numpy as pk
from monosdf_amd.plan import MlpPlan


def _hand_plan():
    """Two units with maps that are no identity: unit 0 has 3 out tiles (odd: one tile of even padding) and 3 k tiles
    (two k blocks of 32, the second half empty), both maps permuted and with holes; unit 1 multiplies unit 0's out
    slots and gives two of its rows as dot-product rows."""
    g = np.random.default_rng(5)
    mp = MlpPlan()
    mp.w_shapes = [(40, 37), (5, 40)]
    rowmap0 = np.full(48, -1, np.int32)
    rowmap0[g.permutation(48)[:40]] = g.permutation(40)
    colmap0 = np.full(48, -1, np.int32)
    colmap0[g.permutation(48)[:37]] = g.permutation(37)
    rowmap1 = np.full(16, -1, np.int32)
    rowmap1[[0, 3, 4, 9, 15]] = [2, 0, 4, 1, 3]
    mp.add_unit(0, rowmap0, colmap0, 0.5)
    mp.add_unit(1, rowmap1, rowmap0.copy(), 1.0)
    P = mp.plan
    P.sdf_slot, P.out_rows, P.wsdf_off = 3, 2, mp.bpack_f
    mp.bpack_f += 2 * 16 * P.layer[1].kt
    mp.finalise()
    return mp


def _dense(mp, u, flat_w, x_slots, transposed):
    """What unit u computes from a slot vector, from the original matrix and the maps alone (float64, exact here)."""
    L, R = mp.plan.layer[u], mp.rules[u]
    rowmap, colmap = mp.rowmaps[u][1], mp.colmaps[u][1]
    W = flat_w[R.w_off:R.w_off + R.rows * R.cols].reshape(R.rows, R.cols).astype(np.float64) * float(R.scale)
    if transposed:
        W, rowmap, colmap = W.T, colmap, rowmap
    x = np.zeros(W.shape[1])
    x[colmap[colmap >= 0]] = x_slots[:len(colmap)][colmap >= 0]
    y = W @ x
    return np.where(rowmap >= 0, y[np.maximum(rowmap, 0)], 0.0)


def _apply_f32(img, RT, KT, x_slots):
    """y[16 rt + (l & 15)] += A[rt][kt][l][r] * x[16 kt + 4 (l >> 4) + r]: v_mfma_f32_16x16x4_f32, A = the pack's float4"""
    y = np.zeros(16 * RT)
    for rt in range(RT):
        for kt in range(KT):
            for l in range(64):
                for r in range(4):
                    y[16 * rt + (l & 15)] += float(img[((rt * KT + kt) * 64 + l) * 4 + r]) * x_slots[16 * kt + 4 * (l >> 4) + r]
    return y


def _bf16_value(bits):
    return torch.from_numpy(np.asarray(bits, np.int16)).view(torch.bfloat16).double().numpy()


def _apply_b16(img, planes, RT, KB, x_slots):
    """the same on k blocks of 32 slots: lane l supplies the 8 k slots 16 (2 kb + j / 4) + 4 (l >> 4) + j % 4, and the
    value of a weight is the sum of its planes"""
    y = np.zeros(16 * RT)
    v = _bf16_value(img).reshape(RT, KB, planes, 64, 8).sum(2)
    for rt in range(RT):
        for kb in range(KB):
            for l in range(64):
                for j in range(8):
                    y[16 * rt + (l & 15)] += v[rt, kb, l, j] * x_slots[16 * (2 * kb + j // 4) + 4 * (l >> 4) + j % 4]
    return y


def _weights(mp, g):
    # small integers (and scale 0.5): every product and sum below is exact, in bf16 too
    return (g.integers(-15, 16, mp.n_w).astype(np.float32), g.integers(-15, 16, mp.n_b).astype(np.float32))


def test_pack_restatement_is_dense_product_through_the_maps():
    mp = _hand_plan()
    g = np.random.default_rng(6)
    flat_w, flat_b = _weights(mp, g)
    x = g.integers(-7, 8, 16 * 17 + 32).astype(np.float64)
    w32, cov32 = pk.wpack_f32(mp, flat_w)
    assert cov32.all()                                       # the fp32 plan has no gaps
    for u in range(2):
        L = mp.plan.layer[u]
        want_f = _dense(mp, u, flat_w, x, False)
        want_b = _dense(mp, u, flat_w, x, True)
        assert np.abs(want_f).max() > 0 and np.abs(want_b).max() > 0
        ev = lambda n: (n + 1) & ~1
        got = _apply_f32(w32[4 * L.wf_off:], ev(L.ot), L.ktp, x)
        assert (got[:16 * L.ot] == want_f).all() and (got[16 * L.ot:] == 0).all()
        got = _apply_f32(w32[4 * L.wb_off:], ev(L.kt), L.otp, x)
        assert (got[:16 * L.kt] == want_b).all() and (got[16 * L.kt:] == 0).all()
        for planes in (2, 3):
            w16, cov16 = pk.wpack_b16(mp, planes, flat_w)
            L16 = mp.build_b16(planes).layer[u]
            n_f, n_b = ev(L.ot) * L16.ktp * planes * 512, ev(L.kt) * L16.otp * planes * 512
            assert cov16[8 * L16.wf_off:8 * L16.wf_off + n_f].all() and cov16[8 * L16.wb_off:8 * L16.wb_off + n_b].all()
            got = _apply_b16(w16[8 * L16.wf_off:8 * L16.wf_off + n_f], planes, ev(L.ot), L16.ktp, x)
            assert (got[:16 * L.ot] == want_f).all() and (got[16 * L.ot:] == 0).all()
            got = _apply_b16(w16[8 * L16.wb_off:8 * L16.wb_off + n_b], planes, ev(L.kt), L16.otp, x)
            assert (got[:16 * L.kt] == want_b).all() and (got[16 * L.kt:] == 0).all()


def test_bias_and_dot_rows():
    mp = _hand_plan()
    flat_w, flat_b = _weights(mp, np.random.default_rng(7))
    b, cov = pk.bpack(mp, flat_w, flat_b)
    assert cov.all() and len(b) == 48 + 16 + 2 * 48
    P = mp.plan
    for u in range(2):
        L, rowmap = P.layer[u], mp.rowmaps[u][1]
        for s in range(16 * L.ot):
            assert b[L.bias_off + s] == (flat_b[mp.rules[u].b_off + rowmap[s]] if rowmap[s] >= 0 else 0.0)
    # the rows of out slots 3 and 4 of unit 1 (original rows 0 and 4) in the order of its in slots
    W1 = flat_w[40 * 37:].reshape(5, 40)
    colmap = mp.colmaps[1][1]
    for rr, row in enumerate((0, 4)):
        for s in range(48):
            assert b[P.wsdf_off + 48 * rr + s] == (W1[row, colmap[s]] if colmap[s] >= 0 else 0.0)


def test_bf16_planes_split():
    """plane 0 is the value rounded to bf16 (nearest even), three planes carry all 24 significand bits, two leave less
    than 2^-16 of the value (8 significand bits: each rounding leaves at most 2^-8 of what it rounds)."""
    g = np.random.default_rng(8)
    w = (g.standard_normal(4096) * np.exp2(g.integers(-12, 4, 4096))).astype(np.float32)
    w[:4] = [0.0, 1.0, 1.00390625, 1.01171875]              # the last two are ties of the first rounding
    p = pk.bf16_planes(w, 3)
    v = _bf16_value(p)
    assert (v[0, :4] == [0.0, 1.0, 1.0, 1.015625]).all()     # ties to even
    assert (np.abs(v[0] - w) <= np.abs(w.astype(np.float64)) * 2.0 ** -8).all()
    assert (v.sum(0) == w.astype(np.float64)).all()
    assert (pk.bf16_planes(w, 2) == p[:2]).all()
    assert (np.abs(v[:2].sum(0) - w) <= np.abs(w.astype(np.float64)) * 2.0 ** -16).all()
