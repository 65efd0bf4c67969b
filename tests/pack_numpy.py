"""The weight packs of the fused MLP kernels, restated in numpy from an MlpPlan's rules and maps (what
msdf_pack_weights writes: csrc/sdf_mlp.hip, csrc/sdf_mlp_b16.hip).

A pack unit multiplies a slot vector: its "slot matrix" S [16 ot, 16 kt] holds scale * W[rowmap[rs], colmap[cs]] at
(rs, cs), zero where either map says -1.  The kernels read S in fragment order (csrc/mlp_core.h): the 16-byte element of
lane l = (row l & 15, quarter l >> 4) in block (row tile rt, k tile kt) holds S[16 rt + (l & 15)][16 kt + 4 (l >> 4) + 0..3].

  fp32    forward      [even(ot)][ktp][64] float4 of S      at float4 offset layer.wf_off
          transposed   [even(kt)][otp][64] float4 of S^T    at float4 offset layer.wb_off
  bf16    the same two orientations with k blocks of 32 slots (two k tiles: 8 values per lane, tile 2 kb then 2 kb + 1),
          every value split into `planes` bf16 (round to nearest even, the remainder w - float(h) exact in fp32):
          [even(row tiles)][k blocks][planes][64] x 8 bf16  at 16-byte offsets wf_off / wb_off of build_b16(planes)
  bpack   per unit the bias row [16 ot] in out-slot order at bias_off; behind the last unit `out_rows` rows of S
          (out slots sdf_slot ...) in in-slot order at wsdf_off

Every function returns (values, covered): flat arrays of the whole buffer and the mask of the elements the plan covers
(the bf16 plans leave gaps: their offsets are padded to whole LDS chunks)."""
import numpy as np
import torch


def _even(n):
    return (n + 1) & ~1


def slot_matrix(mp, u, flat_w):
    """S of pack unit u, fp32: scale * W as one fp32 multiply."""
    L, R = mp.plan.layer[u], mp.rules[u]
    rowmap, colmap = mp.rowmaps[u][1], mp.colmaps[u][1]
    W = np.asarray(flat_w, np.float32)[R.w_off:R.w_off + R.rows * R.cols].reshape(R.rows, R.cols)
    S = np.zeros((16 * L.ot, 16 * L.kt), np.float32)
    rs, cs = np.nonzero(rowmap >= 0)[0], np.nonzero(colmap >= 0)[0]
    S[np.ix_(rs, cs)] = np.float32(R.scale) * W[np.ix_(rowmap[rs], colmap[cs])]
    return S


def _padded(S, rows, cols):
    out = np.zeros((rows, cols), np.float32)
    out[:S.shape[0], :S.shape[1]] = S
    return out


def fragments(M, per_lane):
    """M [16 RT, K] -> [RT][K / (4 n)][64 lanes][per_lane = 4 n]: lane (p, q) of block (rt, kb) holds, for each of the
    n k tiles of the block in turn, M[16 rt + p][16 tile + 4 q + 0..3]."""
    n = per_lane // 4
    RT, KB = M.shape[0] // 16, M.shape[1] // (16 * n)
    # M[rt, p, kb, tile in block, q, r] -> [rt, kb, q, p, tile in block, r]; lane = 16 q + p
    return M.reshape(RT, 16, KB, n, 4, 4).transpose(0, 2, 4, 1, 3, 5).reshape(RT, KB, 64, per_lane)


def bpack(mp, flat_w, flat_b):
    P = mp.plan
    out = np.zeros(mp.bpack_f, np.float32)
    covered = np.zeros(mp.bpack_f, bool)
    flat_b = np.asarray(flat_b, np.float32)
    for u in range(P.n_layers):
        L, R = P.layer[u], mp.rules[u]
        rowmap = mp.rowmaps[u][1]
        out[L.bias_off:L.bias_off + 16 * L.ot] = np.where(rowmap >= 0, flat_b[R.b_off + np.maximum(rowmap, 0)], 0.0)
        covered[L.bias_off:L.bias_off + 16 * L.ot] = True
    u = P.n_layers - 1
    if P.wsdf_off >= 0:
        S, w = slot_matrix(mp, u, flat_w), 16 * P.layer[u].kt
        out[P.wsdf_off:P.wsdf_off + P.out_rows * w] = S[P.sdf_slot:P.sdf_slot + P.out_rows].reshape(-1)
        covered[P.wsdf_off:P.wsdf_off + P.out_rows * w] = True
    return out, covered


def wpack_f32(mp, flat_w):
    """float32 [4 * wpack_f4]"""
    out = np.zeros(4 * mp.wpack_f4, np.float32)
    covered = np.zeros(out.shape, bool)
    for u in range(mp.plan.n_layers):
        L = mp.plan.layer[u]
        S = slot_matrix(mp, u, flat_w)
        for off, M in ((L.wf_off, _padded(S, 16 * _even(L.ot), 16 * L.ktp)),
                       (L.wb_off, _padded(S.T, 16 * _even(L.kt), 16 * L.otp))):
            out[4 * off:4 * off + M.size] = fragments(M, 4).reshape(-1)
            covered[4 * off:4 * off + M.size] = True
    return out, covered


def bf16_planes(w, planes):
    """w (float32 array) -> [planes, ...] int16 bit patterns: h = bf16(w) round-to-nearest-even, w -= float(h), again."""
    w = torch.from_numpy(np.ascontiguousarray(w, np.float32)).clone()
    out = []
    for _ in range(planes):
        h = w.to(torch.bfloat16)
        out.append(h.view(torch.int16).numpy().copy())
        w -= h.float()
    return np.stack(out)


def wpack_b16(mp, planes, flat_w):
    """int16 bit patterns [8 * wpack16_units(planes)]"""
    p16 = mp.build_b16(planes)
    out = np.zeros(8 * mp.wpack16_units(planes), np.int16)
    covered = np.zeros(out.shape, bool)
    for u in range(p16.n_layers):
        L = p16.layer[u]
        S = slot_matrix(mp, u, flat_w)
        for off, M in ((L.wf_off, _padded(S, 16 * _even(L.ot), 32 * L.ktp)),
                       (L.wb_off, _padded(S.T, 16 * _even(L.kt), 32 * L.otp))):
            pl = bf16_planes(fragments(M, 8), planes)             # [planes][RT][KB][64][8]
            img = pl.transpose(1, 2, 0, 3, 4).reshape(-1)         # [RT][KB][planes][64][8]
            out[8 * off:8 * off + img.size] = img
            covered[8 * off:8 * off + img.size] = True
    return out, covered
