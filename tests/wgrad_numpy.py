"""Numpy restatement of what a weight-gradient program (plan.WgradProgram) computes, for the tests.

Written from the ABI comments of include/monosdf_plan.h (msdf_wgrad_item_t, msdf_reduce_rule_t), at the level of the
RESULT: an item contributes the sum over ALL P_pad points of X[p][0:wx]^T Y[p][0:wy] (and, where asked for, the column
sums of X and sum_p v[p] Y[p][:]); a reduce rule adds the items whose partial blocks lie in its block range, multiplies
by its scale in fp32 and scatters through its slot maps.  The per-split partial blocks are never formed, so the result
does not depend on the split counts: that is the property the kernels have to reproduce.

Sums are formed in float64 and cast to fp32 once.  With the integer-valued operands of the exact tests every value on
the way is an integer below 2^24, so the cast is exact and so is any fp32 summation order on the device."""
import hashlib

import numpy as np


def bf16_round(x):
    """fp32 -> nearest bf16 (ties to even), returned as fp32.  Finite inputs only."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    r = (b + np.uint32(0x7fff) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)
    return r.view(np.float32)


def bf16_split(x):
    """The bf16x3 kernel's operand split: hi = bf16(x), lo = bf16(x - hi), both as fp32."""
    x = np.ascontiguousarray(x, np.float32)
    hi = bf16_round(x)
    return hi, bf16_round(x - hi)


def operand(bufs, ref, ld, w, P_pad):
    """View [P_pad, w] of the operand at (buffer name, float offset) with row pitch ld."""
    buf = bufs[ref[0]]
    off = int(ref[1])
    assert off >= 0 and off + (P_pad - 1) * ld + w <= buf.size, (ref, ld, w, P_pad, buf.size)
    return np.lib.stride_tricks.as_strided(buf[off:], shape=(P_pad, w), strides=(4 * ld, 4), writeable=False)


def _matrix(X, Y, mode):
    if mode == 'fp32':
        return X.astype(np.float64).T @ Y.astype(np.float64)
    assert mode == 'bf16x3', mode
    xh, xl = (a.astype(np.float64) for a in bf16_split(X))
    yh, yl = (a.astype(np.float64) for a in bf16_split(Y))
    d = xh.T @ yh                       # lo * lo is dropped: three products
    if yl.any():
        d += xh.T @ yl
    if xl.any():
        d += xl.T @ yh
    return d


def item_terms(it, bufs, P_pad, mode='fp32', cache=None):
    """{'part' | 'colsum' | 'vrow': (float offset of the item's partial blocks, floats per block, float64 full-range sum)}.
    cache: dict shared between programs over the same buffers (the sums depend on the operands only, not on the split
    counts or the partial offsets)."""
    key = (mode, it['x'], it['y'], it['v'], it['x_ld'], it['y_ld'], it['wx'], it['wy'],
           it['colsum_off'] >= 0, it['vrow_off'] >= 0, P_pad)
    if cache is not None and key in cache:
        sums = cache[key]
    else:
        wx, wy = it['wx'], it['wy']
        X = operand(bufs, it['x'], it['x_ld'], wx, P_pad)
        sums = {}
        if wy > 0:
            Y = operand(bufs, it['y'], it['y_ld'], wy, P_pad)
            sums['part'] = _matrix(X, Y, mode)
        if it['colsum_off'] >= 0:
            sums['colsum'] = X.sum(axis=0, dtype=np.float64)
        if it['vrow_off'] >= 0:
            v = operand(bufs, it['v'], 1, 1, P_pad)[:, 0].astype(np.float64)
            sums['vrow'] = v @ Y.astype(np.float64)
        if cache is not None:
            cache[key] = sums
    out = {}
    for name, off in (('part', it['part_off']), ('colsum', it['colsum_off']), ('vrow', it['vrow_off'])):
        if name in sums:
            out[name] = (int(off), int(sums[name].size), sums[name])
    return out


def rule_slots(r, maps_np):
    """Destination rows / columns (or -1) of the rule's wx x wy slots."""
    rows = np.asarray(maps_np[r.rowmap_off:r.rowmap_off + r.wx] if r.rowmap_off >= 0 else np.full(r.wx, r.fixed_row),
                      np.int64)
    cols = np.asarray(maps_np[r.colmap_off:r.colmap_off + r.wy] if r.colmap_off >= 0 else np.zeros(r.wy), np.int64)
    return rows, cols


def reference_grad(prog, maps_np, bufs, P_pad, n_total, init=np.nan, mode='fp32', cache=None, counts=None):
    """Flat fp32 gradient [n_total] of a program over the operand buffers `bufs` (name -> flat fp32 array).
    Elements no rule stores to keep `init`.  counts: optional int array [n_total], incremented per store."""
    dst = np.full(n_total, init, np.float32)
    terms = []
    for it in prog.items:
        for off, size, val in item_terms(it, bufs, P_pad, mode, cache).values():
            terms.append((off, size * it['n_splits'], size, val))
    used = 0
    for r in prog.rules:
        n = r.wx * r.wy
        lo, hi = r.part_off, r.part_off + r.n_blocks * n
        total, blocks = np.zeros(n, np.float64), 0
        for off, span, size, val in terms:
            if lo <= off and off + span <= hi:
                assert size == n and (off - lo) % n == 0, 'a partial block of another shape inside a rule'
                total += val.reshape(-1)
                blocks += span // size
                used += 1
            else:
                assert off + span <= lo or hi <= off, 'a partial block straddles a rule'
        assert blocks == r.n_blocks, 'rule reads %d blocks, items write %d of them' % (r.n_blocks, blocks)
        val = (np.float32(r.scale) * total.astype(np.float32)).reshape(r.wx, r.wy)
        rows, cols = rule_slots(r, maps_np)
        ri, ci = np.nonzero(rows >= 0)[0], np.nonzero(cols >= 0)[0]
        if ri.size == 0 or ci.size == 0:
            continue
        idx = r.dst_off + rows[ri][:, None] * r.dst_ld + cols[ci][None, :]
        assert idx.min() >= 0 and idx.max() < n_total
        dst[idx] = val[np.ix_(ri, ci)]
        if counts is not None:
            np.add.at(counts, idx.reshape(-1), 1)
    assert used == len(terms), 'an item product that no rule reads'
    return dst


def terms_per_rule(prog):
    """Largest number of items whose blocks one reduce rule adds (the two-term layers: 2)."""
    most = 0
    for r in prog.rules:
        lo, hi = r.part_off, r.part_off + r.n_blocks * r.wx * r.wy
        n = 0
        for it in prog.items:
            offs = [it['part_off']] if it['wy'] > 0 else []
            offs += [o for o in (it['colsum_off'], it['vrow_off']) if o >= 0]
            n += sum(1 for o in offs if lo <= o < hi)
        most = max(most, n)
    return most


def split_ranges(n_stages, n_splits):
    """Stage range [begin, end) of every split: the ceiling division of the item ABI, clipped (a split may be empty)."""
    from monosdf_amd import plan as planlib
    return [planlib.split_range(n_stages, n_splits, s) for s in range(n_splits)]


def program_digest(prog, mp):
    """What a program hands to the device, as recorded in tests/golden/wgrad_programs.json: SHA-256 of the item table,
    the workgroup map and the reduce rules, the size of the partial buffer and the zero-fill decision.  Uses nothing
    of a program but items_bytes / wg_map / rules_bytes / part_f / writes_every_element."""
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    return {'items': sha(prog.items_bytes()), 'wg_map': sha(prog.wg_map()), 'rules': sha(prog.rules_bytes()),
            'part_f': int(prog.part_f), 'full': bool(prog.writes_every_element(mp.n_w + mp.n_b, mp.maps_np))}


def headline_plans():
    """name -> (MlpPlan, program builder, workspace layout, headline P_pad) of the four networks the tests run: the
    8 x 256 SDF network, the SDF network behind the hash grid, the colour network and the 64-wide SDF network."""
    from monosdf_amd import plan as planlib
    sdf, color = (planlib.build_sdf_wgrad, planlib.sdf_workspace), (planlib.build_color_wgrad, planlib.color_workspace)
    return {
        'mlp': (planlib.build_sdf_plan([(256, 39), (256, 256), (256, 256), (217, 256), (256, 256), (256, 256),
                                        (256, 256), (256, 256), (257, 256)], [4], 6, 0, False, 256),) + sdf + (104448,),
        'grid': (planlib.build_sdf_plan([(256, 71), (256, 256), (257, 256)], [4], 6, 32, True, 256),) + sdf + (104448,),
        'color': (planlib.build_color_plan([(256, 289), (256, 256), (3, 256)], 'idr', 4, 256),) + color + (100352,),
        'sdf64': (planlib.build_sdf_plan([(64, 39), (64, 64), (65, 64)], [], 6, 0, False, 64),) + sdf + (100352,),
    }
