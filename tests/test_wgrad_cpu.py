"""Host-only checks of the weight-gradient restatement (tests/wgrad_numpy.py) and of the split arithmetic: the
interpreter against a direct einsum on hand-built programs, and on the real programs of the four networks (results
independent of the split counts, every gradient element written exactly once)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import wgrad_numpy as wn
from monosdf_amd import plan as planlib

PLANS = ('color', 'grid', 'mlp', 'sdf64')


def int_buffers(sizes, seed, lo=-3, hi=3):
    rng = np.random.default_rng(seed)
    return {k: rng.integers(lo, hi + 1, n).astype(np.float32) for k, n in sizes.items()}


def test_bf16_split_is_torch_round_to_nearest_even():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(4096).astype(np.float32) * 3,
                        # ties: exactly halfway between two bf16 values, both parities of the kept mantissa
                        np.array([1.00390625, 1.01171875, -1.00390625, 2.0 ** -10 * 3, 0.0, 3.0029296875], np.float32)])
    hi, lo = wn.bf16_split(x)
    t = torch.from_numpy(x)
    hi_t = t.bfloat16().float()
    np.testing.assert_array_equal(hi, hi_t.numpy())
    np.testing.assert_array_equal(lo, (t - hi_t).bfloat16().float().numpy())


def test_interpreter_matches_einsum_on_a_hand_built_item():
    """One item with x_ld > wx, a column offset into Y, holed maps, scale != 1; a v-weighted row through fixed_row and
    column sums through a second rule; everything else keeps the initial value."""
    P_pad, wx, wy, x_ld, y_ld, c0, S = 96, 32, 48, 80, 112, 32, 2
    prog = planlib.WgradProgram(lambda w: S, P_pad)
    part, cs, vr = prog.alloc(S * wx * wy), prog.alloc(S * wx), prog.alloc(S * wy)
    x_off, y_off, v_off = 16, 64, 7
    prog.add_item(('ws', x_off), x_ld, wx, ('feat', y_off + c0), y_ld, wy, part, S, colsum_off=cs,
                  v=('ws', x_off + P_pad * x_ld + v_off), vrow_off=vr)
    rowmap = np.full(wx, -1, np.int32)
    rowmap[:29] = 1 + np.random.default_rng(1).permutation(29)          # row 0 is the fixed row; slots 29..31 padding
    colmap = np.full(wy, -1, np.int32)
    colmap[[0, 1, 2, 5, 47, 20]] = [3, 0, 1, 2, 4, 5]
    maps = np.concatenate([np.zeros(5, np.int32), rowmap, colmap])
    rm, cm = 5, 5 + wx
    dst_ld, scale = 9, float(np.float32(np.sqrt(0.5)))
    n_w = 30 * dst_ld
    prog.add_rule(part, S, wx, wy, rm, cm, 0, dst_ld, scale)
    prog.add_rule(vr, S, 1, wy, -1, cm, 0, dst_ld, scale, fixed_row=0)
    prog.add_rule(cs, S, wx, 1, rm, -1, n_w, 1, 1.0)
    bufs = int_buffers({'ws': x_off + P_pad * x_ld + v_off + P_pad, 'feat': y_off + P_pad * y_ld}, 2)
    got = wn.reference_grad(prog, maps, bufs, P_pad, n_w + 30, init=np.nan)

    X = bufs['ws'][x_off:x_off + P_pad * x_ld].reshape(P_pad, x_ld)[:, :wx].astype(np.float64)
    Y = bufs['feat'][y_off:y_off + P_pad * y_ld].reshape(P_pad, y_ld)[:, c0:c0 + wy].astype(np.float64)
    v = bufs['ws'][x_off + P_pad * x_ld + v_off:][:P_pad].astype(np.float64)
    D = np.einsum('pi,pj->ij', X, Y)
    want = np.full(n_w + 30, np.nan, np.float32)
    W = want[:n_w].reshape(30, dst_ld)
    sc = np.float32(scale)
    for i in range(wx):
        for j in range(wy):
            if rowmap[i] >= 0 and colmap[j] >= 0:
                W[rowmap[i], colmap[j]] = sc * np.float32(D[i, j])
    for j in range(wy):
        if colmap[j] >= 0:
            W[0, colmap[j]] = sc * np.float32(np.einsum('p,p->', v, Y[:, j]))
    for i in range(wx):
        if rowmap[i] >= 0:
            want[n_w + rowmap[i]] = np.float32(X[:, i].sum())
    np.testing.assert_array_equal(got, want)
    assert np.isnan(want).sum() == 30 * 3 + 1          # three unmapped columns of every row, bias slot 0


def test_interpreter_adds_the_items_that_share_a_rule():
    P_pad, w = 64, 16
    prog = planlib.WgradProgram(lambda w: 1, P_pad)
    part = prog.alloc(3 * w * w + 4 * w * w)
    prog.add_item(('ws', 0), w, w, ('ws', P_pad * w), w, w, part, 3)
    prog.add_item(('ws', 2 * P_pad * w), w, w, ('ws', 3 * P_pad * w), w, w, part + 3 * w * w, 4)
    maps = np.arange(w, dtype=np.int32)
    prog.add_rule(part, 7, w, w, 0, 0, 0, w, 1.0)
    bufs = int_buffers({'ws': 4 * P_pad * w}, 3)
    a = bufs['ws'].reshape(4, P_pad, w).astype(np.float64)
    want = (a[0].T @ a[1] + a[2].T @ a[3]).astype(np.float32).reshape(-1)
    np.testing.assert_array_equal(wn.reference_grad(prog, maps, bufs, P_pad, w * w), want)
    # the bf16x3 definition on bf16-exact data is the plain product
    np.testing.assert_array_equal(wn.reference_grad(prog, maps, bufs, P_pad, w * w, mode='bf16x3'), want)


def test_bf16x3_mode_is_the_three_product_definition():
    P_pad, w = 64, 16
    rng = np.random.default_rng(4)
    x = (rng.integers(1, 4, (2, P_pad, w)) + rng.integers(-3, 4, (2, P_pad, w)) * 2.0 ** -10).astype(np.float32)
    prog = planlib.WgradProgram(lambda w: 1, P_pad)
    prog.add_item(('ws', 0), w, w, ('ws', P_pad * w), w, w, prog.alloc(w * w), 1)
    prog.add_rule(0, 1, w, w, 0, 0, 0, w, 1.0)
    got = wn.reference_grad(prog, np.arange(w, dtype=np.int32), {'ws': x.reshape(-1)}, P_pad, w * w, mode='bf16x3')
    t = torch.from_numpy(x)
    hi = t.bfloat16().double()
    lo = (t - hi.float()).bfloat16().double()
    want = hi[0].T @ hi[1] + hi[0].T @ lo[1] + lo[0].T @ hi[1]
    np.testing.assert_array_equal(got.reshape(w, w), want.float().numpy())
    full = (t[0].double().T @ t[1].double()).float().numpy()
    assert (got.reshape(w, w) != full).any()            # the dropped lo * lo product is visible in this data


@pytest.mark.parametrize('name', PLANS)
def test_real_programs_do_not_depend_on_the_split_counts(name):
    mp, build, wsfn, _ = wn.headline_plans()[name]
    P_pad = 128
    _, total = wsfn(mp, P_pad)
    bufs = int_buffers({'ws': total, 'feat': P_pad * 256}, 5)
    n_total = mp.n_w + mp.n_b
    results = []
    for prog in (planlib.balanced_program(build, mp, P_pad), build(mp, P_pad, lambda w: 3)):
        counts = np.zeros(n_total, np.int64)
        results.append(wn.reference_grad(prog, mp.maps_np, bufs, P_pad, n_total, counts=counts))
        assert counts.min() == 1 and counts.max() == 1      # every weight and bias written exactly once
        assert prog.writes_every_element(n_total, mp.maps_np)
    assert not np.isnan(results[0]).any() and np.abs(results[0]).max() > 0
    np.testing.assert_array_equal(results[0], results[1])


@pytest.mark.parametrize('name', PLANS)
def test_split_ranges_of_the_headline_programs_cover_every_stage_once(name):
    """The point range of an item is cut by a ceiling division, so trailing splits may be short or empty.  With the
    chooser's present constants the network behind the hash grid gets 83 splits of 3264 stages (per = 40: split 81 has
    24 stages, split 82 none) and the 48-column items of the 8 x 256 network 50 splits (last one 30 of 66 stages); an
    empty split is exercised on the device by the synthetic cases of test_gpu_wgrad.py whatever the chooser does."""
    mp, build, _, P_pad = wn.headline_plans()[name]
    n = P_pad // planlib.STAGE_POINTS
    pairs = {(n, it['n_splits']) for it in planlib.balanced_program(build, mp, P_pad).items}
    pairs |= {(n, max(1, -(-n // planlib.UNIFORM_STAGES_PER_SPLIT))), (9, 6), (3, 5), (67, 8), (1, 1)}
    for n_stages, n_splits in sorted(pairs):
        assert 1 <= n_splits
        ranges = wn.split_ranges(n_stages, n_splits)
        assert len(ranges) == n_splits
        seen = np.zeros(n_stages, np.int64)
        for b, e in ranges:
            assert 0 <= b <= e <= n_stages or (b > n_stages and b == e)
            seen[b:e] += 1
        assert (seen == 1).all(), (n_stages, n_splits)


# ---------------------------------------------------------------------------
# the programs the library hands to the device, against digests recorded before the schedule rules were named
# ---------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'wgrad_programs.json')
DIGEST_P_PADS = (64, 640, 12800, 100352, 104448)


def program_digests(names):
    """'network/P_pad/kind' -> wn.program_digest of the balanced and the bf16x3 uniform program."""
    out = {}
    for name in names:
        mp, build, _, _ = wn.headline_plans()[name]
        for P_pad in DIGEST_P_PADS:
            out['%s/%d/balanced' % (name, P_pad)] = wn.program_digest(planlib.balanced_program(build, mp, P_pad), mp)
            out['%s/%d/bf16x3' % (name, P_pad)] = wn.program_digest(planlib.uniform_program(build, mp, P_pad), mp)
    return out


def test_programs_reproduce_the_recorded_digests():
    """Item table, workgroup map, reduce rules, partial-buffer size and zero-fill decision of the four networks at five
    point counts, both program kinds: byte for byte what tests/golden/wgrad_programs.json recorded."""
    want = json.load(open(GOLDEN))['default']
    assert len(want) == len(PLANS) * len(DIGEST_P_PADS) * 2
    got = program_digests(PLANS)
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        assert got[key] == want[key], key


def test_programs_reproduce_the_recorded_digests_without_the_narrow_slowdown():
    """MSDF_WGRAD_ALL_NARROW_SLOW=0 (read when plan.py is imported, hence the subprocess) still switches the 30 % off: the
    colour network's balanced programs, two of which differ from the default ones."""
    want = json.load(open(GOLDEN))
    assert any(want['all_narrow_slow_0'][k] != want['default'][k] for k in want['all_narrow_slow_0'])
    code = ('import json, sys; sys.path[:0] = %r; import test_wgrad_cpu as t; '
            'print(json.dumps(t.program_digests(["color"])))' % [p for p in sys.path if p])
    env = dict(os.environ, MSDF_WGRAD_ALL_NARROW_SLOW='0')
    got = json.loads(subprocess.check_output([sys.executable, '-c', code], env=env).decode().strip().splitlines()[-1])
    for key, digest in sorted(want['all_narrow_slow_0'].items()):
        assert got[key] == digest, key
