"""CPU tests of the high-resolution cue merge: the workspace sizes and the host-side refusals of the msdf_hrc_* entry
points; the regenerated inputs (tests/highres_cases.py) against their recorded hashes; the float64 restatement
(tests/highres_numpy.py) against what the reference's own functions returned (tests/golden/highres/*.npz, written by
scripts/make_golden_highres.py); the conditions on the inputs that give the GPU bars of test_gpu_highres.py their
meaning; and decode_normals against numpy."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import highres_cases as hc
import highres_numpy as hn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GAP_CAP = 1e-3                     # every recorded depth gap lies below this: a condition, not a measurement


def golden(name):
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'highres', '%s.npz' % name))


@functools.lru_cache(maxsize=None)
def restated_depth(name):
    patches, mid = hc.depth_inputs(name)
    return [hn.merge_depth(patches[n], hc.CASES[name]['S'], None if mid is None else mid[n])
            for n in range(len(patches))]


@functools.lru_cache(maxsize=None)
def restated_normals(name):
    patches, mid = hc.normal_inputs(name)
    return [hn.merge_normals(hc.decode(patches[n]), hc.CASES[name]['S'], None if mid is None else hc.decode(mid[n]))
            for n in range(len(patches))]


# ---------------------------------------------------------------- the library (header and table: test_abi_cpu.py)

def test_library_exports_the_highres_entries():
    from monosdf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('library not built (run python __graft_entry__.py)')
    lib = _lib.load()
    ws = lib.msdf_hrc_workspace_bytes
    # one image, 1 x 1 patches of 12: no strips; 2 minimum / maximum partials + the pair itself; 256 spare bytes
    assert ws(1, 1, 1, 12, 4, 1) == (4 + 2) * 8 + 256
    # depth at full size: partial sums of the largest launch (the last kernels: 1152 tiles x 2 per image, against
    # 7 x 48 x 4 of a row step), 2 per image, and 6 strips of 384 x 2048 fp32 per image
    assert ws(8, 7, 14, 384, 128, 1) == (8 * 1152 * 2 + 16) * 8 + 8 * 6 * 384 * 2048 * 4 + 256
    assert ws(2, 2, 3, 384, 128, 3) == (2 * 2 * 48 * 9 + 4) * 8 + 2 * 1 * 3 * 384 * 640 * 8 + 256
    # refused on the host, before anything is launched: sizes out of range, an overlap below 2, null pointers
    bad = [(0, 1, 1, 12, 4), (-1, 1, 1, 12, 4), (65537, 1, 1, 12, 4), (1, 0, 1, 12, 4), (1, 1, 0, 12, 4),
           (1, 1025, 1, 12, 4), (1, 1, 1025, 12, 4), (1, 1, 1, 12, 0), (1, 1, 1, 12, 12), (1, 1, 1, 12, 13),
           (1, 1, 1, 12, 11), (1, 1, 1, 16385, 4), (1, 1, 1, 1, 0), (1, 1024, 1024, 16384, 16000),
           (65536, 1024, 1024, 384, 128), (2 ** 40, 1, 1, 12, 4)]
    for n, r, c, p, s in bad:
        for ch in (1, 3):
            assert ws(n, r, c, p, s, ch) == -1, (n, r, c, p, s)
        assert lib.msdf_hrc_merge_depth(None, None, n, r, c, p, s, 1, None, None, None, None) == 1, (n, r, c, p, s)
        assert lib.msdf_hrc_merge_normals(None, None, n, r, c, p, s, None, None, None, None) == 1, (n, r, c, p, s)
    for ch in (0, 2, 4, -1):
        assert ws(1, 1, 1, 12, 4, ch) == -1
    assert ws(1, 1, 1, 12, 10, 1) > 0                               # an overlap of exactly 2
    assert lib.msdf_hrc_merge_depth(None, None, 1, 2, 2, 12, 4, 1, None, None, None, None) == 1
    assert lib.msdf_hrc_merge_normals(None, None, 1, 2, 2, 12, 4, None, None, None, None) == 1


def test_python_surface_without_a_gpu():
    from monosdf_amd.utils import highres_cues as hr
    assert hr.mosaic_size(7, 14, 384, 128) == (1152, 2048)
    assert hr.mosaic_size(2, 3, 20, 8) == (28, 36) and hr.mosaic_size(1, 1, 12, 4) == (12, 12)
    assert hr.step_count(7, 14, True) == 7 * 13 + 6 + 1 and hr.step_count(1, 1) == 0
    for bad in ((1, 1, 12, 12), (1, 1, 12, 0), (1, 1, 12, 11), (0, 1, 12, 4), (1, 0, 12, 4)):
        with pytest.raises(ValueError, match='^mosaic_size'):
            hr.mosaic_size(*bad)
    # a CPU tensor raises, as everywhere in this project
    with pytest.raises(TypeError, match='^merge_depth: patches must be a CUDA tensor'):
        hr.merge_depth(torch.zeros(1, 2, 2, 12, 12), 4)
    with pytest.raises(TypeError, match='^merge_normals: patches must be a CUDA tensor'):
        hr.merge_normals(torch.zeros(1, 2, 2, 3, 12, 12), 4)
    for case in hc.CASES.values():
        assert hc.mosaic_size(case) == hr.mosaic_size(case['R'], case['C'], case['P'], case['S'])
        assert hc.step_count(case) == hr.step_count(case['R'], case['C'], case['mid'])
    script = open(os.path.join(ROOT, 'scripts', 'merge_highres_cues.py')).read()
    assert 'merge_scan' in script


# ---------------------------------------------------------------- the inputs are the recorded ones

@pytest.mark.parametrize('name', sorted(hc.CASES))
def test_regenerated_inputs_hash_to_the_recorded_values(name):
    arrays = []
    if 'depth' in hc.cues(name):
        arrays += list(hc.depth_inputs(name))
    if 'normal' in hc.cues(name):
        arrays += list(hc.normal_inputs(name))
    assert hc.sha256(*arrays) == str(golden(name)['sha256'])


def test_case_6_holds_case_1():
    assert np.array_equal(hc.depth_inputs('c6')[0][1], hc.depth_inputs('c1')[0][0])
    assert np.array_equal(hc.depth_inputs('c6')[1][1], hc.depth_inputs('c1')[1][0])
    assert np.array_equal(hc.normal_inputs('c6')[0][1], hc.normal_inputs('c1')[0][0])
    assert np.array_equal(hc.normal_inputs('c6')[1][1], hc.normal_inputs('c1')[1][0])
    assert not np.array_equal(hc.depth_inputs('c6')[0][0], hc.depth_inputs('c6')[0][2])


# ---------------------------------------------------------------- the restatement against the reference's outputs

@pytest.mark.parametrize('name', hc.RECORDED_OUTPUTS)
def test_normal_restatement_equals_the_reference(name):
    """1e-12 absolute: the restatement repeats the reference's float64 operations (measured: below 1e-15); the room is
    for another BLAS's summation order at the conditioning asserted below."""
    g = golden(name)
    for n, res in enumerate(restated_normals(name)):
        err_out = np.abs(res['out'] - g['normal_out'][n]).max()
        err_rot = np.abs(res['steps'] - g['normal_steps'][n]).max()
        print(name, 'normals: output', err_out, 'rotations', err_rot)
        assert err_out <= 1e-12 and err_rot <= 1e-12
        assert res['out'].dtype == np.float64 and res['out'].shape == (3,) + hc.mosaic_size(hc.CASES[name])


@pytest.mark.parametrize('name', sorted(hc.CASES))
def test_depth_restatement_reproduces_the_recorded_gaps(name):
    """The gap g_ref between the reference's fp32 chain and the restatement is what the GPU is held to (twice it).
    Where the reference's output is stored the gap is measured again from it; everywhere it lies below GAP_CAP and the
    normal gaps below 1e-12."""
    g = golden(name)
    if 'normal' in hc.cues(name):
        # a 1 x 1 grid runs none of the reference's functions; the restatement divides it by its float64 length, which
        # the fp32 decode leaves within 2^-23 of one, and (n + 1) / 2 halves that
        one = hc.CASES[name]['R'] == hc.CASES[name]['C'] == 1
        assert float(g['normal_gap']) <= (2.0 ** -24 if one else 1e-12) and float(g['normal_gap_steps']) <= 1e-12
    if 'depth' not in hc.cues(name):
        return
    raw, out = float(g['depth_gap_raw']), float(g['depth_gap_out'])
    print(name, 'depth gaps', raw, out)
    assert 0.0 <= raw < GAP_CAP and 0.0 <= out < GAP_CAP
    if name in hc.RECORDED_OUTPUTS:
        for n, res in enumerate(restated_depth(name)):
            assert hn.relative_gap(g['depth_raw'][n], res['raw'], res['raw']) <= raw
            assert hn.relative_gap(g['depth_out'][n], res['out'], res['out']) <= out
            # the reference's fp32 coefficients: within the same relative distance of the restatement's
            assert hn.relative_gap(g['depth_steps'][n], res['steps'], res['steps']) <= 10 * raw
        got = max(hn.relative_gap(g['depth_raw'][n], r['raw'], r['raw']) for n, r in enumerate(restated_depth(name)))
        assert got == raw


@pytest.mark.parametrize('variant', [dict(fade='reversed'), dict(fit='mosaic')])
def test_a_wrong_depth_restatement_misses_the_cap(variant):
    """The cross-fade reversed, and the mosaic fitted to the patch instead of the patch to the mosaic: each is more
    than ten times GAP_CAP away from the reference's normalised output on case 1 (measured: 78 and 13 times) and more
    than five times before the normalisation (58 and 6.8 times), so the cap tells a right restatement from these.
    The second variant differs from the right one only by regression dilution, which the noise of the depth patches
    (highres_cases.DEPTH_NOISE) is there to make visible."""
    g = golden('c1')
    patches, mid = hc.depth_inputs('c1')
    res = hn.merge_depth(patches[0], hc.CASES['c1']['S'], mid[0], **variant)
    gap_raw = hn.relative_gap(g['depth_raw'][0], res['raw'], res['raw'])
    gap_out = hn.relative_gap(g['depth_out'][0], res['out'], res['out'])
    print(variant, gap_raw, gap_out)
    assert gap_out > 10 * GAP_CAP and gap_raw > 5 * GAP_CAP


# ---------------------------------------------------------------- conditions the GPU bars rely on

@pytest.mark.parametrize('name', sorted(k for k in hc.CASES if 'normal' in hc.cues(k)))
def test_normal_cases_are_well_conditioned(name):
    """s2 + d s3 >= 0.01 s1 at every step: the rotation moves by at most the perturbation of the correlation matrix
    over this figure, which is what makes 1e-9 a wide bar for an fp64 device SVD."""
    for res in restated_normals(name):
        sv, d = res['sv'], res['d']
        if len(d) == 0:
            continue
        cond = (sv[:, 1] + d * sv[:, 2]) / sv[:, 0]
        print(name, 'd', d.astype(int).tolist(), 'conditioning', np.round(cond, 4).tolist())
        assert (cond >= 0.01).all()
        assert np.abs(np.linalg.norm(res['raw'], axis=0) - 1.0).max() < 1e-12


def test_both_branches_of_the_rotation_occur():
    d = np.concatenate([res['d'] for name in hc.CASES if 'normal' in hc.cues(name) for res in restated_normals(name)])
    assert (d == 1.0).any() and (d == -1.0).any()
    case = hc.CASES['c9']
    d9 = restated_normals('c9')[0]['d']
    assert d9[hc.row_step(case, *case['improper'])] == -1.0
    assert (d9[:hc.row_step(case, *case['improper'])] == 1.0).all()


def test_depth_determinants():
    """Every fit is regular except the one of case 7's zero patch, whose coefficients are exactly zero; case 8's
    negative scale survives to its step and changes the output."""
    for name in hc.CASES:
        if 'depth' not in hc.cues(name):
            continue
        case = hc.CASES[name]
        for res in restated_depth(name):
            singular = np.flatnonzero(res['det'] == 0)
            if 'zero' in case:
                assert singular.tolist() == [hc.row_step(case, *case['zero'])]
                assert res['steps'][singular[0]].tolist() == [0.0, 0.0]
            else:
                assert len(singular) == 0
            assert np.isfinite(res['out']).all() and res['out'].min() == 0.0 and res['out'].max() == 1.0
    case = hc.CASES['c8']
    steps = restated_depth('c8')[0]['steps']
    k = hc.row_step(case, *case['negative'])
    assert steps[k, 0] < -0.1 and (np.delete(steps[:, 0], k) > 0.1).all()


# ---------------------------------------------------------------- decode

def test_decode_normals_equals_numpy_bitwise():
    from monosdf_amd.utils import highres_cues as hr
    for name in ('c1', 'c2', 'c9'):
        patches, mid = hc.normal_inputs(name)
        want = hc.decode(patches)
        got = hr.decode_normals(torch.from_numpy(patches))
        assert got.dtype == torch.float32 and want.dtype == np.float32
        assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32))
        assert np.array_equal(hr.decode_normals(torch.from_numpy(patches[0, 0, 0])).numpy(), hc.decode(patches[0, 0, 0]))
    # the reference's own statement of it, on one patch
    v = hc.normal_inputs('c4')[0][0, 1, 2]
    n = v * 2. - 1.
    n = n / (np.linalg.norm(n, axis=0) + 1e-15)[None]
    assert np.array_equal(hr.decode_normals(torch.from_numpy(v)).numpy(), n)
    with pytest.raises(ValueError, match='^decode_normals'):
        hr.decode_normals(torch.zeros(2, 4, 4))
    with pytest.raises(TypeError, match='^decode_normals'):
        hr.decode_normals(np.zeros((3, 4, 4)))
