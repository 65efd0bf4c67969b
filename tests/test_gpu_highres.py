"""GPU tests of utils/highres_cues.py against the float64 restatement (tests/highres_numpy.py), which
test_highres_cpu.py pins to the reference's recorded outputs and whose inputs it shows to be well conditioned.

Depth bar: max |gpu - restatement| / max |mosaic| <= 2 g_ref(case), g_ref being the recorded distance of the
reference's own fp32 chain from the restatement on the same inputs (tests/golden/highres/<case>.npz), before and after
the final normalisation, with the factor 2 of every reference-sensitivity bar of this project.  The per-step scale and
shift are held to the same relative bar.  Normal bar: 1e-9 absolute on output and rotations: an fp64 device SVD
perturbs the correlation matrix by about 1e-15 relative, the rotation moves by at most that over the conditioning
0.01 that test_highres_cpu.py asserts, four orders of magnitude below the bar."""
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

pytestmark = pytest.mark.gpu

DEPTH_CASES = sorted(k for k in hc.CASES if 'depth' in hc.cues(k))
NORMAL_CASES = sorted(k for k in hc.CASES if 'normal' in hc.cues(k))


def _hr():
    from monosdf_amd.utils import highres_cues
    return highres_cues


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def golden(name):
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'highres', '%s.npz' % name))


@functools.lru_cache(maxsize=None)
def depth_reference(name):
    """The restatement of every image of the case, computed once and never written to."""
    patches, mid = hc.depth_inputs(name)
    return [hn.merge_depth(patches[n], hc.CASES[name]['S'], None if mid is None else mid[n])
            for n in range(len(patches))]


@functools.lru_cache(maxsize=None)
def normal_inputs(name):
    """The case's normals decoded on the host as numpy decodes them (fp32), which is what the kernels are given."""
    patches, mid = hc.normal_inputs(name)
    return hc.decode(patches), None if mid is None else hc.decode(mid)


@functools.lru_cache(maxsize=None)
def normal_reference(name):
    patches, mid = normal_inputs(name)
    return [hn.merge_normals(patches[n], hc.CASES[name]['S'], None if mid is None else mid[n])
            for n in range(len(patches))]


@functools.lru_cache(maxsize=None)
def gpu_depth(name, normalize=True):
    patches, mid = hc.depth_inputs(name)
    out, steps = _hr().merge_depth(_cuda(patches), hc.CASES[name]['S'], _cuda(mid), normalize=normalize,
                                   return_steps=True)
    assert out.dtype == torch.float32 and out.is_cuda and steps.dtype == torch.float64
    assert tuple(out.shape) == (len(patches),) + hc.mosaic_size(hc.CASES[name])
    assert tuple(steps.shape) == (len(patches), hc.step_count(hc.CASES[name]), 2)
    return out.cpu().numpy(), steps.cpu().numpy()


@functools.lru_cache(maxsize=None)
def gpu_normals(name):
    patches, mid = normal_inputs(name)
    out, steps = _hr().merge_normals(_cuda(patches), hc.CASES[name]['S'], _cuda(mid), encoded=False, return_steps=True)
    assert out.dtype == torch.float64 and out.is_cuda and steps.dtype == torch.float64
    assert tuple(out.shape) == (len(patches), 3) + hc.mosaic_size(hc.CASES[name])
    assert tuple(steps.shape) == (len(patches), hc.step_count(hc.CASES[name]), 3, 3)
    return out.cpu().numpy(), steps.cpu().numpy()


# ---------------------------------------------------------------- depth

@pytest.mark.parametrize('name', DEPTH_CASES)
def test_depth_within_twice_the_references_own_gap(name, errlog):
    g = golden(name)
    bar_raw, bar_out = 2.0 * float(g['depth_gap_raw']), 2.0 * float(g['depth_gap_out'])
    raw, steps = gpu_depth(name, False)
    out, steps_out = gpu_depth(name, True)
    assert np.array_equal(steps, steps_out)
    for n, ref in enumerate(depth_reference(name)):
        err_raw = hn.relative_gap(raw[n], ref['raw'], ref['raw'])
        err_out = hn.relative_gap(out[n], ref['out'], ref['out'])
        err_steps = hn.relative_gap(steps[n], ref['steps'], ref['steps']) if len(ref['steps']) else 0.0
        print(name, n, 'raw %.3g (bar %.3g)  out %.3g (bar %.3g)  steps %.3g' % (err_raw, bar_raw, err_out, bar_out,
                                                                               err_steps))
        errlog('highres_depth', name, 'raw[%d]' % n, err_raw, bar_raw)
        errlog('highres_depth', name, 'out[%d]' % n, err_out, bar_out)
        errlog('highres_depth', name, 'steps[%d]' % n, err_steps, bar_raw)
        assert np.isfinite(out[n]).all()
        assert err_raw <= bar_raw and err_out <= bar_out and err_steps <= bar_raw


def test_depth_singular_fit_gives_exact_zeros():
    case = hc.CASES['c7']
    k = hc.row_step(case, *case['zero'])
    steps = gpu_depth('c7', False)[1][0]
    assert steps[k].tolist() == [0.0, 0.0] and not np.signbit(steps[k]).any()
    assert (np.delete(steps, k, axis=0)[:, 0] != 0).all()
    # what the zeros do to the mosaic is held to the restatement by test_depth_within_twice_the_references_own_gap
    assert depth_reference('c7')[0]['steps'][k].tolist() == [0.0, 0.0]


def test_depth_negative_scale_survives():
    case = hc.CASES['c8']
    k = hc.row_step(case, *case['negative'])
    steps = gpu_depth('c8', False)[1][0]
    want = depth_reference('c8')[0]['steps']
    assert steps[k, 0] < -0.1 and np.array_equal(np.sign(steps[:, 0]), np.sign(want[:, 0]))


# ---------------------------------------------------------------- normals

@pytest.mark.parametrize('name', NORMAL_CASES)
def test_normals_within_1e_9_of_the_restatement(name, errlog):
    out, steps = gpu_normals(name)
    for n, ref in enumerate(normal_reference(name)):
        err_out = float(np.abs(out[n] - ref['out']).max())
        err_rot = float(np.abs(steps[n] - ref['steps']).max()) if len(ref['steps']) else 0.0
        length = np.linalg.norm(2.0 * out[n] - 1.0, axis=0)
        err_len = float(np.abs(length - 1.0).max())
        print(name, n, 'output %.3g  rotations %.3g  |length - 1| %.3g' % (err_out, err_rot, err_len))
        errlog('highres_normals', name, 'out[%d]' % n, err_out, 1e-9)
        errlog('highres_normals', name, 'rotations[%d]' % n, err_rot, 1e-9)
        errlog('highres_normals', name, 'length[%d]' % n, err_len, 1e-12)
        assert err_out <= 1e-9 and err_rot <= 1e-9
        assert err_len <= 1e-12                             # also after the centre fit's rotation
        if len(steps[n]):
            assert np.abs(steps[n] @ np.swapaxes(steps[n], 1, 2) - np.eye(3)).max() <= 1e-13
            assert np.abs(np.linalg.det(steps[n]) - 1.0).max() <= 1e-13


def test_normals_reflection_branch():
    case = hc.CASES['c9']
    k = hc.row_step(case, *case['improper'])
    ref = normal_reference('c9')[0]
    assert ref['d'][k] == -1.0
    assert np.abs(gpu_normals('c9')[1][0][k] - ref['steps'][k]).max() <= 1e-9


def test_encoded_input_is_decoded_as_the_host_decodes():
    """The fp32 decode on the device may differ from the host's in the last place of a division or a square root:
    2^-22 = 2.4e-7 per component at most.  Were every component off by that much, a correlation matrix would move by
    2.4e-7 relative and its rotation by at most that over the conditioning (>= 0.07 on case 1): 3.4e-6 a step, and an
    image's longest chain of dependent steps here is 3 + 2 + 1, so 1e-4 bounds the merge of it with room."""
    hr = _hr()
    patches, mid = hc.normal_inputs('c1')
    dev = hr.decode_normals(_cuda(patches)).cpu().numpy()
    assert dev.dtype == np.float32 and np.abs(dev - hc.decode(patches)).max() <= 2.0 ** -22
    out = hr.merge_normals(_cuda(patches), hc.CASES['c1']['S'], _cuda(mid)).cpu().numpy()
    assert np.abs(out - gpu_normals('c1')[0]).max() <= 1e-4
    one = hr.merge_normals(_cuda(patches[0]), hc.CASES['c1']['S'], _cuda(mid[0]))
    assert tuple(one.shape) == (3,) + hc.mosaic_size(hc.CASES['c1']) and np.array_equal(one.cpu().numpy(), out[0])


# ---------------------------------------------------------------- batches, repeats, edges

def test_an_image_does_not_depend_on_its_batch():
    d6, s6 = gpu_depth('c6', True)
    d1, s1 = gpu_depth('c1', True)
    assert np.array_equal(d6[1], d1[0]) and np.array_equal(s6[1], s1[0])
    assert np.array_equal(gpu_depth('c6', False)[0][1], gpu_depth('c1', False)[0][0])
    n6, r6 = gpu_normals('c6')
    n1, r1 = gpu_normals('c1')
    assert np.array_equal(n6[1], n1[0]) and np.array_equal(r6[1], r1[0])
    assert not np.array_equal(d6[0], d6[1]) and not np.array_equal(n6[0], n6[2])


def test_two_calls_give_the_same_bits():
    hr, S = _hr(), hc.CASES['c3']['S']
    patches = _cuda(hc.depth_inputs('c3')[0])
    a, sa = hr.merge_depth(patches, S, return_steps=True)
    b, sb = hr.merge_depth(patches, S, return_steps=True)
    assert torch.equal(a, b) and torch.equal(sa, sb)
    assert np.array_equal(a.cpu().numpy(), gpu_depth('c3', True)[0])
    normals = _cuda(normal_inputs('c3')[0])
    a, sa = hr.merge_normals(normals, S, encoded=False, return_steps=True)
    b, sb = hr.merge_normals(normals, S, encoded=False, return_steps=True)
    assert torch.equal(a, b) and torch.equal(sa, sb)


def test_a_single_patch_is_returned_normalised():
    patches = hc.depth_inputs('c5_one')[0]
    raw, steps = gpu_depth('c5_one', False)
    assert np.array_equal(raw[0], patches[0, 0, 0]) and steps.shape == (1, 0, 2)
    p = patches[0, 0, 0].astype(np.float64)
    want = ((p - p.min()) / (p.max() - p.min())).astype(np.float32)
    out = gpu_depth('c5_one', True)[0][0]
    assert np.array_equal(out, want) and out.min() == 0.0 and out.max() == 1.0
    normals = normal_inputs('c5_one')[0]
    got = gpu_normals('c5_one')[0][0]
    n = normals[0, 0, 0].astype(np.float64)
    n = n / (np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]) + 1e-15)[None]
    # divided by its fp64 length once and nothing else: a square root, a division and (n + 1) / 2, each within an
    # ulp of values below 1
    assert np.abs(got - (n + 1.0) / 2.0).max() <= 4 * 2.0 ** -53
    # one image without the batch dimension
    single = _hr().merge_depth(_cuda(patches[0]), hc.CASES['c5_one']['S'])
    assert tuple(single.shape) == (12, 12) and np.array_equal(single.cpu().numpy(), out)


def test_arguments_are_refused():
    hr = _hr()
    good = _cuda(hc.depth_inputs('c4')[0])
    with pytest.raises(TypeError, match='^merge_depth: patches must be torch.float32'):
        hr.merge_depth(good.double(), 8)
    with pytest.raises(ValueError, match='^mosaic_size'):
        hr.merge_depth(good, 19)
    with pytest.raises(ValueError, match='^merge_depth: mid must be'):
        hr.merge_depth(good, 8, mid=good[:, 0, 0, :10])
    with pytest.raises(ValueError, match='^merge_depth: patches must be square'):
        hr.merge_depth(good[..., :10], 8)
    with pytest.raises(TypeError, match='^merge_depth: mid must be a CUDA tensor'):
        hr.merge_depth(good, 8, mid=good[:, 0, 0].cpu())
    with pytest.raises(ValueError, match='^merge_normals: patches must be'):
        hr.merge_normals(good.unsqueeze(3), 8)


# ---------------------------------------------------------------- files

def test_merge_scan_writes_what_the_calls_return(tmp_path):
    hr, case = _hr(), hc.CASES['c6']
    depth, mid_d = hc.depth_inputs('c6')
    normal, mid_n = hc.normal_inputs('c6')
    src, dst = tmp_path / 'patches', tmp_path / 'out'
    src.mkdir()
    for n in range(len(depth)):
        for j in range(case['R']):
            for i in range(case['C']):
                np.save(src / ('%06d_%02d_%02d_depth.npy' % (n, j, i)), depth[n, j, i])
                np.save(src / ('%06d_%02d_%02d_normal.npy' % (n, j, i)), normal[n, j, i])
        np.save(src / ('%06d_mid_depth.npy' % n), mid_d[n])
        np.save(src / ('%06d_mid_normal.npy' % n), mid_n[n])
    done = hr.merge_scan(str(src), str(dst), rows=case['R'], cols=case['C'], patch=case['P'], stride=case['S'], batch=2)
    assert done == [0, 1, 2]
    want_d = hr.merge_depth(_cuda(depth), case['S'], _cuda(mid_d)).cpu().numpy()
    want_n = hr.merge_normals(_cuda(normal), case['S'], _cuda(mid_n)).cpu().numpy()
    assert np.array_equal(want_d, gpu_depth('c6', True)[0])
    for n in range(len(depth)):
        d = np.load(dst / ('%06d_depth.npy' % n))
        v = np.load(dst / ('%06d_normal.npy' % n))
        assert d.dtype == np.float32 and v.dtype == np.float64
        assert np.array_equal(d, want_d[n]) and np.array_equal(v, want_n[n])
        for kind in ('depth', 'normal'):
            png = dst / ('%06d_%s.png' % (n, kind))
            assert png.exists() and png.read_bytes()[:8] == b'\x89PNG\r\n\x1a\n'
