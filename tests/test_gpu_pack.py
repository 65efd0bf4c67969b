"""msdf_pack_weights against its numpy restatement (tests/pack_numpy.py, itself pinned by test_pack_numpy.py), element
by element with ==: the bf16 planes as bit patterns, everything else as the one fp32 multiply scale * W.  The buffers
FusedMlp.pack allocates are filled with NaN first, so an element the kernel leaves out does not compare equal."""
import numpy as np
import pytest
import torch

import pack_numpy as pk
from monosdf_amd import plan as planlib

pytestmark = pytest.mark.gpu


def _sdf_plan(aux_cols):
    # width 48 = 3 tiles (odd: the packs pad to 4), a skip layer, multires 6; with the 32 hash-feature columns the
    # network input is 5 tiles (3 k blocks of 32 for the bf16 cores) and the skip layer's input 6
    d0 = 3 + 6 * 6 + aux_cols
    return planlib.build_sdf_plan([(48, d0), (9, 48), (48, 9 + d0), (1 + 20, 48)], skip_in=[2], n_freqs=6,
                                  aux_cols=aux_cols, aux_active=aux_cols > 0, feature_size=20)


def _color_plan():
    # idr with a per-image code: the first layer as two pack units, three dot-product rows behind the last
    lead, feat, code = 3 + (3 + 6 * 4) + 3, 20, 32
    return planlib.build_color_plan([(48, lead + feat + code), (48, 48), (3, 48)], 'idr', 4, feat, code_cols=code)


PLANS = {'sdf_w48_skip': lambda: _sdf_plan(0), 'sdf_w48_skip_grid': lambda: _sdf_plan(32), 'color_code': _color_plan}


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3', 'bf16x6'])
@pytest.mark.parametrize('name', sorted(PLANS))
def test_pack_weights_exact(name, precision, monkeypatch):
    from monosdf_amd.ops import FusedMlp
    mp = PLANS[name]()
    g = torch.Generator().manual_seed(11)
    flat_w, flat_b = torch.randn(mp.n_w, generator=g), torch.randn(mp.n_b, generator=g)
    mlp = FusedMlp(mp, 'cuda', precision)
    empty = torch.empty
    monkeypatch.setattr(torch, 'empty', lambda *a, **k: empty(*a, **k).fill_(float('nan')))
    wpack, bpack = mlp.pack(flat_w.cuda(), flat_b.cuda())
    monkeypatch.undo()
    torch.cuda.synchronize()
    if precision == 'fp32':
        want, covered = pk.wpack_f32(mp, flat_w.numpy())
        got = wpack.cpu().numpy()[:len(want)]
    else:
        want, covered = pk.wpack_b16(mp, {'bf16x3': 2, 'bf16x6': 3}[precision], flat_w.numpy())
        got = wpack.cpu().view(torch.int16).numpy()[:len(want)]
    assert covered.sum() > 1000 and np.count_nonzero(want[covered]) > 1000
    bad = np.nonzero(covered & ~(got == want))[0]
    assert bad.size == 0, (name, precision, 'wpack', bad[:8], got[bad[:8]], want[bad[:8]])
    want_b, covered_b = pk.bpack(mp, flat_w.numpy(), flat_b.numpy())
    got_b = bpack.cpu().numpy()[:len(want_b)]
    bad = np.nonzero(covered_b & ~(got_b == want_b))[0]
    assert bad.size == 0, (name, precision, 'bpack', bad[:8], got_b[bad[:8]], want_b[bad[:8]])
