"""The compositor's edge cases (tests/composite_cases.py) are fair: conditions on the INPUTS that the GPU test
(tests/test_gpu_composite_edges.py) relies on, checked on the CPU.  If one fails, the case changes, not the threshold.

  reference deviation  the fp32 oracle stays within 1e-5 (a tenth of the parity bar) of the float64 oracle: per-sample
                       tensors per 64-sample chunk, per-ray outputs and d/d beta whole -- so a kernel that misses the
                       bar on such a case cannot blame the reference's own formula;
  no hidden chunk      every chunk's largest reference weight is at least 1e-3;
  last-sample rule     every ray ends with sdf <= 0, sdf/beta <= 12 or sdf/beta >= 60 (in between, the 1e10 last interval
                       multiplies the lost digits of 0.5 + 0.5 expm1(-s/beta) and the last weight flips between 0 and T);
  coverage             every listed crossing index below S occurs, and S-2 and S-1;
  autograd             the float64 oracle's autograd stays within 1e-5 of the derivative itself (composite_cases.
                       density_smooth).  It does not everywhere: it forms e^t as expm1(t) + 1, which is 0 once expm1 has
                       saturated -- at S = 1 the whole d/d sdf reference is 0, and an escaping sample at 80 beta fails this
                       by 1e-3 (composite_cases.ESCAPE) -- and it returns 0 at sdf == 0.0 exactly, where sign(s) = 0
                       (composite_cases.with_zero_crossings: exact zeros have a GPU test of their own).
"""
import pytest
import torch

import composite_cases as cc
from helpers import rel_err
from oracle import monosdf_oracle as mo

CASES = [(S, b) for S in cc.SAMPLES for b in cc.BETAS]
PER_SAMPLE = ('weights', 'd/d sdf', 'd/d rgb', 'd/d normals')


@pytest.fixture(scope='module')
def refs():
    memo = {}

    def get(S, beta):
        if (S, beta) not in memo:
            c = cc.edge_case(S, beta, cc.case_seed(S, beta))
            memo[(S, beta)] = (c, cc.reference(c, torch.float32), cc.reference(c, torch.float64))
        return memo[(S, beta)]
    return get


def test_transmittance_weights_with_one_sample():
    """The reference builds the 1e10 column per ray (network.py:631), so one sample per ray gives w = 1 - exp(-1e10 sigma)
    with T = 1; the oracle used to copy the column's shape from an empty slice and returned [N, 0]."""
    z = torch.tensor([[0.5], [1.5], [2.5]], dtype=torch.float64)
    dens = torch.tensor([[0.0], [3e-11], [7.0]], dtype=torch.float64)
    w, trans, dists = mo.transmittance_weights(z, dens)
    assert w.shape == trans.shape == dists.shape == (3, 1)
    assert torch.equal(dists, torch.full((3, 1), 1e10, dtype=torch.float64))
    assert torch.equal(trans, torch.ones(3, 1, dtype=torch.float64))
    assert torch.equal(w, 1 - torch.exp(-1e10 * dens))
    assert w[0, 0] == 0 and 0 < w[1, 0] < 1 and w[2, 0] == 1
    # and S = 2 is what it was: one interval, then 1e10
    w2, trans2, dists2 = mo.transmittance_weights(torch.tensor([[0.5, 0.75]], dtype=torch.float64),
                                                  torch.tensor([[2.0, 0.0]], dtype=torch.float64))
    assert torch.equal(dists2, torch.tensor([[0.25, 1e10]], dtype=torch.float64))
    assert torch.equal(trans2, torch.exp(-torch.tensor([[0.0, 0.5]], dtype=torch.float64)))
    assert torch.equal(w2, torch.stack([1 - torch.exp(torch.tensor(-0.5, dtype=torch.float64)),
                                        torch.tensor(0.0, dtype=torch.float64)])[None])


@pytest.mark.parametrize('S,beta', CASES)
def test_fp32_oracle_within_a_tenth_of_the_bar(S, beta, refs):
    _, r32, r64 = refs(S, beta)
    for k, v in _deviation(r32, r64).items():
        assert v <= 1e-5, (S, beta, k, v)
    # d/d beta is no cancelled sum (edge_case aligns the signs of its terms)
    c = refs(S, beta)[0]
    parts = cc.beta_partials(c)
    assert (parts >= 0).all() and abs(parts.sum().item() - r64[1]['d/d beta'].item()) <= 1e-9 * parts.sum().item() + 1e-300


def _deviation(r32, r64):
    """fp32 oracle against float64 oracle: per-sample tensors per chunk, per-ray outputs and d/d beta whole."""
    (o32, g32), (o64, g64) = r32, r64
    dev = {k: cc.chunk_rel_err(o32[k] if k in o32 else g32[k], o64[k] if k in o64 else g64[k]) for k in PER_SAMPLE}
    dev.update({k: rel_err(o32[k], o64[k]) for k in ('rgb_values', 'depth', 'normal_map')})
    dev['d/d beta'] = rel_err(g32['d/d beta'], g64['d/d beta'])
    return dev


@pytest.mark.parametrize('S,beta', CASES)
def test_autograd_of_the_oracle_is_the_derivative(S, beta, refs):
    c, _, r64 = refs(S, beta)
    for k, v in _deviation(r64, cc.reference(c, torch.float64, density=cc.density_smooth)).items():
        assert v <= 1e-5, (S, beta, k, v)


def test_why_the_exact_zeros_and_the_80_beta_escape_are_not_parity_cases():
    """The two artefacts of the reference's autograd that the condition above exists for, so that nobody puts them
    back: an exact zero fails it by hundreds of bars (6e-2), an escape at 80 beta with one sample by 1e-3 -- and the oracle at +-1e-30,
    the reference the GPU test uses for exact zeros, is the derivative from either side."""
    c = cc.edge_case(65, 0.07, cc.case_seed(65, 0.07))
    smooth = cc.reference(cc.with_zero_crossings(c), torch.float64, density=cc.density_smooth)
    dev = _deviation(cc.reference(cc.with_zero_crossings(c), torch.float64), smooth)
    assert dev['d/d sdf'] > 1e-2 and max(v for k, v in dev.items() if k not in ('d/d sdf', 'd/d beta')) <= 1e-9
    for tiny in (1e-30, -1e-30):
        side = _deviation(cc.reference(cc.with_zero_crossings(c, tiny), torch.float64), smooth)
        assert max(side.values()) <= 1e-9, (tiny, side)
    try:
        cc.ESCAPE = 80.0
        c1 = cc.edge_case(1, 0.07, cc.case_seed(1, 0.07))
    finally:
        cc.ESCAPE = 100.0
    dev = _deviation(cc.reference(c1, torch.float64), cc.reference(c1, torch.float64, density=cc.density_smooth))
    assert 1e-3 < dev['d/d sdf'] < 1e-1 and not cc.reference(c1, torch.float64)[1]['d/d sdf'].any()


def _both(c, **kw):
    return _deviation(cc.reference(c, torch.float32, **kw), cc.reference(c, torch.float64, **kw))


@pytest.mark.parametrize('name', sorted(cc.OPTIONS))
@pytest.mark.parametrize('S', cc.OPTION_SAMPLES)
def test_fp32_oracle_within_a_tenth_of_the_bar_with_options(S, name, refs):
    """The same for the option runs: white background, poses, losses of one output (their unused gradients are exact
    zeros on both sides)."""
    white, n_poses, use = cc.OPTIONS[name]
    c = refs(S, 0.07)[0]
    for k, v in _both(c, white=white, pose=cc.option_pose(c, n_poses), use=use).items():
        assert v <= 1e-5, (S, name, k, v)


def test_fp32_oracle_within_a_tenth_of_the_bar_many_rays_beta_raw(refs):
    """N = 130 at S = 3 with beta = |beta_raw| + beta_min (the GPU test's msdf_beta_grad case), and the ray counts
    cut from the S = 65 case."""
    c = cc.edge_case(*cc.BETA_RAW_CASE)
    assert c['z'].shape == (130, 3)
    for k, v in _both(c, beta_raw=cc.BETA_RAW, beta_min=cc.BETA_MIN).items():
        assert v <= 1e-5, (k, v)
    for n in cc.RAY_COUNTS:
        for k, v in _both(cc.take(refs(65, 0.07)[0], n)).items():
            assert v <= 1e-5, (n, k, v)


@pytest.mark.parametrize('S,beta', CASES)
def test_every_chunk_carries_weight(S, beta, refs):
    _, _, (o64, g64) = refs(S, beta)
    w = o64['weights']
    for lo in range(0, S, 64):
        assert w[:, lo:lo + 64].max().item() >= 1e-3, (S, beta, lo, w[:, lo:lo + 64].max().item())
    # the escaping rays leave mass for the background; the crossing rays do not
    wsum = w.sum(1)
    assert (wsum[-2:] < 1 - 1e-4).all() and (wsum[:-2] > 1 - 1e-9).all(), wsum


@pytest.mark.parametrize('S,beta', CASES)
def test_last_sample_rule_and_coverage(S, beta, refs):
    c = refs(S, beta)[0]
    last = c['sdf'][:, -1].double() / c['beta'].double()
    assert ((last <= 0) | (last <= 12) | (last >= 60)).all(), last
    assert (c['sdf'].double().abs() / c['beta'].double() <= 3.0 + 1e-6)[:, :-1].all()
    ks = c['crossings']
    assert set(ks) == {k for k in cc.CROSSINGS if k < S} | {k for k in (S - 2, S - 1) if k >= 0}
    assert c['z'].shape[0] == len(ks) + 2
    for r, k in enumerate(ks):
        s = c['sdf'][r]
        assert (s[:k] > 0).all() and (s[k:] <= 0).all(), (S, beta, r, k)
    assert (c['sdf'][-2:] > 0).all() and (c['sdf'][-2:, -1] == cc.ESCAPE * c['beta']).all()
    assert (c['sdf'] == 0).sum() == 0 and (c['nrm'].abs().sum(-1) == 0).sum() == 1
    assert (c['z'][:, 1:] >= c['z'][:, :-1]).all()


def test_chunk_rel_err_sees_what_rel_err_hides():
    """An error of 1e-3 of a late chunk's own scale, in a tensor whose first chunk is 1e4 times larger."""
    b = torch.ones(3, 130)
    b[:, 64:] = 1e-4
    a = b.clone()
    a[1, 129] += 1e-7
    assert rel_err(a, b) < 2e-7 and abs(cc.chunk_rel_err(a, b) - 1e-3) < 1e-5
    assert cc.chunk_rel_err(b, b) == 0.0
    assert abs(cc.chunk_rel_err(torch.ones(2, 5, 3), torch.ones(2, 5, 3) * 2) - 0.5) < 1e-9
