"""The weight-norm kernels (csrc/weightnorm.hip) on their own: one table that mixes layers of 1 ... 257 columns and 1 ... 5
rows, with and without weight norm in turn, against float64 g v / ||v|| and its float64 autograd.  One wave handles one
row and four rows share a workgroup: the table has 26 rows (no multiple of 4) and all but two of its layer boundaries
fall inside a workgroup.  Layers without weight norm pass v through: dv = dw, their dg rows are 0.

The bar is derived, not measured: a row's dot product takes ceil(cols / 64) serial adds per lane, 6 butterfly adds and
about 3 further roundings, so 2 (ceil(cols / 64) + 9) 2^-24 -- of the reference value for the norms and the effective
weights, of sum |dw_i v_i| / ||v|| for dg and dv.  (dv = (g / n) dw - (g <dw, v> / n^3) v inherits the dot product's
error times |g v_c| / n^2: the rows here have |g| <= 1 <= ||v||, so that the same bar bounds it.)
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 1234.5
# (rows, cols, has_g): every column count with and without weight norm somewhere, layer starts at rows 0 2 3 8 10 11 16 18
# 23 25 -- inside a four-row workgroup but for 8 and 16
SHAPES = ((2, 1, True), (1, 3, False), (5, 63, True), (2, 64, False), (1, 65, True), (5, 257, False), (2, 257, True),
          (5, 65, False), (2, 3, True), (1, 1, False))
ORTHOGONAL = (2, 0)          # (layer, row): dw orthogonal to v, dg = 0
NEGATIVE_G = (6, 1)          # (layer, row): g < 0


def bar(cols):
    return 2.0 * (math.ceil(cols / 64) + 9) * 2.0 ** -24


def make_table(seed=0):
    """Per layer the fp32 parameters v [rows, cols] (1 <= ||v|| <= 2 per row), g [rows, 1] (0.5 <= |g| <= 1) or None,
    b [rows], and the cotangents dw, db."""
    gen = torch.Generator().manual_seed(seed)
    layers = []
    for i, (rows, cols, has_g) in enumerate(SHAPES):
        v = torch.randn(rows, cols, generator=gen)
        v = v * ((1.0 + torch.rand(rows, 1, generator=gen)) / v.norm(dim=1, keepdim=True))
        g = (0.5 + 0.5 * torch.rand(rows, 1, generator=gen)) if has_g else None
        dw = torch.randn(rows, cols, generator=gen)
        if i == NEGATIVE_G[0]:
            g[NEGATIVE_G[1]] = -g[NEGATIVE_G[1]]
        if i == ORTHOGONAL[0]:
            r = ORTHOGONAL[1]
            v64, d64 = v[r].double(), dw[r].double()
            dw[r] = (d64 - (d64 @ v64) / (v64 @ v64) * v64).float()
        layers.append({'v': v, 'g': g, 'b': torch.randn(rows, generator=gen), 'dw': dw,
                       'db': torch.randn(rows, generator=gen)})
    return layers


def reference(layers):
    """float64: per layer w, the row norms, dv, dg (zeros without weight norm) and the dot scale sum |dw v| / n."""
    out = []
    for l in layers:
        v = l['v'].double().requires_grad_(True)
        dw = l['dw'].double()
        n = v.detach().norm(dim=1, keepdim=True)
        if l['g'] is None:
            w, dv, dg = v.detach(), dw, torch.zeros(v.shape[0], 1, dtype=torch.float64)
        else:
            g = l['g'].double().requires_grad_(True)
            w = g * v / v.norm(dim=1, keepdim=True)
            dv, dg = torch.autograd.grad((dw * w).sum(), [v, g])
            w = w.detach()
        out.append({'w': w, 'n': n, 'dv': dv, 'dg': dg, 'scale': (dw * v.detach()).abs().sum(1, keepdim=True) / n})
    return out


def _compare(errlog, name, layers, ref, flat_w, norms, dv, dg):
    """Per row against the derived bar; flat tensors on the CPU.  norms / flat_w None: the backward alone."""
    w_off = row = 0
    worst = {}
    for i, ((rows, cols, has_g), l, r) in enumerate(zip(SHAPES, layers, ref)):
        n_el = rows * cols
        sl, rs = slice(w_off, w_off + n_el), slice(row, row + rows)
        tol = bar(cols)
        errs = {}
        if flat_w is not None:
            w = flat_w[sl].view(rows, cols).double()
            if has_g and norms is not None:
                errs['norms'] = ((norms[rs].double().view(rows, 1) - r['n']).abs() / r['n']).max().item()
            if has_g:
                errs['flat_w'] = ((w - r['w']).abs() / r['w'].abs().clamp(min=1e-300)).max().item()
            else:
                assert torch.equal(flat_w[sl].view(rows, cols), l['v']), (name, i)
        if dv is not None:
            if has_g:
                errs['dv'] = ((dv[sl].view(rows, cols).double() - r['dv']).abs() / r['scale']).max().item()
                errs['dg'] = ((dg[rs].view(rows, 1).double() - r['dg']).abs() / r['scale']).max().item()
            else:
                assert torch.equal(dv[sl].view(rows, cols), l['dw']), (name, i)
                assert bool((dg[rs] == 0).all()), (name, i)
        for k, e in errs.items():
            worst[k] = max(worst.get(k, 0.0), e / tol)
            errlog('weightnorm', name, 'layer%d %dx%d %s' % (i, rows, cols, k), e, tol)
            assert e <= tol, (name, i, (rows, cols), k, e, tol)
        w_off += n_el
        row += rows
    return worst


def test_forward_and_backward_kernels_on_a_mixed_table(errlog):
    from monosdf_amd import _lib, ops
    layers = make_table()
    ref = reference(layers)
    dev = 'cuda'
    tensors, shapes = [], []
    for (rows, cols, has_g), l in zip(SHAPES, layers):
        tensors += [l[k].to(dev).contiguous() for k in (('v', 'g', 'b') if has_g else ('v', 'b'))]
        shapes.append((rows, cols, has_g))
    tab = ops.WeightNormTables(shapes, tensors)
    n_w, total = tab.n_w, tab.total_rows
    assert total == sum(s[0] for s in SHAPES) == 26 and total % 4 != 0
    assert n_w == sum(s[0] * s[1] for s in SHAPES)
    guard = 257                                           # a guard row after the last layer
    flat_w = torch.full((n_w + guard,), SENTINEL, device=dev)
    flat_b, norms = torch.full((total + 1,), SENTINEL, device=dev), torch.full((total + 1,), SENTINEL, device=dev)
    P, st = _lib.ptr, _lib.stream_ptr()
    _lib.call('msdf_weightnorm_forward', P(tab.layers_dev), P(tab.row_layer_dev), total, P(flat_w), P(flat_b), P(norms), st)
    g_w = torch.cat([l['dw'].reshape(-1) for l in layers]).to(dev).contiguous()
    dv = torch.full((n_w + guard,), SENTINEL, device=dev)
    dg = torch.full((total + 1,), SENTINEL, device=dev)
    # the backward reads the norms the forward left; the rows without weight norm hold the sentinel and are not read
    _lib.call('msdf_weightnorm_backward', P(tab.layers_dev), P(tab.row_layer_dev), total, P(g_w), P(norms), P(dv), P(dg), st)
    torch.cuda.synchronize()
    flat_w, flat_b, norms, dv, dg = [t.cpu() for t in (flat_w, flat_b, norms, dv, dg)]
    assert torch.equal(flat_b[:total], torch.cat([l['b'] for l in layers]))
    for t, n in ((flat_w, n_w), (dv, n_w), (flat_b, total), (norms, total), (dg, total)):
        assert bool((t[n:] == SENTINEL).all())
    has_g_rows = torch.cat([torch.full((s[0],), s[2]) for s in SHAPES])
    assert bool((norms[:total][~has_g_rows] == SENTINEL).all())
    _compare(errlog, 'kernels', layers, ref, flat_w, norms, dv, dg)
    # the two special rows are what they claim to be
    row0 = sum(s[0] for s in SHAPES[:ORTHOGONAL[0]]) + ORTHOGONAL[1]
    assert abs(float(ref[ORTHOGONAL[0]]['dg'][ORTHOGONAL[1]])) <= 1e-7 * float(ref[ORTHOGONAL[0]]['scale'][ORTHOGONAL[1]])
    assert abs(float(dg[row0])) <= bar(SHAPES[ORTHOGONAL[0]][1]) * float(ref[ORTHOGONAL[0]]['scale'][ORTHOGONAL[1]])
    assert float(layers[NEGATIVE_G[0]]['g'][NEGATIVE_G[1]]) < 0


class _Layer:
    """What ops.fused_weight_norm reads of a layer."""

    def __init__(self, l, dev):
        leaf = lambda t: t.to(dev).contiguous().requires_grad_(True)
        self.out_features, self.in_features = l['v'].shape
        self.has_weight_norm = l['g'] is not None
        if self.has_weight_norm:
            self.weight_v, self.weight_g = leaf(l['v']), leaf(l['g'])
        else:
            self.weight = leaf(l['v'])
        self.bias = leaf(l['b'])


def test_fused_weight_norm_through_autograd(errlog):
    """ops.fused_weight_norm over stand-in layers: the flat outputs, and the gradients autograd hands to each parameter
    (a layer without weight norm has no g: the list of gradients is one shorter there)."""
    from monosdf_amd import ops
    layers = make_table(seed=1)
    ref = reference(layers)
    mods = [_Layer(l, 'cuda') for l in layers]
    flat_w, flat_b = ops.fused_weight_norm(ops.WeightNormState(), mods)
    g_w = torch.cat([l['dw'].reshape(-1) for l in layers]).cuda()
    g_b = torch.cat([l['db'] for l in layers]).cuda()
    ((flat_w * g_w).sum() + (flat_b * g_b).sum()).backward()
    assert torch.equal(flat_b.detach().cpu(), torch.cat([l['b'] for l in layers]))
    dv = torch.cat([(m.weight_v if m.has_weight_norm else m.weight).grad.reshape(-1) for m in mods]).cpu()
    dg = torch.cat([m.weight_g.grad.reshape(-1) if m.has_weight_norm else torch.zeros(m.out_features, device='cuda')
                    for m in mods]).cpu()
    for m, l in zip(mods, layers):
        assert torch.equal(m.bias.grad.cpu(), l['db'])
        assert (m.weight_v if m.has_weight_norm else m.weight).grad.shape == l['v'].shape
        assert not m.has_weight_norm or m.weight_g.grad.shape == l['g'].shape
    _compare(errlog, 'autograd', layers, ref, flat_w.detach().cpu(), None, dv, dg)
