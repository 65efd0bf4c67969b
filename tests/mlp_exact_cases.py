"""Inputs on which the fused MLP kernels (csrc/mlp_core.h, mlp_core_b16.h, sdf_kernels.h, color_kernels.h) are exactly
computable in fp32, on the CPU only.

Both networks are built as integer ReLU networks:

  colour   if_hdr (ReLU output, backward mask y > 0), multires_view = 0, no weight norm: affine maps and ReLUs only
  SDF      multires = 0, no weight norm (SDF_CASES: no skip, no sphere clamp); hidden weights multiples of 4, hidden
           biases = 2 (mod 4), integer inputs: every hidden pre-activation is an integer = 2 (mod 4), so |a| >= 2 and softplus(beta = 100) IS
           ReLU (common.h: softplus100 returns a for a >= 2 and fma(0.01, 0, 0) = 0 for a <= -2; the sigmoid factor of the
           sweeps is exactly 0 or 1 and the second-order term exactly 0)
  skip     the same with skip_in = (l,): layer l reads [h | x] / sqrt(2).  The kernels fold s32 = float32(1 / sqrt(2))
           into the packed weights, float32(s32 * W); the stored weights are the fp32 values v with float32(s32 * v) = 4
           and = 8 exactly (skip_magnitudes()), so the layer is an integer layer for the kernels.  The gradient of the
           stored weights is float32(s32) * float32(G), G the exact integer gradient of the effective ones
  clamp    the same with the bounding-sphere clamp: integer points, dyadic radius and scale; sqrt, subtract, divide and
           multiply restated in numpy fp32, one rounding per operation (clamp_restatement()), no decision near a tie
  group    the clamp case under evaluate(x, n_clamp, n_feat, split): all choices compute the same exact integers
  grid     the same SDF network behind a hash grid of levels of scale 8, points on multiples of 1/8, integer tables,
           first-layer weights multiples of 32: features, Jacobian and chain factor are dyadic numbers.  The geometry
           (num_levels, level_dim, logmap) belongs to the case (case.args, grid_conf()): between them the cases take
           every piece of the SDF kernels' level-major loads and every path a grid model can run (grid_structure())

A float64 evaluation of such a network is the exact answer, and every fp32 result -- whatever the summation order, on the
fp32 matrix instructions or as bf16 plane products accumulated in fp32 -- is bit-equal to it as long as every term of a
sum is a multiple of one granule g and the sum of the terms' magnitudes stays below 2^24 g.  On the bf16 cores an operand
is split into planes (round to nearest even, b16_split) and only some plane products are formed (b16_step):

  bf16x3   2 planes   pairs (i, j) with i + j <= 3
  bf16x6   3 planes   pairs (i, j) with i + j <= 4

so a product is exact there if every pair of non-zero planes it needs is among the kept ones.

reference()    the float64 restatement of a case, every output (autograd), independent of oracle/monosdf_oracle.py (the
               hash-grid arithmetic alone comes from oracle/hashgrid_oracle.py, its only statement)
products()     the same pass product by product, as the kernels form it, with the float64 operands of each product
certificate()  the conditions above, checked on those operands (and on the hash grid's own sums, other_sums()): a GPU
               test asserts it before it looks at a GPU result
emulate()      a product as a core forms it: planes, kept pairs, fp32 accumulation in a shuffled order
structure()    which gemm_tiles / gemm_b16 specialisation each product takes, from the plans of monosdf_amd/plan.py
grid_structure()  hash-grid cases: the pieces of aux_load_tile / aux_store_tile (sdf_kernels.h) a case takes and which of
               the five paths of a grid model a (core, flags) pair runs it on
"""
import collections
import math

import numpy as np
import torch

from monosdf_amd import plan as planlib
from oracle import hashgrid_oracle as hg

CORES = ('fp32', 'bf16x3', 'bf16x6')
PLANES = {'bf16x3': 2, 'bf16x6': 3}
# b16_step (mlp_core_b16.h): (plane of the weight fragment, plane of the activation), 1-based, in its order
KEPT = {2: ((1, 1), (1, 2), (2, 1)),
        3: ((1, 1), (1, 2), (2, 1), (1, 3), (2, 2), (3, 1))}
SUM_BOUND = 2.0 ** 24
MT = planlib.MT                      # 17 tiles
# an integer with exactly 1 / 2 / 3 non-zero bf16 planes (and so has k times it, k = 1, 2, 3): 257 = 256 + 1;
# 131329 = 2^17 + 2^8 + 1 -> 131072, 256 (the tie 257 goes to even), 1
PLANE_UNIT = {1: 1.0, 2: 257.0, 3: 131329.0}

Case = collections.namedtuple('Case', 'name kind args state inputs up')
# role: 'forward' | 'transposed' | 'wgrad' | 'dot';  unit: who forms it -- 'core' (the matrix core of the precision),
# 'wgrad' (msdf_wgrad_k: fp32 for fp32 and bf16x6; msdf_wgrad_b16_k, two planes, for bf16x3), 'dot' (plain fp32)
# A [m, k], B [k, n], adds: tensors broadcastable to [m, n] that the sum starts from or ends with (bias, the
# accumulators of the product before);  key: (pack unit, 'f' | 't') of the plan, None where no matrix core runs
Product = collections.namedtuple('Product', 'name role unit A B adds key')


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _memo(cache, case, fn):
    """fn(case), computed once per Case (or Product) object: keyed by identity, kept alive by the entry."""
    ent = cache.get(id(case))
    if ent is None or ent[0] is not case:
        ent = cache[id(case)] = (case, fn(case))
    return ent[1]


def _n_layers(case):
    return case.args['hidden'] + 1


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _sparse(g, rows, cols, nnz, values):
    """[rows, cols] with nnz non-zeros per row drawn from `values`."""
    W = torch.zeros(rows, cols)
    vals = torch.tensor(values, dtype=torch.float32)
    for r in range(rows):
        idx = torch.randperm(cols, generator=g)[:min(nnz, cols)]
        W[r, idx] = vals[torch.randint(len(vals), (len(idx),), generator=g)]
    return W


# ---------------------------------------------------------------------------
# case builders
# ---------------------------------------------------------------------------
def color_case(name, width=64, hidden=1, mode='idr', code=False, F=32, spr=1, P=64, seed=0, wp=1, fp=1, gp=1,
               in_max=2):
    """RenderingNetwork(F, mode, ..., dims = [width] * hidden, weight_norm = False, multires_view = 0, if_hdr = True).
    wp / fp / gp: planes of the first layer's feature weights / of the features / of the upstream gradient (probes)."""
    g = _gen(seed)
    lead = 9 if mode == 'idr' else 3
    n_rays = P // spr
    assert n_rays * spr == P
    in0 = lead + F + (32 if code else 0)
    state = {}
    W0 = torch.zeros(width, in0)
    W0[:, :lead] = _sparse(g, width, lead, 1, (-2, -1, 1, 2))
    W0[:, lead:lead + F] = _sparse(g, width, F, 2, (-1, 1)) * PLANE_UNIT[wp]
    if code:
        W0[:, lead + F:] = _sparse(g, width, 32, 1, (-1, 1))
    state['lin0.weight'], state['lin0.bias'] = W0, _ints(g, (width,), -2, 2)
    for l in range(1, hidden):
        state['lin%d.weight' % l], state['lin%d.bias' % l] = _sparse(g, width, width, 3, (-1, 1)), _ints(g, (width,), -2, 2)
    state['lin%d.weight' % hidden] = _sparse(g, 3, width, 2 if max(wp, fp, gp) > 1 else 6, (-1, 1))
    state['lin%d.bias' % hidden] = _ints(g, (3,), -1, 1)
    if code:
        state['embeddings'] = _ints(g, (1024, 32), -1, 1)
    inputs = dict(points=_ints(g, (P, 3), -in_max, in_max), normals=_ints(g, (P, 3), -in_max, in_max),
                  dirs=_ints(g, (n_rays, 3), -in_max, in_max), feat=_ints(g, (P, F), -in_max, in_max) * PLANE_UNIT[fp],
                  indices=(torch.arange(n_rays) * 3) % 11)
    up = dict(g_rgb=_ints(g, (P, 3), -in_max, in_max) * PLANE_UNIT[gp])
    args = dict(width=width, hidden=hidden, mode=mode, code=code, F=F, spr=spr, P=P)
    return Case(name, 'color', args, state, inputs, up)


HIDDEN_BIAS = (-6, -2, 2, 6)


def skip_scale(shapes, skip_in, F):
    """The factor of a skip layer as the kernels hold it: msdf_packrule_t.scale of the plan (plan.py: 1 / sqrt(2)).  The
    rule's field is a C float, which reads back as a Python float holding that fp32 value: s32 = float32(1 / sqrt(2))."""
    mp = planlib.build_sdf_plan(list(shapes), tuple(skip_in), 0, 0, False, F)
    s = {float(mp.rules[l].scale) for l in skip_in}
    assert len(s) == 1
    s32 = s.pop()
    assert isinstance(s32, float) and float(np.float32(s32)) == s32 == float(np.float32(1.0 / math.sqrt(2.0)))
    return s32


def skip_magnitudes(s32):
    """The stored fp32 magnitudes v4, v8 with float32(s32 * v) exactly 4 and exactly 8: searched among the fp32
    neighbours of 4 sqrt(2) and 8 sqrt(2), nearest first (none exists for 3 or 12)."""
    s, out = np.float32(s32), []
    for k in (4.0, 8.0):
        v = np.float32(k * math.sqrt(2.0))
        lo = hi = v
        cands = [v]
        for _ in range(8):
            lo, hi = np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(np.inf))
            cands += [lo, hi]
        hits = [c for c in cands if np.float32(s * c) == np.float32(k)]
        assert hits, k
        assert float(np.float32(s * hits[0])) == k
        out.append(float(hits[0]))
    return tuple(out)


# points of the clamp cases, in front of the random ones: the origin; axis points (power-of-two norm: exact under any
# sqrt); integer norms 3, 7 and 5 with permutations and signs
SPECIAL_POINTS = ((0, 0, 0), (1, 0, 0), (0, -2, 0), (0, 0, 4), (1, 2, 2), (-2, 1, 2), (2, -2, -1), (2, 3, 6), (-6, 2, 3),
                  (0, 3, 4), (4, 0, -3), (-3, -4, 0))
CLAMP_MARGIN = 2.0 ** -10


def _sdf_build(name, g, width, hidden, F, P, skip_in, radius, sphere_scale, n_clamp, n_feat, split):
    bias = torch.tensor(HIDDEN_BIAS, dtype=torch.float32)
    state = {}
    outs = [width - 3 if (l + 1) in skip_in else width for l in range(hidden)]
    shapes = [(outs[l], 3 if l == 0 else width) for l in range(hidden)] + [(1 + F, width)]
    if skip_in:
        assert all(0 < l < hidden for l in skip_in)
        v4, v8 = skip_magnitudes(skip_scale(shapes, skip_in, F))
    for l in range(hidden):
        rows, cols = shapes[l]
        if l in skip_in:
            # [h | x]: +-v4, +-v8, for the kernels the integers +-4, +-8; two non-zeros per row in h, one in x
            vals = (-v8, -v4, v4, v8)
            state['lin%d.weight' % l] = torch.cat([_sparse(g, rows, cols - 3, 2, vals), _sparse(g, rows, 3, 1, vals)], 1)
        else:
            state['lin%d.weight' % l] = _sparse(g, rows, cols, 2, (-4, 4))
        state['lin%d.bias' % l] = bias[torch.randint(4, (rows,), generator=g)]
    state['lin%d.weight' % hidden] = _sparse(g, 1 + F, width, 4, (-2, -1, 1, 2))
    state['lin%d.bias' % hidden] = _ints(g, (1 + F,), -2, 2)
    x = _ints(g, (P, 3), -3, 3)
    if radius > 0:
        ns = len(SPECIAL_POINTS)
        assert P > ns
        x[:ns] = torch.tensor(SPECIAL_POINTS, dtype=torch.float32)
        x[P - 1] = 0                          # the origin again, in the ragged last workgroup
    up = dict(a=_ints(g, (P, 1), -2, 2), B=_ints(g, (P, F), -2, 2), C=_ints(g, (P, 3), -2, 2))
    if split is not None:
        # the node's backward receives two tensors per output; evaluate() does not return sdf [split:], so no gradient
        # of it exists: the second of the pair is None.  B stays [P, F]: the loss uses its first n_feat rows
        up = dict(a=(up['a'][:split], None), B=up['B'], C=(up['C'][:split], up['C'][split:]))
    args = dict(width=width, hidden=hidden, F=F, P=P)
    if skip_in or radius > 0 or split is not None or n_clamp is not None or n_feat is not None:
        args.update(skip_in=tuple(skip_in), radius=float(radius), sphere_scale=float(sphere_scale), n_clamp=n_clamp,
                    n_feat=n_feat, split=split)
    return Case(name, 'sdf', args, state, dict(x=x), up)


def sdf_case(name, width=64, hidden=2, F=16, P=64, seed=0, skip_in=(), radius=0.0, sphere_scale=1.0, n_clamp=None,
             n_feat=None, split=None):
    """ImplicitNetwork(F, radius, 3, 1, [width] * hidden, geometric_init = False, skip_in, weight_norm = False,
    multires = 0, sphere_scale): radius = sdf_bounding_sphere = 0 switches the clamp off.
    skip_in = (l,): layer l - 1 has width - 3 outputs, layer l reads [h | x] / sqrt(2) -- its stored weights are the fp32
    values that the folded factor turns into +-4 and +-8 exactly (skip_magnitudes()).
    radius, sphere_scale (dyadic): the points begin with SPECIAL_POINTS and end with the origin; the seed moves on
    (seed + 1009 k) until clamp_conditions() holds -- every kind of point present, no decision within CLAMP_MARGIN.
    n_clamp, n_feat, split: the arguments of evaluate() (None: P, P and no split, what get_outputs() passes); with a
    split, up['a'] and up['C'] are the pairs of tensors the node's backward receives."""
    skip_in = tuple(skip_in)
    for k in range(64 if radius > 0 or skip_in else 1):
        case = _sdf_build(name, _gen(seed + 1009 * k), width, hidden, F, P, skip_in, radius, sphere_scale, n_clamp,
                          n_feat, split)
        why = (clamp_conditions(case) if radius > 0 else []) + (skip_conditions(case) if skip_in else [])
        if not why:
            return case
    raise AssertionError('%s: no seed gives the case what it is there for: %r' % (name, why[:3]))


def skip_conditions(case):
    """Reasons why a skip case does NOT show its skip layer (empty: it does): d sdf / d input behind the skip layer's
    hidden tiles must be non-zero at half the points at least (a deep sparse ReLU network can be dead at most)."""
    whole, first = _sdf_products(case)[1]['grad'], _sdf_products(case, 'one_input_arrival')[1]['grad']
    alive = int((whole != first).any(1).sum())
    return [] if 2 * alive >= case.args['P'] else ['skip: the input gradient arrives behind the skip layer at %d points of %d'
                                                    % (alive, case.args['P'])]


def groups(case):
    """(n_clamp, n_feat, split) of the evaluation of this case: evaluate()'s arguments."""
    a = case.args
    P = a['P']
    nc, nf = a.get('n_clamp'), a.get('n_feat')
    return (P if nc is None else nc, P if nf is None else nf, a.get('split'))


def effective_weight(case, l):
    """float64 weights of layer l as the kernels multiply by them: float32(s32 * W) for a skip layer (the pack folds the
    factor in, one rounding), W itself otherwise."""
    W = case.state['lin%d.weight' % l]
    skip = case.args.get('skip_in', ())
    if l not in skip:
        return W.double()
    n = _n_layers(case)
    s32 = skip_scale([tuple(case.state['lin%d.weight' % i].shape) for i in range(n)], skip, case.args['F'])
    return (torch.tensor(s32, dtype=torch.float32) * W).double()


def scaled_gradient(case, G):
    """Gradient of the stored weights of a skip layer from the exact gradient G of the effective ones: msdf_reduce_k
    applies the factor to the finished sum, one rounding: float32(s32) * float32(G)."""
    n = _n_layers(case)
    s32 = skip_scale([tuple(case.state['lin%d.weight' % i].shape) for i in range(n)], case.args['skip_in'], case.args['F'])
    return (torch.tensor(s32, dtype=torch.float32) * G.float()).double()


Clamp = collections.namedtuple('Clamp', 'nx sph normals')
_CLAMP = {}


def clamp_restatement(case):
    """The clamp's fp32 arithmetic (sdf_kernels.h), one rounding per operation, in numpy: nx = sqrtf(x0 x0 + x1 x1 +
    x2 x2) (integers: the sum is exact however it is fused), sph = scale * (r - nx), inv = -scale / nx (0 at the
    origin, as torch's minimum gives that point a zero gradient), normals x_i * inv.  float64 tensors of fp32 values."""
    def run(case):
        a = case.args
        x = case.inputs['x'].numpy().astype(np.float32)
        r, sc = np.float32(a['radius']), np.float32(a['sphere_scale'])
        nx = np.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2])
        sph = sc * (r - nx)
        with np.errstate(divide='ignore'):
            inv = np.where(nx > 0, -sc / nx, np.float32(0))
        nrm = x * inv[:, None]
        assert nx.dtype == sph.dtype == nrm.dtype == np.float32
        t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).double()
        return Clamp(t(nx), t(sph), t(nrm))
    return _memo(_CLAMP, case, run)


def raw_sdf(case):
    """The unclamped sdf [P] of a case in float64 (forward chain only)."""
    n = _n_layers(case)
    x = case.inputs['x'].double()
    h = x
    for l in range(n - 1):
        if l in case.args.get('skip_in', ()):
            h = torch.cat([h, x], 1)
        h = torch.relu(h @ effective_weight(case, l).t() + case.state['lin%d.bias' % l].double())
    return h @ case.state['lin%d.weight' % (n - 1)].double()[0] + case.state['lin%d.bias' % (n - 1)].double()[0]


def clamp_categories(case):
    """Boolean masks [P] of the kinds of point a clamp case must hold; `would` = sph < sdf, whatever n_clamp says."""
    c = clamp_restatement(case)
    sdf = raw_sdf(case)
    inside = c.nx < case.args['radius']
    would = c.sph < sdf
    x = case.inputs['x']
    axis = (x != 0).sum(1) == 1
    return collections.OrderedDict([
        ('inside_unclamped', inside & ~would), ('inside_clamped', inside & would), ('outside_clamped', ~inside & would),
        ('outside_unclamped', ~inside & ~would & (c.sph < 0)), ('integer_norm', (c.nx == c.nx.round()) & (c.nx > 0) & ~axis),
        ('power_of_two_norm', axis & (torch.frexp(c.nx)[0] == 0.5)), ('origin', c.nx == 0), ('would', would)])


def clamp_conditions(case):
    """Reasons why a clamp case does NOT hold what it is there for (empty: it does).  No decision hangs on a rounding:
    |sdf - sph| >= CLAMP_MARGIN everywhere (the net's sdf is an integer, sph an fp32 value).  With n_clamp >= 64 every
    kind of point sits among the first n_clamp (the special points are the first twelve; the four kinds that depend on
    the network need some tens of random points to turn up); with 0 < n_clamp < 64 the special points do and both a
    clamped and an unclamped point; an origin among them is clamped.  With n_clamp < P a point beyond would be clamped."""
    n_clamp, _, _ = groups(case)
    P = case.args['P']
    c = clamp_restatement(case)
    sdf = raw_sdf(case)
    why = []
    if not torch.equal(sdf, sdf.round()):
        why.append('clamp: the sdf is no integer')
    if (sdf - c.sph).abs().min().item() < CLAMP_MARGIN:
        why.append('clamp: |sdf - sph| = %g' % (sdf - c.sph).abs().min().item())
    cat = clamp_categories(case)
    head = torch.arange(P) < n_clamp
    if not cat['inside_unclamped'].any() or not cat['outside_unclamped'].any():
        why.append('clamp: the network leaves no point unclamped')
    if n_clamp >= 64:
        need = [k for k in cat if k != 'would']
    elif n_clamp > 0:
        need = ['integer_norm', 'power_of_two_norm', 'origin']
        if not (head & cat['would']).any() or not (head & ~cat['would']).any():
            why.append('clamp: no clamped or no unclamped point among the first %d' % n_clamp)
    else:
        need = []
    for k in need:
        if not (head & cat[k]).any():
            why.append('clamp: no %s point among the first %d' % (k, n_clamp))
    if n_clamp > 0 and not (head & cat['origin'] & cat['would']).any():
        why.append('clamp: the origin is not clamped')
    if n_clamp < P and not (~head & ~(c.nx < case.args['radius']) & cat['would']).any():
        why.append('clamp: no outside point beyond n_clamp that would be clamped')
    return why


# Hash-grid model: levels of scale 8 (S = 0, resolution 9; dense tables of 729 entries, or hashed ones of 2^logmap
# where that is smaller), points at multiples of 1/8 so that x01 = k / 16 sits on a grid node or half-way between two
# (smoothstep 0, 1/2, 1: corner weights multiples of 1/8), integer tables, first-layer weights multiples of 32 --
# features, their Jacobian and the chain factor 0.5 are dyadic numbers and the first pre-activation stays an integer
# = 2 (mod 4).  What every grid case shares; num_levels, level_dim and logmap are in case.args
GRID_FIXED = dict(base_size=9, end_size=9, divide_factor=1.0)
# the geometry of the three first grid cases (grid_case's defaults): four dense levels of two features
GRID = dict(GRID_FIXED, num_levels=4, level_dim=2, logmap=19)


def grid_conf(case):
    """The hash-grid options of ImplicitNetworkGrid for this case (also what hg.level_geometry reads)."""
    a = case.args
    return dict(GRID_FIXED, num_levels=a['num_levels'], level_dim=a['level_dim'], logmap=a['logmap'])


def grid_case(name, width=64, hidden=2, F=16, P=64, seed=0, num_levels=GRID['num_levels'], level_dim=GRID['level_dim'],
              logmap=GRID['logmap']):
    """ImplicitNetworkGrid(F, 0.0, 3, 1, [width] * hidden, geometric_init = False, skip_in = (), weight_norm = False,
    multires = 0, **grid_conf(case)).  level_dim = 1 has no second-order term (neither has the reference: no C = 1
    second backward): its upstream gradient of d sdf / d x is zero and args['second_order'] False."""
    g = _gen(seed)
    args = dict(width=width, hidden=hidden, F=F, P=P, num_levels=num_levels, level_dim=level_dim, logmap=logmap,
                second_order=level_dim > 1)
    geo = hg.level_geometry(dict(GRID_FIXED, num_levels=num_levels, level_dim=level_dim, logmap=logmap))
    n_aux = num_levels * level_dim
    base = sdf_case(name, width, hidden, F, P, seed + 1000)
    state = dict(base.state)
    state['lin0.weight'] = torch.cat([_sparse(g, width, 3, 1, (-32, 32)), _sparse(g, width, n_aux, 2, (-32, 32))], 1)
    state['encoding.embeddings'] = _ints(g, (geo['n_entries'], level_dim), -2, 2)
    inputs = dict(x=_ints(g, (P, 3), -8, 8) / 8)
    up = base.up if level_dim > 1 else dict(base.up, C=torch.zeros_like(base.up['C']))
    return Case(name, 'grid', args, state, inputs, up)


def _cases(builder, specs):
    out = collections.OrderedDict()
    for i, (name, kw) in enumerate(specs):
        out[name] = builder(name, seed=100 + i, **kw)
    return out


# every P of {1, 15, 16, 17, 63, 64, 65, 213}; 7 samples per ray with P = 7 x 31 (rays end inside waves and workgroups)
COLOR_CASES = _cases(color_case, [
    ('w64_h1_idr_p213', dict(width=64, hidden=1, P=213)),
    ('w48_h2_idr_p65', dict(width=48, hidden=2, P=65)),
    ('w100_h2_idr_code_f40_p63', dict(width=100, hidden=2, code=True, F=40, P=63)),
    ('w176_h1_idr_p64', dict(width=176, hidden=1, P=64)),
    ('w176_h2_nerf_code_p17', dict(width=176, hidden=2, mode='nerf', code=True, P=17)),
    ('w256_h3_idr_f256_p16', dict(width=256, hidden=3, F=256, P=16)),
    ('w64_h3_nerf_p15', dict(width=64, hidden=3, mode='nerf', P=15)),
    ('w64_h2_idr_code_spr7_p217', dict(width=64, hidden=2, code=True, spr=7, P=217)),
    ('w64_h1_idr_p1', dict(width=64, hidden=1, P=1)),
    ('w64_h2_idr_big_p65', dict(width=64, hidden=2, P=65, in_max=300)),      # two-plane activations and gradients
])
SDF_CASES = _cases(sdf_case, [
    ('w64_h2_p213', dict(width=64, hidden=2, P=213)),
    ('w48_h3_f24_p65', dict(width=48, hidden=3, F=24, P=65)),
    ('w100_h2_p63', dict(width=100, hidden=2, P=63)),
    ('w256_h2_f256_p17', dict(width=256, hidden=2, F=256, P=17)),
    ('w64_h3_p1', dict(width=64, hidden=3, P=1)),
    ('w64_h2_p15', dict(width=64, hidden=2, P=15)),
    ('w48_h2_p16', dict(width=48, hidden=2, P=16)),
    ('w100_h3_p64', dict(width=100, hidden=3, P=64)),
])
# plane probes: one hidden layer, the first layer's feature product forward (weights x features) and transposed
# (weights^T x a-bar).  w<i>f<j>g<k>: planes of the weights, the features, the upstream gradient
PROBE_CASES = _cases(color_case, [
    ('w3f1g1', dict(wp=3, P=17, in_max=1)),
    ('w1f3g1', dict(fp=3, P=17, in_max=1)),
    ('w1f1g3', dict(gp=3, P=17, in_max=1)),
    ('w2f2g1', dict(wp=2, fp=2, P=17, in_max=1)),
    ('w2f1g2', dict(wp=2, gp=2, P=17, in_max=1)),
    ('w2f1g1', dict(wp=2, P=17, in_max=1)),
    ('w1f2g1', dict(fp=2, P=17, in_max=1)),
    ('w1f1g2', dict(gp=2, P=17, in_max=1)),
    # two hidden layers: the first hands two- and three-plane activations to a hidden product (bias and ReLU hooks), the
    # transposed hidden product gets a two- or three-plane a-bar
    ('h2_w1f3g1', dict(hidden=2, fp=3, P=17, in_max=1)),
    ('h2_w1f1g3', dict(hidden=2, gp=3, P=17, in_max=1)),
    ('h2_w1f2g1', dict(hidden=2, fp=2, P=17, in_max=1)),
    ('h2_w1f1g2', dict(hidden=2, gp=2, P=17, in_max=1)),
])
GRID_CASES = _cases(grid_case, [
    ('w64_h2_p213', dict(width=64, hidden=2, P=213)),
    ('w48_h3_p65', dict(width=48, hidden=3, P=65)),
    ('w64_h2_p17', dict(width=64, hidden=2, P=17)),
])
# every aux layout and every path: (level_dim, num_levels, logmap) at P = 17 and 65 (and the reference's own 16 x 2 at
# P = 213).  logmap 9: levels of 512 entries, hashed with a power-of-two size -- corners collide in the table gradient
GRID_LAYOUTS = [(2, 3, 19), (2, 5, 19), (2, 8, 19), (2, 9, 19), (2, 15, 19), (2, 16, 19), (2, 4, 9),
                (4, 3, 19), (4, 8, 19), (8, 2, 19), (8, 4, 19), (1, 5, 19)]


def grid_layout_name(level_dim, num_levels, logmap, P):
    return 'l%dc%d%s_p%d' % (num_levels, level_dim, '' if logmap == 19 else '_log%d' % logmap, P)


GRID_LAYOUT_CASES = collections.OrderedDict()
for _i, (_c, _l, _m) in enumerate(GRID_LAYOUTS):
    for _j, _p in enumerate((17, 65, 213) if (_c, _l) == (2, 16) else (17, 65)):
        _n = grid_layout_name(_c, _l, _m, _p)
        GRID_LAYOUT_CASES[_n] = grid_case(_n, width=64, hidden=2, P=_p, seed=200 + 3 * _i + _j, num_levels=_l,
                                          level_dim=_c, logmap=_m)
GRID_CASES.update(GRID_LAYOUT_CASES)
ALL_CASES = collections.OrderedDict()
for _group, _cs in (('color', COLOR_CASES), ('sdf', SDF_CASES), ('probe', PROBE_CASES), ('grid', GRID_CASES)):
    for _n, _c in _cs.items():
        ALL_CASES['%s.%s' % (_group, _n)] = _c


# ---------------------------------------------------------------------------
# float64 reference (autograd)
# ---------------------------------------------------------------------------
def _color_input(case, feat, nrm, emb):
    a, i = case.args, case.inputs
    ray = torch.arange(a['P']) // a['spr']
    v = i['dirs'].double()[ray]
    cols = [i['points'].double(), v, nrm] if a['mode'] == 'idr' else [v]
    cols.append(feat)
    if a['code']:
        cols.append(emb[i['indices']][ray])
    return torch.cat(cols, 1)


def _reference_color(case):
    st = {k: v.double().requires_grad_() for k, v in case.state.items()}
    feat = case.inputs['feat'].double().requires_grad_()
    nrm = case.inputs['normals'].double().requires_grad_()
    h = _color_input(case, feat, nrm, st.get('embeddings'))
    for l in range(_n_layers(case)):
        h = torch.relu(h @ st['lin%d.weight' % l].t() + st['lin%d.bias' % l])
    out = {'rgb': h.detach()}
    leaves = {'g_feat': feat}
    if case.args['mode'] == 'idr':
        leaves['g_nrm'] = nrm
    leaves.update({('g_code' if k == 'embeddings' else k): v for k, v in st.items()})
    grads = torch.autograd.grad((h * case.up['g_rgb'].double()).sum(), list(leaves.values()))
    out.update(dict(zip(leaves, grads)))
    return out


def _reference_sdf(case):
    st = {k: v.double().requires_grad_() for k, v in case.state.items()}
    x = case.inputs['x'].double().requires_grad_()
    n = _n_layers(case)
    h = x
    if case.kind == 'grid':
        conf = grid_conf(case)
        feat = hg.hash_encode_autograd(x / conf['divide_factor'], st['encoding.embeddings'], hg.level_geometry(conf))
        h = torch.cat([x, feat], 1)
    a = case.args
    skip = a.get('skip_in', ())
    # a skip layer multiplies by its effective weights (the gradient of the stored ones: scaled_gradient())
    eff = {l: effective_weight(case, l).requires_grad_() for l in skip}
    for l in range(n - 1):
        if l in skip:
            h = torch.cat([h, x], 1)
        h = torch.relu(h @ (eff[l] if l in skip else st['lin%d.weight' % l]).t() + st['lin%d.bias' % l])
    o = h @ st['lin%d.weight' % (n - 1)].t() + st['lin%d.bias' % (n - 1)]
    raw, feat = o[:, :1], o[:, 1:]
    n_clamp, n_feat, _ = groups(case)
    sdf = raw
    if a.get('radius', 0.0) > 0:
        sph = a['sphere_scale'] * (a['radius'] - x.norm(dim=1, keepdim=True))
        sdf = torch.where((torch.arange(a['P']) < n_clamp)[:, None], torch.minimum(raw, sph), raw)
    grad, = torch.autograd.grad(sdf.sum(), x, create_graph=True)
    ua, uB, uC = upstream(case)
    loss = (ua * sdf).sum() + (uB * feat).sum() + (uC * grad).sum()
    out = {'sdf': sdf.detach(), 'feat': feat.detach()[:n_feat], 'grad': grad.detach()}
    if a.get('radius', 0.0) > 0:
        # the clamped entries as the kernels' fp32 arithmetic gives them; forward() and gradient_sdf() do not clamp
        c = clamp_restatement(case)
        cl = (torch.arange(a['P']) < n_clamp) & (c.sph < raw.detach()[:, 0])
        out['sdf'] = torch.where(cl[:, None], c.sph[:, None], out['sdf'])
        out['grad'] = torch.where(cl[:, None], c.normals, out['grad'])
        out['sdf_raw'] = raw.detach()
        out['grad_raw'] = torch.autograd.grad(raw.sum(), x, retain_graph=True)[0]
    leaves = [eff[int(k[3:-7])] if k.endswith('.weight') and int(k[3:-7]) in skip else v for k, v in st.items()]
    for k, g in zip(st, torch.autograd.grad(loss, leaves)):
        out[k] = scaled_gradient(case, g) if k.endswith('.weight') and int(k[3:-7]) in skip else g
    return out


def upstream(case, mutate=None):
    """The upstream gradients of a case as float64 tensors over all P points: a [P, 1], B [P, F] with the rows from
    n_feat on zero, C [P, 3].  With a split, a and C are put together from the pairs of tensors the node's backward
    receives (no tensor: zeros).  mutate: what a wrong kernel would do ('feat_row_n_feat', 'second_tensor_at_pt')."""
    P = case.args['P']
    _, n_feat, split = groups(case)
    up = case.up
    if split is None:
        a, C = up['a'].double(), up['C'].double()
    else:
        a, C = torch.zeros(P, 1, dtype=torch.float64), torch.zeros(P, 3, dtype=torch.float64)
        for full, (first, second) in ((a, up['a']), (C, up['C'])):
            full[:split] = first.double()
            if second is None:
                continue
            if mutate == 'second_tensor_at_pt':
                # row p >= split reads row p of the second tensor instead of row p - split (past its end: nothing)
                m = second.shape[0]
                full[split:m] = second.double()[split:m]
            else:
                full[split:] = second.double()
    B = up['B'].double().clone()
    B[n_feat + (1 if mutate == 'feat_row_n_feat' else 0):] = 0
    return a, B, C


_REFERENCE = {}


def reference(case):
    """Every output of the case in float64, computed once: {'rgb', 'g_feat', 'g_nrm', 'g_code', parameter gradients} or
    {'sdf', 'feat', 'grad', parameter gradients of <a, sdf> + <B, feat> + <C, grad>}.  Treat as read-only."""
    return _memo(_REFERENCE, case, _reference_color if case.kind == 'color' else _reference_sdf)      # 'sdf', 'grid'


# ---------------------------------------------------------------------------
# the pass product by product, as the kernels form it
# ---------------------------------------------------------------------------
def _color_products(case):
    a = case.args
    n, hid = _n_layers(case), case.args['hidden']
    W = [case.state['lin%d.weight' % l].double() for l in range(n)]
    b = [case.state['lin%d.bias' % l].double()[:, None] for l in range(n)]
    P, F = a['P'], a['F']
    feat, nrm = case.inputs['feat'].double(), case.inputs['normals'].double()
    emb = case.state['embeddings'].double() if a['code'] else None
    full = _color_input(case, feat, nrm, emb)
    lead = 9 if a['mode'] == 'idr' else 3
    misc = torch.cat([full[:, :lead], full[:, lead + F:]], 1)
    W0f, W0m = W[0][:, lead:lead + F], torch.cat([W[0][:, :lead], W[0][:, lead + F:]], 1)
    pr = []
    acc0 = W0f @ feat.t() + b[0]
    pr.append(Product('u0.fwd', 'forward', 'core', W0f, feat.t(), (b[0],), (0, 'f')))
    pre = [acc0 + W0m @ misc.t()]
    pr.append(Product('u1.fwd', 'forward', 'core', W0m, misc.t(), (acc0,), (1, 'f')))
    h = [torch.relu(pre[0])]
    for l in range(1, hid):
        pr.append(Product('u%d.fwd' % (l + 1), 'forward', 'core', W[l], h[-1], (b[l],), (l + 1, 'f')))
        pre.append(W[l] @ h[-1] + b[l])
        h.append(torch.relu(pre[-1]))
    pr.append(Product('out.dot', 'dot', 'dot', W[hid], h[-1], (b[hid],), None))
    o = W[hid] @ h[-1] + b[hid]
    ab_out = case.up['g_rgb'].double().t() * (o > 0)
    pr.append(Product('out.dot_t', 'dot', 'dot', W[hid].t(), ab_out, (), None))
    ab = {hid - 1: (W[hid].t() @ ab_out) * (h[-1] > 0)}
    for l in range(hid - 1, 0, -1):
        pr.append(Product('u%d.bwd' % (l + 1), 'transposed', 'core', W[l].t(), ab[l], (), (l + 1, 't')))
        ab[l - 1] = (W[l].t() @ ab[l]) * (h[l - 1] > 0)
    pr.append(Product('u0.bwd', 'transposed', 'core', W0f.t(), ab[0], (), (0, 't')))
    pr.append(Product('u1.bwd', 'transposed', 'core', W0m.t(), ab[0], (), (1, 't')))
    g_misc = (W0m.t() @ ab[0]).t()
    ones = torch.ones(P, 1, dtype=torch.float64)
    pr.append(Product('u0.wgrad', 'wgrad', 'wgrad', ab[0], feat, (), None))
    pr.append(Product('u1.wgrad', 'wgrad', 'wgrad', ab[0], misc, (), None))
    for l in range(1, hid):
        pr.append(Product('u%d.wgrad' % (l + 1), 'wgrad', 'wgrad', ab[l], h[l - 1].t(), (), None))
    pr.append(Product('out.wgrad', 'wgrad', 'wgrad', ab_out, h[-1].t(), (), None))
    for l in range(hid):
        pr.append(Product('b%d.colsum' % l, 'dot', 'dot', ab[l], ones, (), None))
    pr.append(Product('b%d.colsum' % hid, 'dot', 'dot', ab_out, ones, (), None))
    # the outputs these products amount to (test_mlp_exact_cases_cpu.py compares them with reference())
    dW0m = ab[0] @ misc
    out = {'rgb': torch.relu(o).t(), 'g_feat': (W0f.t() @ ab[0]).t(),
           'lin0.weight': torch.cat([dW0m[:, :lead], ab[0] @ feat, dW0m[:, lead:]], 1)}
    if a['mode'] == 'idr':
        out['g_nrm'] = g_misc[:, 6:9]
    if a['code']:
        ray = torch.arange(P) // a['spr']
        out['g_code'] = torch.zeros(1024, 32, dtype=torch.float64).index_add_(0, case.inputs['indices'][ray],
                                                                            g_misc[:, lead:])
    for l in range(1, hid):
        out['lin%d.weight' % l] = ab[l] @ h[l - 1].t()
    out['lin%d.weight' % hid] = ab_out @ h[-1].t()
    for l in range(hid):
        out['lin%d.bias' % l] = ab[l].sum(1)
    out['lin%d.bias' % hid] = ab_out.sum(1)
    return pr, out, pre + [o]


def _grid_terms(case):
    """Hash-grid cases: x01, the features [n_aux, P] and the Jacobian J [P, L, 3, C] = d feature / d x01, in float64."""
    conf = grid_conf(case)
    geo = hg.level_geometry(conf)
    x01 = (case.inputs['x'].double() / conf['divide_factor'] + 1) / 2
    out, dy = hg.encode_forward(x01, case.state['encoding.embeddings'].double(), geo, True)
    P = x01.shape[0]
    return geo, x01, out.permute(1, 0, 2).reshape(P, -1).t(), dy.reshape(P, geo['L'], 3, geo['C'])


def _second_order_magnitude(r, x01, gg, geo, n_entries):
    """hg.second_backward_embedding with every term counted by its magnitude at both corners it goes to."""
    mag = torch.zeros(n_entries, geo['C'], dtype=torch.float64)
    off = geo['offsets']
    for l in range(geo['L']):
        scale, res, cell, sm, dsm = hg._locate(x01, geo, l)
        for gd in range(3):
            others = [d for d in range(3) if d != gd]
            for combo in range(4):
                w = torch.full((x01.shape[0],), scale, dtype=torch.float64)
                pos = cell.clone()
                for nd, d in enumerate(others):
                    on = bool(combo & (1 << nd))
                    w = w * (sm[:, d] if on else 1 - sm[:, d])
                    pos[:, d] += int(on)
                term = ((w * gg[:, gd] * dsm[:, gd]).unsqueeze(1) * r[l]).abs()
                for step in (0, 1):
                    pos[:, gd] += step
                    mag.index_add_(0, hg.grid_index(pos, off[l + 1] - off[l], res) + off[l], term)
    return mag


def _level_major(rows, geo):
    """[n_aux, P] (column l C + c of a point) -> the encoder's [L, P, C]."""
    return rows.t().reshape(-1, geo['L'], geo['C']).permute(1, 0, 2).contiguous()


# What a wrong kernel (or launcher) would do to the skip layer, the clamp or the point groups: _sdf_products(case, m)
# restates the pass with that mistake in it.  tests/test_mlp_exact_cases_cpu.py shows that each one changes an expected
# value of a certified case, i.e. that the exact comparison on the GPU would see it
MUTATIONS = ('one_input_arrival',           # d sdf / d input behind the skip layer's hidden tiles is not taken
             'no_input_columns',            # the skip layer's weight-gradient item without its input-block part
             'scale_twice', 'no_scale',     # 1 / sqrt(2) on the finished weight-gradient sum: twice, not at all
             'clamp_all',                   # points beyond n_clamp are clamped too
             'clamped_live',                # clamped points hand a and C on to the parameter gradients
             'no_feat_grad_when_clamped',   # ... or lose their feature gradient as well
             'feat_row_n_feat',             # row n_feat gets features (and their gradient)
             'second_tensor_at_pt')         # the second gradient tensor read at c.pt instead of c.pt - n_split


def _sdf_products(case, mutate=None):
    """ImplicitNetwork and ImplicitNetworkGrid.  Besides the products: `sums`, the other fp32 sums of the pass as
    (name, sum of the terms' magnitudes, granule).  mutate: one of MUTATIONS (the result is then not the case's)."""
    assert mutate is None or mutate in MUTATIONS
    n, hid = _n_layers(case), case.args['hidden']
    skip = tuple(case.args.get('skip_in', ()))
    W = [effective_weight(case, l) for l in range(n)]
    b = [case.state['lin%d.bias' % l].double()[:, None] for l in range(n)]
    P = case.args['P']
    x = case.inputs['x'].double().t()                      # [3, P]: columns are points, as in the kernels
    n_clamp, n_feat, split = groups(case)
    up = dict(zip('aBC', (t.t() for t in upstream(case, mutate))))
    grid = case.kind == 'grid'
    assert not (grid and (skip or case.args.get('radius', 0.0) > 0))
    sums = []
    if grid:
        geo, x01, aux, J = _grid_terms(case)
        k = 0.5 / GRID_FIXED['divide_factor']              # d x01 / d x
        emb = case.state['encoding.embeddings'].double()
        sums.append(('grid.features', hg.encode_forward(x01, emb.abs(), geo, False)[0], 1 / 8 * granule(emb)))
    pr, pre, h = [], [], [torch.cat([x, aux], 0) if grid else x]
    # forward chain (all three kernels)
    hin = []                                               # what layer l multiplies: h_{l-1}, behind a skip [h_{l-1} | x]
    for l in range(hid):
        hin.append(torch.cat([h[-1], x], 0) if l in skip else h[-1])
        pr.append(Product('l%d.fwd' % l, 'forward', 'core', W[l], hin[l], (b[l],), (l, 'f')))
        pre.append(W[l] @ hin[l] + b[l])
        h.append(torch.relu(pre[-1]))
    s = [(p > 0).double() for p in pre]
    # output layer: a matrix product where features are wanted, the sdf row as a dot product otherwise
    pr.append(Product('out.fwd', 'forward', 'core', W[hid], h[-1], (b[hid],), (hid, 'f')))
    pr.append(Product('out.dot', 'dot', 'dot', W[hid][:1], h[-1], (b[hid][:1],), None))
    o = W[hid] @ h[-1] + b[hid]
    # gradient sweep: p_l = s_l g_{l+1}, g_l = W_l^T p_l
    # behind a skip layer's hidden rows the product yields d sdf / d input: its first arrival (the second: layer 0)
    p = {hid - 1: s[hid - 1] * W[hid][:1].t()}
    arrivals = []
    for l in range(hid - 1, -1, -1):
        pr.append(Product('l%d.sweep' % l, 'transposed', 'core', W[l].t(), p[l], (), (l, 't')))
        g = W[l].t() @ p[l]
        if l in skip:
            arrivals.append(g[h[l].shape[0]:])
            g = g[:h[l].shape[0]]
        if l > 0:
            p[l - 1] = s[l - 1] * g
    grad = g[:3]
    if arrivals:
        sums.append(('input_gradient', sum(t.abs() for t in arrivals) + grad.abs(), 1.0))
        if mutate != 'one_input_arrival':
            grad = grad + sum(arrivals)
    # the bounding-sphere clamp, per point among the first n_clamp; a clamped point hands on neither a nor C
    raw, grad_raw = o[:1], grad
    sdf_row = raw
    clamped = torch.zeros(P, dtype=torch.bool)
    if case.args.get('radius', 0.0) > 0:
        c = clamp_restatement(case)
        clamped = (torch.arange(P) < (P if mutate == 'clamp_all' else n_clamp)) & (c.sph < raw[0])
        sdf_row = torch.where(clamped, c.sph, raw[0])[None]
        grad = torch.where(clamped, c.normals.t(), grad)
    live = torch.ones(P, dtype=torch.float64) if mutate == 'clamped_live' else (~clamped).double()
    up['a'], up['C'] = up['a'] * live, up['C'] * live
    if mutate == 'no_feat_grad_when_clamped':
        up['B'] = up['B'] * live
    q0 = up['C']
    if grid:
        # d sdf / d x through the grid: k sum_{l,c} r[l,c] J[l,d,c] with r = d sdf / d features; the gradient arriving at
        # r in the double backward: sum_d (k C_d) J[l,d,c]
        r_aux = g[3:]
        r_lc = r_aux.t().reshape(P, geo['L'], 1, geo['C'])
        grad = grad + k * (r_lc * J).sum((1, 3)).t()
        sums.append(('grid.jacobian_t', k * (r_lc * J).abs().sum((1, 3)) + g[:3].t().abs(), k * granule(r_aux) * granule(J)))
        gg = k * up['C'].t()                               # [P, 3]
        rbar = (gg[:, None, :, None] * J).sum(2).reshape(P, -1).t()
        sums.append(('grid.jacobian', (gg[:, None, :, None] * J).abs().sum(2), granule(gg) * granule(J)))
        q0 = torch.cat([up['C'], rbar], 0)
    # double backward, sweep up: q-bar_0 = C, p-bar_l = W_l q-bar_l, q-bar_{l+1} = s_l p-bar_l
    # (behind a skip the input block of q-bar is C again: the second load_rbar)
    q = [q0]
    for l in range(hid):
        if l in skip:
            q[l] = torch.cat([q[l], q0], 0)
        pr.append(Product('l%d.up' % l, 'forward', 'core', W[l], q[l], (), (l, 'f')))
        q.append(s[l] * (W[l] @ q[l]))
    # sweep down: a-bar of the output layer = [a | B], a-bar_l = s_l W_{l+1}^T a-bar_{l+1} (second-order term: zero)
    ab = {hid: torch.cat([up['a'], up['B']], 0)}
    pr.append(Product('out.down', 'transposed', 'core', W[hid].t(), ab[hid], (), (hid, 't')))
    ab[hid - 1] = s[hid - 1] * (W[hid].t() @ ab[hid])
    for l in range(hid - 1, 0, -1):
        pr.append(Product('l%d.down' % l, 'transposed', 'core', W[l].t(), ab[l], (), (l, 't')))
        ab[l - 1] = s[l - 1] * (W[l].t() @ ab[l])[:h[l].shape[0]]      # (a skip layer's input rows: d loss / d x, unused)
    # weight gradients: d W_l = p_l q-bar_l^T + a-bar_l h_l^T, both terms reduced into one sum
    ones = torch.ones(P, 1, dtype=torch.float64)
    out = {'sdf': sdf_row.t(), 'feat': o[1:].t()[:n_feat], 'grad': grad.t()}
    if case.args.get('radius', 0.0) > 0:
        out['sdf_raw'], out['grad_raw'] = raw.t(), grad_raw.t()
    if grid:
        # the product down to the network input runs for its feature rows: d loss / d features; the table gradient is its
        # scatter plus the second-order term of the grid part of d sdf / d x
        pr.append(Product('l0.down', 'transposed', 'core', W[0].t(), ab[0], (), (0, 't')))
        g_aux = _level_major((W[0].t() @ ab[0])[3:], geo)
        r_lm = _level_major(r_aux, geo)
        n_e = geo['n_entries']
        out['encoding.embeddings'] = hg.encode_backward_grid(g_aux, x01, geo, n_e) + \
            hg.second_backward_embedding(r_lm, x01, gg, geo, n_e)
        # magnitudes: the first-order records are w g (w: multiples of 1/8), the second-order ones +-(w' gg dsm) r, added
        # to one corner and subtracted from its neighbour (w' = 8 x multiples of 1/4, dsm: multiples of 1/2)
        sums.append(('grid.table', hg.encode_backward_grid(g_aux.abs(), x01, geo, n_e) +
                     _second_order_magnitude(r_lm, x01, gg, geo, n_e),
                     min(1 / 8 * granule(g_aux), granule(gg) * granule(r_lm))))
    for l in range(hid):
        A, B = torch.cat([p[l], ab[l]], 1), torch.cat([q[l].t(), hin[l].t()], 0)
        if l in skip:
            # a two-part item (plan.py _col_parts): the hidden columns and the input block, each a product of its own;
            # the reduction applies 1 / sqrt(2) to the finished sums
            nh = h[l].shape[0]
            pr.append(Product('l%d.wgrad' % l, 'wgrad', 'wgrad', A, B[:, :nh], (), None))
            pr.append(Product('l%d.wgrad_in' % l, 'wgrad', 'wgrad', A, B[:, nh:], (), None))
            G = A @ B
            if mutate == 'no_input_columns':
                G[:, nh:] = 0
            sums.append(('l%d.scaled_gradient' % l, G.abs(), 1.0))
            dW = G if mutate == 'no_scale' else scaled_gradient(case, G)
            out['lin%d.weight' % l] = scaled_gradient(case, dW) if mutate == 'scale_twice' else dW
        else:
            pr.append(Product('l%d.wgrad' % l, 'wgrad', 'wgrad', A, B, (), None))
            out['lin%d.weight' % l] = A @ B
        pr.append(Product('b%d.colsum' % l, 'dot', 'dot', ab[l], ones, (), None))
        out['lin%d.bias' % l] = ab[l].sum(1)
    pr.append(Product('out.wgrad', 'wgrad', 'wgrad', ab[hid][1:], h[hid].t(), (), None))
    # the sdf row: sum_p a[p] h[p] (the v-weighted row sums) + the column sums of the last q-bar, plain fp32
    A, B = torch.cat([up['a'], ones.t()], 1), torch.cat([h[hid].t(), q[hid].t()], 0)
    pr.append(Product('out.sdf_row', 'dot', 'dot', A, B, (), None))
    pr.append(Product('b%d.colsum' % hid, 'dot', 'dot', ab[hid], ones, (), None))
    out['lin%d.weight' % hid] = torch.cat([A @ B, ab[hid][1:] @ h[hid].t()], 0)
    out['lin%d.bias' % hid] = ab[hid].sum(1)
    if mutate is None:
        _SUMS[id(case)] = (case, sums)
    return pr, out, pre


def mutated_outputs(case, mutate):
    """The outputs of an SDF case as a kernel with the mistake `mutate` (MUTATIONS) would give them."""
    return _sdf_products(case, mutate)[1]


_SUMS = {}


def other_sums(case):
    """(name, magnitudes, granule) of the fp32 sums outside the matrix products (hash-grid cases; else none)."""
    products(case)
    return _SUMS[id(case)][1] if id(case) in _SUMS and _SUMS[id(case)][0] is case else []


_PRODUCTS = {}


def products(case):
    """(products, the outputs they amount to, pre-activations per layer), computed once per case."""
    return _memo(_PRODUCTS, case, _color_products if case.kind == 'color' else _sdf_products)


def want(pr):
    """The exact result of a product."""
    r = pr.A @ pr.B
    for t in pr.adds:
        r = r + t
    return r


# ---------------------------------------------------------------------------
# exactness certificate
# ---------------------------------------------------------------------------
def split_planes(t, n=3):
    """bf16 planes of an fp32 tensor as b16_split forms them (round to nearest even, exact differences); three planes
    hold every fp32 value."""
    r = t.float().clone()
    planes = []
    for _ in range(n):
        hi = r.to(torch.bfloat16).float()
        planes.append(hi)
        r = r - hi
    assert not r.any()
    return planes


def granule(t):
    """The largest power of two that divides every entry of t (1 for an all-zero tensor)."""
    v = t.double().flatten()
    v = v[v != 0]
    if v.numel() == 0:
        return 1.0
    m, e = torch.frexp(v)
    bits = (m.abs() * 2.0 ** 53).long()
    low = (bits & -bits).double().log2()
    return float(2.0 ** (e.double() - 53 + low).min().item())


def arithmetic(unit, core):
    """How many bf16 planes the unit that forms a product uses on this core: 0 = plain fp32."""
    if core == 'fp32' or unit == 'dot' or (unit == 'wgrad' and core != 'bf16x3'):
        return 0
    return PLANES[core]


_PAIR_MAGS = {}


def _pair_magnitudes(pr):
    """[i][j]: sum over k of |plane i + 1 of A| |plane j + 1 of B|."""
    pa, pb = split_planes(pr.A), split_planes(pr.B)
    return [[pa[i].double().abs() @ pb[j].double().abs() for j in range(3)] for i in range(3)]


def check_product(pr, core):
    """Reasons why the product is NOT certainly exact on this core (empty: it is)."""
    why = []
    A, B = pr.A.double(), pr.B.double()
    for name, t in (('A', A), ('B', B)):
        if not torch.equal(t.float().double(), t):
            why.append('%s: operand %s is not an fp32 value' % (pr.name, name))
    if why:
        return why
    # one granule for every term of the sums: plane values are multiples of their element's granule too
    g = min([granule(A) * granule(B)] + [granule(t) for t in pr.adds])
    mag = torch.zeros(A.shape[0], B.shape[1], dtype=torch.float64)
    for t in pr.adds:
        mag = mag + t.abs()
    ns = arithmetic(pr.unit, core)
    if ns == 0:
        mag = mag + A.abs() @ B.abs()
    else:
        pairs = _memo(_PAIR_MAGS, pr, _pair_magnitudes)
        for i in range(3):
            for j in range(3):
                m = pairs[i][j]
                if (i + 1, j + 1) in KEPT[ns]:
                    mag = mag + m
                elif m.any():
                    why.append('%s: needs the plane product (%d, %d), which %s does not form' % (pr.name, i + 1, j + 1, core))
    if mag.numel() and mag.max().item() >= SUM_BOUND * g:
        why.append('%s: sum of magnitudes %g reaches 2^24 granules of %g' % (pr.name, mag.max().item(), g))
    return why


def check_preactivations(pre):
    """SDF cases: every hidden pre-activation an integer with |a| >= 2 (softplus(beta = 100) is then ReLU exactly)."""
    why = []
    for l, a in enumerate(pre):
        if not torch.equal(a, torch.round(a)):
            why.append('layer %d: a pre-activation is no integer' % l)
        elif a.numel() and a.abs().min().item() < 2:
            why.append('layer %d: a pre-activation of %g' % (l, a.abs().min().item()))
    return why


Certificate = collections.namedtuple('Certificate', 'ok failures')
_CERT = {}


def certificate(case, core):
    """Certificate(ok, failures): whether every sum of the pass is exact on this core -- forward, sweeps, weight
    gradients, dot-product rows -- and why not."""
    def run(case):
        pr, _, pre = products(case)
        why = []
        for p in pr:
            why += check_product(p, core)
        if case.kind != 'color':
            why += check_preactivations(pre)
        if case.args.get('radius', 0.0) > 0:
            why += clamp_conditions(case)
        for name, mag, g in other_sums(case):
            if mag.numel() and mag.max().item() >= SUM_BOUND * g:
                why.append('%s: sum of magnitudes %g reaches 2^24 granules of %g' % (name, mag.max().item(), g))
        return Certificate(not why, why)
    return _memo(_CERT.setdefault(core, {}), case, run)


# ---------------------------------------------------------------------------
# emulation of one product on one core
# ---------------------------------------------------------------------------
def emulate(pr, core, seed=0, drop=None, k_block=8):
    """The product as the unit of this core forms it: both operands split into bf16 planes, the kept plane products,
    fp32 accumulation -- blocks of k_block terms of one plane pair, in a shuffled order, the other summands shuffled in.
    drop: ('pair', (i, j)) | ('ktile', t) | ('otile', t) | ('point', p): what a wrong kernel would lose."""
    ns = arithmetic(pr.unit, core)
    A, B = pr.A.float(), pr.B.float()
    if drop is not None and drop[0] == 'ktile':
        A = A.clone()
        A[:, 16 * drop[1]:16 * drop[1] + 16] = 0
    if drop is not None and drop[0] == 'otile':
        A = A.clone()
        A[16 * drop[1]:16 * drop[1] + 16] = 0
    if drop is not None and drop[0] == 'point':
        B = B.clone()
        B[:, drop[1]] = 0
    if ns == 0:
        pairs = [(A, B)]
    else:
        pa, pb = split_planes(A), split_planes(B)
        pairs = [(pa[i - 1], pb[j - 1]) for i, j in KEPT[ns] if drop is None or drop != ('pair', (i, j))]
    K = A.shape[1]
    terms = [(x[:, k:k + k_block], y[k:k + k_block]) for x, y in pairs for k in range(0, K, k_block)]
    terms += [(None, t.float()) for t in pr.adds]
    g = _gen(seed)
    acc = torch.zeros(A.shape[0], B.shape[1])
    for i in torch.randperm(len(terms), generator=g).tolist():
        x, y = terms[i]
        acc = acc + (y if x is None else x @ y)
    return acc


# ---------------------------------------------------------------------------
# which specialisation a product takes (mlp_core.h gemm_dispatch, mlp_core_b16.h gemm_b16_dispatch)
# ---------------------------------------------------------------------------
F32_SPECIAL = {3: 4, 5: 3, 16: 1, 17: 1}       # K tiles -> pairs of out tiles per weight chunk; anything else: guarded
B16_SPECIAL = (2, 3, 8, 9)                     # K blocks with an unrolled path


def build_plan(case):
    a = case.args
    n = _n_layers(case)
    shapes = [tuple(case.state['lin%d.weight' % l].shape) for l in range(n)]
    if case.kind == 'color':
        return planlib.build_color_plan(shapes, a['mode'], 0, a['F'], 32 if a['code'] else 0, True)
    n_aux = a['num_levels'] * a['level_dim'] if case.kind == 'grid' else 0
    return planlib.build_sdf_plan(shapes, tuple(a.get('skip_in', ())), 0, n_aux, n_aux > 0, a['F'])


def _describe(core, k, ot):
    pairs = (ot + 1) // 2
    d = dict(k=k, out_tiles=ot, pairs=pairs, odd_last_tile=ot % 2 == 1, dead_pair=ot == MT)
    if core == 'fp32':
        ppc = F32_SPECIAL.get(k, 1)
        d.update(kernel='gemm_tiles<%d,%d>' % (k if k in F32_SPECIAL else 0, ppc), pairs_per_chunk=ppc,
                 chunks=-(-pairs // ppc), partial_last_chunk=pairs % ppc != 0)
    else:
        ns = PLANES[core]
        ch = 2 if ns == 2 else 1                # B16Cfg::CH out tiles per chunk
        d.update(kernel='gemm_b16<%d,%d>' % (ns, k if k in B16_SPECIAL else 0), tiles_per_chunk=ch,
                 chunks=-(-ot // ch), partial_last_chunk=ot % ch != 0)
    return d


def structure(case, core):
    """{product name: what the matrix core dispatches on for it}, for the products a matrix core forms -- and, for the
    weight-gradient item of a skip layer (no 'kernel' field), its two column parts as (slot start, width), the tile the
    input block sits at and the layer's kt."""
    mp = build_plan(case)
    plan = mp.plan if core == 'fp32' else mp.build_b16(PLANES[core])
    out = {}
    for l in case.args.get('skip_in', ()) if case.kind == 'sdf' else ():
        L = mp.plan.layer[l]
        parts = planlib._col_parts(L, mp.in0_tiles)
        out['l%d.wgrad' % l] = dict(two_part=len(parts) == 2, parts=parts, skip_tile=L.skip_tile, kt=L.kt)
    for pr in products(case)[0]:
        if pr.key is None:
            continue
        u, side = pr.key
        L = plan.layer[u]
        out[pr.name] = _describe(core, L.ktp, L.ot) if side == 'f' else _describe(core, L.otp, L.kt)
    return out


# What each case is there for: (core, product, the fields of structure() it must show).  A retuning of the dispatch
# (plan.py _pad_k / build_b16, gemm_dispatch, gemm_b16_dispatch) fails these instead of silently uncovering a branch.
REACHES = {
    # three tiles: the odd last tile (one out tile in the last chunk of the two-plane core)
    'color.w48_h2_idr_p65': [
        ('fp32', 'u1.fwd', dict(kernel='gemm_tiles<3,4>', odd_last_tile=True, partial_last_chunk=True, chunks=1)),
        ('fp32', 'u2.fwd', dict(kernel='gemm_tiles<3,4>', odd_last_tile=True)),
        ('bf16x3', 'u2.fwd', dict(kernel='gemm_b16<2,2>', tiles_per_chunk=2, odd_last_tile=True, partial_last_chunk=True)),
        ('bf16x6', 'u2.fwd', dict(kernel='gemm_b16<3,2>', tiles_per_chunk=1, odd_last_tile=True, chunks=3))],
    # 100 = 7 tiles with 12 padded slots, 40 features = 3 tiles with 8 padded slots, misc block of 5 tiles
    'color.w100_h2_idr_code_f40_p63': [
        ('fp32', 'u0.fwd', dict(kernel='gemm_tiles<3,4>', k=3, out_tiles=7)),
        ('fp32', 'u1.fwd', dict(kernel='gemm_tiles<5,3>', pairs=4, chunks=2, partial_last_chunk=True)),
        ('fp32', 'u2.fwd', dict(kernel='gemm_tiles<0,1>', k=7, odd_last_tile=True)),
        ('bf16x3', 'u1.fwd', dict(kernel='gemm_b16<2,3>')), ('bf16x6', 'u1.fwd', dict(kernel='gemm_b16<3,3>')),
        ('bf16x3', 'u2.fwd', dict(kernel='gemm_b16<2,0>', k=4)), ('bf16x6', 'u2.fwd', dict(kernel='gemm_b16<3,0>', k=4))],
    # 11 tiles: several pairs per chunk, the last chunk partial (misc block of 3 tiles) or full (5 tiles)
    'color.w176_h1_idr_p64': [
        ('fp32', 'u1.fwd', dict(kernel='gemm_tiles<3,4>', pairs=6, chunks=2, partial_last_chunk=True, odd_last_tile=True))],
    'color.w176_h2_nerf_code_p17': [
        ('fp32', 'u1.fwd', dict(kernel='gemm_tiles<5,3>', pairs=6, chunks=2, partial_last_chunk=False)),
        ('fp32', 'u2.fwd', dict(kernel='gemm_tiles<0,1>', k=11)),
        ('bf16x3', 'u2.fwd', dict(kernel='gemm_b16<2,8>')), ('bf16x6', 'u2.fwd', dict(kernel='gemm_b16<3,8>'))],
    'color.w256_h3_idr_f256_p16': [
        ('fp32', 'u0.fwd', dict(kernel='gemm_tiles<16,1>')), ('fp32', 'u3.bwd', dict(kernel='gemm_tiles<16,1>')),
        ('bf16x3', 'u2.fwd', dict(kernel='gemm_b16<2,8>')), ('bf16x6', 'u3.bwd', dict(kernel='gemm_b16<3,8>'))],
    'color.w64_h2_idr_code_spr7_p217': [
        ('fp32', 'u1.fwd', dict(kernel='gemm_tiles<5,3>', chunks=1, partial_last_chunk=True)),
        ('fp32', 'u2.fwd', dict(kernel='gemm_tiles<0,1>', k=4))],
    'sdf.w48_h3_f24_p65': [
        ('fp32', 'l1.fwd', dict(kernel='gemm_tiles<3,4>', odd_last_tile=True, partial_last_chunk=True)),
        ('fp32', 'out.fwd', dict(out_tiles=3, odd_last_tile=True)),
        ('bf16x3', 'l1.down', dict(kernel='gemm_b16<2,2>', partial_last_chunk=True))],
    'sdf.w100_h2_p63': [
        ('fp32', 'l0.fwd', dict(kernel='gemm_tiles<3,4>', pairs=4, chunks=1, partial_last_chunk=False)),
        ('fp32', 'l1.fwd', dict(kernel='gemm_tiles<0,1>', k=7)),
        ('bf16x6', 'l1.up', dict(kernel='gemm_b16<3,0>', k=4))],
    # 256 features + the sdf row = 17 out tiles: the dead pair of the odd last tile, K = 17 in the transposed product
    'sdf.w256_h2_f256_p17': [
        ('fp32', 'out.fwd', dict(kernel='gemm_tiles<16,1>', out_tiles=17, dead_pair=True)),
        ('fp32', 'out.down', dict(kernel='gemm_tiles<17,1>', out_tiles=16)),
        ('fp32', 'l0.fwd', dict(kernel='gemm_tiles<3,4>', chunks=2, partial_last_chunk=False)),
        ('bf16x3', 'out.fwd', dict(kernel='gemm_b16<2,8>', dead_pair=True, partial_last_chunk=True)),
        ('bf16x3', 'out.down', dict(kernel='gemm_b16<2,9>')),
        ('bf16x6', 'out.fwd', dict(kernel='gemm_b16<3,8>', dead_pair=True)),
        ('bf16x6', 'out.down', dict(kernel='gemm_b16<3,9>'))],
    'sdf.w64_h2_p213': [
        ('fp32', 'l1.fwd', dict(kernel='gemm_tiles<0,1>', k=4)),
        ('bf16x3', 'l0.fwd', dict(kernel='gemm_b16<2,2>')), ('bf16x6', 'l1.fwd', dict(kernel='gemm_b16<3,2>'))],
    # skip layers: the input block behind 4, 3, 7, 11 and 14 hidden tiles; the transposed product has kt out tiles
    'skip.w64_h3_s2_p213': [
        ('fp32', 'l2.fwd', dict(kernel='gemm_tiles<0,1>', k=7, out_tiles=4)),
        ('fp32', 'l2.sweep', dict(k=4, out_tiles=7, odd_last_tile=True)),
        ('bf16x3', 'l2.fwd', dict(kernel='gemm_b16<2,0>', k=4)), ('bf16x6', 'l2.down', dict(kernel='gemm_b16<3,2>', out_tiles=7)),
    ] + [(c, 'l2.wgrad', dict(two_part=True, parts=[(0, 64), (64, 48)], skip_tile=4, kt=7)) for c in CORES],
    'skip.w48_h2_s1_p65': [
        ('fp32', 'l1.fwd', dict(kernel='gemm_tiles<0,1>', k=6, out_tiles=3)),
        ('fp32', 'l1.sweep', dict(kernel='gemm_tiles<3,4>', out_tiles=6, chunks=1)),
        ('bf16x3', 'l1.up', dict(kernel='gemm_b16<2,3>')), ('bf16x6', 'l1.fwd', dict(kernel='gemm_b16<3,3>')),
    ] + [(c, 'l1.wgrad', dict(two_part=True, parts=[(0, 48), (48, 48)], skip_tile=3, kt=6)) for c in CORES],
    'skip.w100_h3_s2_p63': [
        ('fp32', 'l2.fwd', dict(kernel='gemm_tiles<0,1>', k=10, out_tiles=7)),
        ('bf16x6', 'l2.fwd', dict(kernel='gemm_b16<3,0>', k=5)),
    ] + [(c, 'l2.wgrad', dict(two_part=True, parts=[(0, 112), (112, 48)], skip_tile=7, kt=10)) for c in CORES],
    # kt = 14 padded to the unrolled K = 16 path
    'skip.w176_h4_s2_p17': [
        ('fp32', 'l2.fwd', dict(kernel='gemm_tiles<16,1>', k=16, out_tiles=11)),
        ('fp32', 'l2.sweep', dict(kernel='gemm_tiles<0,1>', k=11, out_tiles=14)),
        ('bf16x3', 'l2.fwd', dict(kernel='gemm_b16<2,8>')),
    ] + [(c, 'l2.wgrad', dict(two_part=True, parts=[(0, 176), (176, 48)], skip_tile=11, kt=14)) for c in CORES],
    # kt = 17 = MT: the register layout's maximum, the tile count of the reference's headline network
    'skip.w227_h3_s2_p65': [
        ('fp32', 'l2.fwd', dict(kernel='gemm_tiles<17,1>', k=17, out_tiles=15)),
        ('fp32', 'l2.sweep', dict(kernel='gemm_tiles<16,1>', out_tiles=17, dead_pair=True)),
        ('bf16x3', 'l2.fwd', dict(kernel='gemm_b16<2,9>')), ('bf16x6', 'l2.up', dict(kernel='gemm_b16<3,9>')),
    ] + [(c, 'l2.wgrad', dict(two_part=True, parts=[(0, 224), (224, 48)], skip_tile=14, kt=MT)) for c in CORES],
    'clamp.w64_h3_s2_r2.5_p65': [(c, 'l2.wgrad', dict(two_part=True, skip_tile=4, kt=7)) for c in CORES],
}
REACHES['skip.w227_h3_s2_p1'] = REACHES['skip.w227_h3_s2_p65']


# ---------------------------------------------------------------------------
# hash-grid cases: the aux layouts of the SDF kernels and the paths of a grid model
# ---------------------------------------------------------------------------
# The five ways ImplicitNetworkGrid runs (model/network.py _SdfBase.evaluate, ops.GridSdfFunction, ops._encode_points),
# and for each the hash-grid entry points one evaluation with its double backward must and must not call:
#   fused_jacobian   fp32 core, two features per level: the SDF kernels read the encoder's level-major tensors and apply
#                    its Jacobian themselves (aux_load_tile<true>, aux_store_tile<true>, aux_jacobian_transpose / _tile)
#   level_major      the same without ops.FUSE_JACOBIAN: the Jacobian by the two small node kernels, pitch 0
#   rows_fp32        fp32 core, level_dim 4 or 8: rows through msdf_hash_transpose, the node kernels at the row pitch
#   rows_b16         the bf16 cores: rows, whatever the level_dim
#   separate         ops.HASH_SCATTER == 'atomic', or level_dim 1: HashEncodeWithJacobian and HashEncodeBackwardFunction
#                    around SdfMlpFunction, rows padded to whole tiles by the module
_NODE = ('msdf_hash_node_forward', 'msdf_hash_node_scatter')
_SMALL = ('msdf_hash_node_input_gradient', 'msdf_hash_node_second_grad')
_REF_ORDER = ('msdf_hash_encode_forward', 'msdf_hash_encode_backward', 'msdf_hash_encode_second_backward')
PATH_CALLS = {
    'fused_jacobian': (_NODE, _SMALL + ('msdf_hash_transpose',) + _REF_ORDER),
    'level_major': (_NODE + _SMALL, ('msdf_hash_transpose',) + _REF_ORDER),
    'rows_fp32': (_NODE + _SMALL + ('msdf_hash_transpose',), _REF_ORDER),
    'rows_b16': (_NODE + _SMALL + ('msdf_hash_transpose',), _REF_ORDER),
    'separate': (_REF_ORDER, ('msdf_hash_node_scatter', 'msdf_hash_transpose') + _SMALL),
}
# the runs of tests/test_gpu_mlp_exact.py: name -> (core, ops.FUSE_JACOBIAN, ops.HASH_SCATTER)
GRID_RUNS = collections.OrderedDict([
    ('fp32', ('fp32', True, 'binned')), ('fp32_unfused', ('fp32', False, 'binned')),
    ('fp32_atomic', ('fp32', True, 'atomic')), ('bf16x6', ('bf16x6', True, 'binned')),
    ('bf16x3', ('bf16x3', True, 'binned'))])


def grid_path(case, core, fuse_jacobian=True, hash_scatter='binned'):
    """Which of the five paths this case takes on this core with these flags of monosdf_amd.ops."""
    C = case.args['level_dim']
    if hash_scatter == 'atomic' or C == 1:
        return 'separate'
    if core == 'fp32' and C == 2:
        return 'fused_jacobian' if fuse_jacobian else 'level_major'
    return 'rows_fp32' if core == 'fp32' else 'rows_b16'


def grid_structure(case):
    """aux_tiles of the plan, L C, and the pieces the lanes of a point take in aux_load_tile / aux_store_tile when the
    tensors are level-major (a lane owns the columns s0 .. s0 + 3, s0 = 16 t + 4 q, of tile t < aux_tiles: two levels
    of two features): 'full' both levels inside, 'half' (s0 + 2 == L C: only when L is odd) the first one, 'empty'
    neither; as [(t, q, piece)] and as counts; `second_tile`: a tile 1 exists."""
    a = case.args
    lc = a['num_levels'] * a['level_dim']
    tiles = build_plan(case).plan.aux_tiles
    pieces = []
    for t in range(tiles):
        for q in range(4):
            s0 = 16 * t + 4 * q
            pieces.append((t, q, 'empty' if s0 >= lc else 'half' if s0 + 2 >= lc else 'full'))
    count = lambda kind, t=None: sum(1 for tt, _, k in pieces if k == kind and (t is None or tt == t))
    half = [(t, q) for t, q, k in pieces if k == 'half']
    return dict(LC=lc, aux_tiles=tiles, second_tile=tiles > 1, pieces=pieces, full=count('full'), half=count('half'),
                empty=count('empty'), half_at=half[0] if half else None, row_pad=16 * tiles - lc,
                hashed=a['logmap'] < 10, level_major=a['level_dim'] == 2)


# (level_dim, num_levels, logmap) -> the fields of grid_structure() the layout is there for
GRID_REACHES = {
    (2, 3, 19): dict(aux_tiles=1, full=1, half=1, empty=2, half_at=(0, 1)),              # half-piece in tile 0
    (2, 5, 19): dict(aux_tiles=1, full=2, half=1, empty=1, half_at=(0, 2)),              # half-piece at q = 2
    (2, 8, 19): dict(aux_tiles=1, full=4, half=0, empty=0),                              # one full tile
    (2, 9, 19): dict(aux_tiles=2, second_tile=True, full=4, half=1, empty=3, half_at=(1, 0)),
    (2, 15, 19): dict(aux_tiles=2, second_tile=True, full=7, half=1, empty=0, half_at=(1, 3)),
    (2, 16, 19): dict(aux_tiles=2, second_tile=True, full=8, half=0, empty=0),           # the reference's own shape
    (2, 4, 9): dict(aux_tiles=1, full=2, half=0, empty=2, hashed=True),                  # colliding corners
    (2, 4, 19): dict(aux_tiles=1, full=2, half=0, empty=2, hashed=False),                # the three first cases
    (4, 3, 19): dict(aux_tiles=1, level_major=False, row_pad=4),
    (4, 8, 19): dict(aux_tiles=2, level_major=False, row_pad=0),
    (8, 2, 19): dict(aux_tiles=1, level_major=False, row_pad=0),
    (8, 4, 19): dict(aux_tiles=2, level_major=False, row_pad=0),
    (1, 5, 19): dict(aux_tiles=1, level_major=False, row_pad=11),                        # rows padded from an odd width
}
# ... and the path each run of GRID_RUNS must take, by level_dim
GRID_PATHS = {
    2: dict(fp32='fused_jacobian', fp32_unfused='level_major', fp32_atomic='separate', bf16x6='rows_b16', bf16x3='rows_b16'),
    4: dict(fp32='rows_fp32', fp32_unfused='rows_fp32', fp32_atomic='separate', bf16x6='rows_b16', bf16x3='rows_b16'),
    8: dict(fp32='rows_fp32', fp32_unfused='rows_fp32', fp32_atomic='separate', bf16x6='rows_b16', bf16x3='rows_b16'),
    1: dict(fp32='separate', fp32_unfused='separate', fp32_atomic='separate', bf16x6='separate', bf16x3='separate'),
}


def assert_grid_reaches(name, run=None):
    """The layout assertions of one grid case and, for a run of GRID_RUNS, the path it must take.  Returns the path."""
    case = ALL_CASES[name]
    a = case.args
    gs = grid_structure(case)
    fields = GRID_REACHES[(a['level_dim'], a['num_levels'], a['logmap'])]
    got = {k: gs[k] for k in fields}
    assert got == fields, (name, got, fields)
    geo = hg.level_geometry(grid_conf(case))
    sizes = {geo['offsets'][l + 1] - geo['offsets'][l] for l in range(geo['L'])}
    assert sizes == ({2 ** a['logmap']} if gs['hashed'] else {729}), (name, sizes)
    if run is None:
        return None
    core, fuse, scatter = GRID_RUNS[run]
    path = grid_path(case, core, fuse, scatter)
    assert path == GRID_PATHS[a['level_dim']][run], (name, run, path)
    return path


def assert_reaches(name, core):
    """The structure assertions of one case on one core (a GPU test runs them before it runs the case)."""
    st = structure(ALL_CASES[name], core)
    for c, product, fields in REACHES.get(name, ()):
        if c == core:
            got = {k: st[product][k] for k in fields}
            assert got == fields, (name, core, product, got, fields)
    if ALL_CASES[name].kind == 'grid':
        assert_grid_reaches(name)


def first_difference(got, want_):
    """None, or where the first differing element of a [rows, columns] result sits: row and column and, for a tensor of
    one row per point, the workgroup, wave, tile, quarter and component of that slot (mlp_core.h: lane = (point & 15,
    quarter), tile t, component r <-> slot 16 t + 4 q + r)."""
    got, want_ = got.detach().cpu().double(), want_.detach().cpu().double()
    if got.shape != want_.shape:
        return dict(shape=(tuple(got.shape), tuple(want_.shape)))
    g2, w2 = got.reshape(got.shape[0], -1) if got.dim() else got.reshape(1, 1), \
        want_.reshape(want_.shape[0], -1) if want_.dim() else want_.reshape(1, 1)
    ne = (g2 != w2).nonzero()
    if ne.numel() == 0:
        return None
    r, c = int(ne[0, 0]), int(ne[0, 1])
    return dict(row=r, column=c, workgroup=r // 64, wave=r % 64 // 16, tile=c // 16, quarter=c % 16 // 4,
                component=c % 4, got=float(g2[r, c]), want=float(w2[r, c]), n_different=int(ne.shape[0]))


# ---------------------------------------------------------------------------
# skip, clamp and group cases (built down here: their builder looks at the pass itself, skip_conditions())
# ---------------------------------------------------------------------------
# the skip layer (every MLP configuration of the reference has one): 61 outputs = four tiles with 13 live slots in the
# last; right behind the input layer; 97 outputs, padded; 173 outputs with kt = 14 padded to the K = 16 path; 224
# outputs = 14 tiles + 3 = kt 17 = MT, the register layout's maximum
SDF_SKIP_CASES = _cases(sdf_case, [
    ('w64_h3_s2_p213', dict(width=64, hidden=3, skip_in=(2,), P=213)),
    ('w48_h2_s1_p65', dict(width=48, hidden=2, skip_in=(1,), P=65)),
    ('w100_h3_s2_p63', dict(width=100, hidden=3, skip_in=(2,), P=63)),
    ('w176_h4_s2_p17', dict(width=176, hidden=4, skip_in=(2,), P=17)),
    ('w227_h3_s2_p1', dict(width=227, hidden=3, skip_in=(2,), P=1)),
])
SDF_SKIP_CASES.update((n, sdf_case(n, seed=110 + i, **kw)) for i, (n, kw) in enumerate([
    ('w227_h3_s2_p65', dict(width=227, hidden=3, skip_in=(2,), P=65))]))
# the bounding-sphere clamp on every point (get_outputs(), get_sdf_vals()): dyadic radius and scale
SDF_CLAMP_CASES = collections.OrderedDict((n, sdf_case(n, seed=120 + i, **kw)) for i, (n, kw) in enumerate([
    ('w64_h2_r2.5_p213', dict(width=64, hidden=2, radius=2.5, sphere_scale=1.0, P=213)),
    ('w100_h2_r3_s0.5_p65', dict(width=100, hidden=2, radius=3.0, sphere_scale=0.5, P=65)),
    ('w64_h3_s2_r2.5_p65', dict(width=64, hidden=3, skip_in=(2,), radius=2.5, sphere_scale=1.0, P=65)),
]))
# the point groups of one launch: three workgroups of 64, the last ragged; (n_clamp, n_feat, split)
GROUPS = [(0, 0, 0), (17, 1, 15), (64, 16, 64), (150, 63, 129), (17, 64, 150), (64, 65, 15), (150, 150, 0),
          (0, 150, 129), (17, 63, 64), (150, 65, 150)]
SDF_GROUP_CASES = collections.OrderedDict()
for _i, (_c, _f, _s) in enumerate(GROUPS):
    _n = 'c%d_f%d_s%d' % (_c, _f, _s)
    SDF_GROUP_CASES[_n] = sdf_case(_n, width=64, hidden=2, P=150, seed=130, radius=2.5, sphere_scale=1.0, n_clamp=_c,
                                   n_feat=_f, split=_s)
for _group, _cs in (('skip', SDF_SKIP_CASES), ('clamp', SDF_CLAMP_CASES), ('group', SDF_GROUP_CASES)):
    for _n, _c in _cs.items():
        ALL_CASES['%s.%s' % (_group, _n)] = _c
