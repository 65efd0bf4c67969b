"""Inputs and references for the tests of the hash grid's read side (csrc/hashgrid.hip outside hash_scatter.h), on the
CPU only.

GatherCase builds points, tables and gradients on which EVERY fp32 product and sum of the gather kernels is exact, in
any order: outputs, dy_dx, the input gradient and the second-order gradient of a correct kernel are then bit-equal to
the float64 oracle (oracle/hashgrid_oracle.py, the only statement of the arithmetic used here).

  S = 0, H = 2^n + 1   as tests/scatter_cases.py: every level has scale 2^n and resolution 2^n + 1, and the index form
                       (dense, mask, modulo) follows from the caller's offsets alone
  x = m / 2^(n+2)      integer m: x * scale = m / 4, fractional position in {0, 1/4, 1/2, 3/4}, smoothstep in
                       {0, 5/32, 1/2, 27/32}, its derivative in {0, 9/8, 3/2}.  Half cells are not enough: their eight
                       corner weights are equal whenever all are non-zero, so a kernel that handed corner k the weight of
                       corner k' would pass.  On quarter cells the two weights of an axis differ.
                       m = -1 or m = 2^(n+2) + 1: out of range
  table, grad, gg      integers in [-2, 2]

so outputs are multiples of 2^-15, dy_dx of 2^(n-13), and every product on the way fits 24 bits.  certificate() checks
what that argument needs on the case's own numbers; a test asserts it before it looks at a GPU result.

GatherRealCase is the realistic geometry of scatter_cases.RealCase (same points) with a random float table, compared
level by level."""
import numpy as np
import torch

import scatter_cases as sc
from oracle import hashgrid_oracle as hg

SUM_BOUND = 2.0 ** 24


def _multiple(t, g):
    return bool(((t / g).round() * g == t).all())


def exact_points(rng, n, B):
    """int64 [B, 3] numerators m of x = m / 2^(n+2).  The first half (rounded up) and the last point: inside a cell on
    all three axes (m % 4 != 0); the first quarter and the last point at 1/4 or 3/4 on every axis.  Then random quarter
    positions, cell borders among them, and from B >= 8 on: a point on 0, a point on 1, a point with both among its
    coordinates, one below 0 and one above 1, then a few more of each."""
    top = 2 ** (n + 2)
    m = rng.integers(0, top + 1, size=(B, 3))
    inside = 4 * rng.integers(0, top // 4, size=(B, 3)) + rng.integers(1, 4, size=(B, 3))
    half = (B + 1) // 2
    m[:half] = inside[:half]
    m[B - 1] = inside[B - 1]
    skew = 4 * rng.integers(0, top // 4, size=(B, 3)) + rng.choice([1, 3], size=(B, 3))
    m[:(B + 3) // 4] = skew[:(B + 3) // 4]               # ... and off the middle too: the two weights of an axis differ
    m[B - 1] = skew[B - 1]
    if B >= 8:
        free = np.arange(half, B - 1)
        m[free[0]] = 0
        m[free[1]] = top
        m[free[2]] = (0, top, inside[free[2], 2])
        m[free[3], 0] = -1
        m[free[4], 2] = top + 1
        rest = free[5:]
        k = min(len(rest) // 4, 12)
        if k:
            pick = rng.choice(rest, size=k, replace=False)
            kinds = rng.integers(0, 4, size=k)
            axes = rng.integers(0, 3, size=k)
            m[pick, axes] = np.choose(kinds, [0, top, -1, top + 1])
    return m


class GatherCase:
    """geo; the operands as float32 CPU tensors: x01 [B, 3], emb [n_entries, C], grad [L, B, C], gg [B, 3], inout [B, 3];
    the float64 references: outputs [L, B, C], dy_dx [B, L 3 C] (the reference's layout), dy_lm [L, B, 3 C] (level-major),
    grad_inputs [B, 3], grad_grad [L, B, C]."""

    def __init__(self, seed, n, C, sizes, B):
        rng = np.random.default_rng(seed)
        self.n, self.C, self.B, self.sizes = n, C, B, list(sizes)
        self.geo = geo = sc.make_geo(n, C, sizes)
        L = self.L = geo['L']
        self.m = exact_points(rng, n, B)
        self.x01 = torch.from_numpy(self.m / float(2 ** (n + 2))).float()
        self.emb = torch.from_numpy(rng.integers(-2, 3, size=(geo['n_entries'], C))).float()
        self.grad = torch.from_numpy(rng.integers(-2, 3, size=(L, B, C))).float()
        self.gg = torch.from_numpy(rng.integers(-2, 3, size=(B, 3))).float()
        self.inout = torch.from_numpy(rng.integers(-3, 4, size=(B, 3))).float()
        x64, e64 = self.x01.double(), self.emb.double()
        self.outputs, self.dy_dx = hg.encode_forward(x64, e64, geo, True)
        self.dy_lm = self.level_major(self.dy_dx)
        self.grad_inputs = hg.encode_backward_input(self.grad.double(), self.dy_dx, geo)
        self.grad_grad = hg.second_backward_grad(self.gg.double(), self.dy_dx, geo)
        self.in_range = hg._in_range(x64)

    # ---- layouts ----
    def level_major(self, dy):
        """[B, L 3 C] -> [L, B, 3 C]."""
        return dy.reshape(self.B, self.L, 3 * self.C).permute(1, 0, 2).contiguous()

    def rows(self, t, pitch, pad=0.0):
        """[L, B, C] -> point-major [B, pitch] (level l, channel c at column l C + c), the padding columns = pad."""
        m = torch.full((self.B, pitch), float(pad), dtype=t.dtype)
        m[:, :self.L * self.C] = t.permute(1, 0, 2).reshape(self.B, self.L * self.C)
        return m

    def world(self, divide_factor):
        """World coordinates whose x01 = (x / divide_factor + 1) / 2 is exactly self.x01 (divide_factor a power of two)."""
        x = (self.x01.double() * 2 - 1) * divide_factor
        assert torch.equal(x.float().double(), x)
        assert torch.equal(((x.float() * np.float32(1.0 / divide_factor) + 1) * 0.5), self.x01)
        return x.float()

    def padded_pitch(self):
        """L C rounded up to 16, with at least one padding column."""
        return (self.L * self.C // 16 + 1) * 16

    # ---- the references of the node forms ----
    def node_input_gradient(self, scale):
        """inout + r * scale, r the input gradient: exact for scale a power of two."""
        return self.inout.double() + self.grad_inputs * scale

    def node_second_grad(self, scale, n_split, have_a=True, have_b=True):
        """(gg_out [B, 3], grad_grad [L, B, C]) of msdf_hash_node_second_grad with g_a = gg[:n_split], g_b = gg[n_split:]."""
        g = self.gg.double() * scale
        if not have_a:
            g[:n_split] = 0
        if not have_b:
            g[n_split:] = 0
        return g, hg.second_backward_grad(g, self.dy_dx, self.geo)

    # ---- the certificate ----
    def certificate(self):
        """granular: every reference value is a multiple of its granule.  bounded: for each output element of each
        kernel the sum of |terms| stays below 2^24 granules (`max_granules`: the largest, per kernel).  f32_equal: the
        oracle evaluated in float32 equals the float64 oracle bit for bit."""
        geo, n = self.geo, self.n
        g_out, g_dy = 2.0 ** -15, 2.0 ** (n - 13)
        granular = _multiple(self.outputs, g_out) and _multiple(self.dy_dx, g_dy) and \
            _multiple(self.grad_inputs, g_dy) and _multiple(self.grad_grad, g_dy) and \
            _multiple(self.node_input_gradient(0.25), g_dy / 4)
        x64 = self.x01.double()
        scale = float(2 ** n)
        # forward: the weights are non-negative; dy_dx: the four weights of the other two axes sum to 1, a difference of
        # two table values is at most twice the largest
        mag = dict(outputs=hg.encode_forward(x64, self.emb.double().abs(), geo, False)[0].max().item() / g_out)
        dsm = hg._locate(x64, geo, 0)[4]
        mag['dy_dx'] = (scale * dsm.max().item() * 2 * self.emb.abs().max().item()) / g_dy
        mag['grad_inputs'] = (hg.encode_backward_input(self.grad.double().abs(), self.dy_dx.abs(), geo).max().item()
                              + self.inout.abs().max().item() * 4) / g_dy
        mag['grad_grad'] = hg.second_backward_grad(self.gg.double().abs(), self.dy_dx.abs(), geo).max().item() / g_dy
        o32, d32 = hg.encode_forward(self.x01, self.emb, geo, True)
        gi32 = hg.encode_backward_input(self.grad, d32, geo)
        gg32 = hg.second_backward_grad(self.gg, d32, geo)
        f32_equal = all(torch.equal(a.double(), b) for a, b in ((o32, self.outputs), (d32, self.dy_dx),
                                                                (gi32, self.grad_inputs), (gg32, self.grad_grad)))
        bounded = max(mag.values()) < SUM_BOUND
        return dict(granular=granular, max_granules=mag, bounded=bounded, f32_equal=f32_equal,
                    ok=granular and bounded and f32_equal)

    # ---- what the points reach ----
    def structure(self):
        """kinds: level_kind of every level; per level kind the number of in-range points inside a cell on all three
        axes (`generic`: all eight corner weights non-zero) -- S = 0, so it is the same number on every level; `skew`:
        those of them at 1/4 or 3/4 on every axis (the two weights of each axis differ: `weights_distinct`); the numbers of out-of-range points and of points with a coordinate exactly on 0 / on 1;
        whether the upper corners of a point on 1 leave a dense level's res^3 entries (the modulo brings them back)."""
        top = 2 ** (self.n + 2)
        m = torch.from_numpy(self.m)
        ok = self.in_range
        generic = ok & (m % 4 != 0).all(1)
        skew = generic & (m % 4 != 2).all(1)
        frac = (m % 4).double() / 4
        sm = frac * frac * (3 - 2 * frac)
        distinct = bool((sm != 1 - sm)[skew].all())
        kinds = [sc.level_kind(self.geo, l) for l in range(self.L)]
        res = 2 ** self.n + 1
        on1 = ok & (m == top).any(1)
        beyond = []
        for l, k in enumerate(kinds):
            if k == 'dense' and bool(on1.any()):
                p = (m[on1] // 4) + 1
                beyond.append(bool(((p[:, 0] + p[:, 1] * res + p[:, 2] * res * res) >= res ** 3).any()))
        return dict(kinds=kinds, generic={k: int(generic.sum()) for k in set(kinds)}, weights_distinct=distinct,
                    skew=int(skew.sum()),
                    n_oob=int((~ok).sum()), n_on0=int((ok & (m == 0).any(1)).sum()), n_on1=int(on1.sum()),
                    below=int((m < 0).any(1).sum()), above=int((m > top).any(1).sum()),
                    corner_beyond_dense=bool(beyond) and all(beyond),
                    first_generic=bool(skew[0]), last_generic=bool(skew[-1]))


# ---- the cases of tests/test_gpu_hash_gather.py, shared with tests/test_gather_cases_cpu.py ----
N_EXP = sc.N_EXP                                          # H = 65: scale 64, resolution 65
DENSE = sc.DENSE                                          # 65^3
SIZES_EVERY_FORM = [DENSE, DENSE + 1000, 4096, 3001, 25]  # A1: dense | dense with slack | mask | modulo | tiny (modulo)
KINDS_EVERY_FORM = ['dense', 'dense', 'mask', 'modulo', 'modulo']
B_EVERY_FORM = 1025                                       # four blocks of the forward kernels and one lane
CHANNELS = (1, 2, 4, 8)
SIZES_BATCH_EDGES = sc.SIZES_BATCH_EDGES                  # A2, C = 2: dense, mask, modulo
BATCH_EDGES = (1, 63, 64, 65, 255, 256, 257, 513)
# the other geometries on which the exactness argument was checked: (n, C, sizes)
OTHER_GEOMETRIES = [(6, 2, [DENSE, DENSE + 1000, 4096, 3001, 25, 2 ** 19] + [2 ** 19, 3001 * 7] * 5),
                    (4, 8, [17 ** 3, 17 ** 3 + 100, 1024, 3001, 25]),
                    (7, 1, [2 ** 19, 2 ** 19 + 8, 25])]

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def case_every_form(C):
    return _cached(('form', C), lambda: GatherCase(700 + C, N_EXP, C, SIZES_EVERY_FORM, B_EVERY_FORM))


def case_batch_edge(B):
    return _cached(('edge', B), lambda: GatherCase(800 + B, N_EXP, 2, SIZES_BATCH_EDGES, B))


def case_other(i):
    n, C, sizes = OTHER_GEOMETRIES[i]
    return _cached(('other', i), lambda: GatherCase(900 + i, n, C, sizes, 257))


# ---- A4: the transposes ----
TRANSPOSE_LC = ((5, 1), (3, 2), (16, 2), (4, 8), (31, 8))
TRANSPOSE_B = (1, 63, 64, 65, 129)
HT_PTS, HT_LDS_MAX = 64, 64 * 1024                        # msdf_hash_transpose: points per LDS tile, its LDS limit


def transpose_lds_bytes(L, C):
    return HT_PTS * (L * C + 1) * 4


def transpose_pitches(L, C):
    lc = L * C
    up = -(-lc // 16) * 16
    return (lc, up, up + 16) if up != lc else (lc, up + 16)


# ---- A6: realistic geometry, per level ----
class GatherRealCase:
    """Configuration `index` of scatter_cases.REAL_CONFIGS with the points of scatter_cases.RealCase and a random float
    table in [-1/2, 1/2]: the float64 oracle's outputs [L, B, C] and level-major dy_dx [L, B, 3 C], and per level what
    the float32 oracle deviates from them (`oracle_dev`: the same arithmetic in float32)."""

    def __init__(self, index):
        real = sc.real_case(index)
        self.geo, self.x, self.B = real.geo, real.x, real.B
        L, C = self.geo['L'], self.geo['C']
        g = torch.Generator().manual_seed(77 + index)
        self.emb = torch.rand(self.geo['n_entries'], C, generator=g) - 0.5
        lm = lambda dy: dy.reshape(self.B, L, 3 * C).permute(1, 0, 2).contiguous()
        o64, d64 = hg.encode_forward(self.x.double(), self.emb.double(), self.geo, True)
        o32, d32 = hg.encode_forward(self.x, self.emb, self.geo, True)
        self.ref = dict(outputs=o64, dy_dx=lm(d64))
        ref32 = dict(outputs=o32, dy_dx=lm(d32))
        self.oracle_dev = {k: [rel_level(ref32[k], self.ref[k], l) for l in range(L)] for k in self.ref}

    def bar(self, key, level):
        """4 x what the float32 oracle loses on this level (another order of the 8-term and 4-term sums), at least
        4 x 2^-23."""
        return 4 * max(self.oracle_dev[key][level], 2.0 ** -23)


def rel_level(a, b, level):
    """max |a - b| / max |b| over one level of a level-major tensor."""
    a, b = a[level].detach().double().cpu(), b[level].detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max()).item()


def real_case(index):
    return _cached(('real', index), lambda: GatherRealCase(index))


def first_difference(got, want, levels=1):
    """scatter_cases.first_difference on a tensor of `levels` equal blocks of rows ([L, B, ...]: a level's B points are
    its 'entries'; [B, ...] with levels = 1: one block): None if equal, else the first differing value."""
    got, want = got.detach().cpu(), want.detach().cpu()
    if got.shape != want.shape:
        return 'shape %r, want %r' % (tuple(got.shape), tuple(want.shape))
    rows = got.shape[0] * (got.shape[1] if levels > 1 else 1) if got.dim() > 1 else got.shape[0]
    per = rows // levels
    geo = dict(L=levels, offsets=[l * per for l in range(levels + 1)])
    return sc.first_difference(got.reshape(rows, -1), want.reshape(rows, -1), geo)
