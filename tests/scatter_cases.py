"""Inputs for the tests of the hash grid's table-gradient scatter (csrc/hash_scatter.h), on the CPU only.

exact_case() builds points and gradients for which EVERY fp32 sum of the scatter is exact, whatever its order: the table
gradient of any correct kernel is then bit-equal to the float64 oracle (oracle/hashgrid_oracle.py, the only statement of
the arithmetic used here), and one lost, doubled or misplaced record shows whatever else lands in its entry.

  S = 0, H = 2^n + 1   every level has scale = 2^n exactly and resolution 2^n + 1 (nothing in the entry points looks at
                       S): what kind of level it is -- dense, hashed with a power-of-two size (mask), hashed otherwise
                       (modulo) -- follows from the caller's offsets alone
  x = m / 2^(n+1)      integer m: x * scale = m / 2, fractional position 0 or 1/2, smoothstep in {0, 1/2}, its
                       derivative in {0, 3/2}; corner weights are multiples of 1/8.  m = -1 or m > 2^(n+1): out of range
  grad, grad2, gg      integers in [-4, 4], [-4, 4], [-2, 2]

so every record value is an integer multiple of 2^-3 below 2^12 in magnitude, every product on the way is exact, and every
partial sum is exact while the sum of |value| over an entry's records stays below 2^21 (2^24 steps of 2^-3).  That
condition on the INPUTS is the exactness certificate; a test asserts it before it looks at a GPU result.

structure() restates from the level sizes what the launcher and the kernels decide (workgroups, slices, groups, which
flush, which index form), so that each GPU test can assert that its inputs reach the branch it is named for."""
import numpy as np
import torch

from oracle import hashgrid_oracle as hg

# ---- the constants of monosdf_amd/csrc/hash_scatter.h (a retuning there must fail the structure assertions here) ----
K = dict(
    HB_SLICE_FLOATS=8192,      # floats of one table slice (one LDS accumulator)
    HB_CHUNK=8192,             # first form: records per accumulate workgroup of a crowded bin
    HB_THREADS=256,
    HB_PTS=4,                  # points per thread of the place kernels: HB_PTS * HB_THREADS points per place workgroup
    HB_MAX_SLICES=1024,        # first form: slices per level its LDS histogram holds
    HB_RANK_SHIFT=19,          # first form: (index | rank << 19) needs hsize <= 2^19
    HB2_NS_MAX=8192,           # second form: taken when no more slices than this (otherwise the first form)
    HB2_TILE=256,              # second form: runs per pass of the accumulate kernel
    HG_LDS_MAX_BYTES=100 * 1024,   # atomic form: a level whose dense table fits this is accumulated in LDS
    HG_LDS_WGS=128,            # ... by this many workgroups per level
    HG_LDS_THREADS=1024,
)
WG_POINTS = K['HB_PTS'] * K['HB_THREADS']
ROW, WAVE = 16, 64             # runs of equal cells are merged inside 16-lane rows of a 64-lane wave

GRAN = 2.0 ** -3               # every record value is a multiple of this
SUM_BOUND = 2.0 ** 21          # ... and every entry's sum of |value| stays below this


def _cdiv(a, b):
    return -(-a // b)


def make_geo(n, C, sizes):
    """The oracle's geometry dict for S = 0, H = 2^n + 1 and the given level sizes (entries per level)."""
    offsets = [0]
    for s in sizes:
        offsets.append(offsets[-1] + int(s))
    return dict(D=3, L=len(sizes), C=int(C), H=2 ** n + 1, S=0.0, per_level_scale=1.0, offsets=offsets,
                n_entries=offsets[-1])


def level_kind(geo, level):
    """'dense' | 'mask' | 'modulo': the index form of hg_level() for this level."""
    hsize = geo['offsets'][level + 1] - geo['offsets'][level]
    _, res = hg.level_scale(geo, level)
    stride, d = 1, 0
    while d < 3 and stride <= hsize:
        stride *= res
        d += 1
    if stride <= hsize:
        return 'dense'
    return 'mask' if hsize & (hsize - 1) == 0 else 'modulo'


def structure(geo, B, C):
    """What hg_table_gradient / hb_run and the kernels decide for this geometry and batch, from the level sizes alone."""
    L, off = geo['L'], geo['offsets']
    epb = K['HB_SLICE_FLOATS'] // C
    n_wg = _cdiv(B, WG_POINTS)
    total_slices = _cdiv(geo['n_entries'] * C, K['HB_SLICE_FLOATS'])
    ns_bound = total_slices + 1
    levels = []
    for l in range(L):
        hsize = off[l + 1] - off[l]
        ns = _cdiv(hsize, epb)
        G = min(ns, n_wg)
        groups = _cdiv(n_wg, G)
        levels.append(dict(
            hsize=hsize, kind=level_kind(geo, l), ns=ns, partial_last_slice=(hsize * C) % K['HB_SLICE_FLOATS'] != 0,
            # second form (hb2_*)
            G=G, groups=groups, partial_group=n_wg % G != 0, shared_slice=G < n_wg, zero_share=ns < n_wg,
            passes=_cdiv(G, K['HB2_TILE']), items=ns * groups,
            # first form (hb_*): the LDS histogram of the count kernel; the packed ranks of the place kernel
            count_local=ns <= K['HB_MAX_SLICES'],
            place_local=ns <= K['HB_MAX_SLICES'] and hsize <= (1 << K['HB_RANK_SHIFT']),
            hashed=level_kind(geo, l) != 'dense'))
    return dict(n_wg=n_wg, last_wg_partial=B % WG_POINTS != 0, ns_bound=ns_bound,
                second_form=ns_bound <= K['HB2_NS_MAX'], levels=levels,
                items=sum(v['items'] for v in levels), work_max=total_slices + L + L * n_wg)


def atomic_structure(geo, B, C):
    """What hg_small_levels and hg_scatter_lds_kernel decide for the atomic form: the leading levels whose DENSE table
    (resolution^3 entries of C floats) fits HG_LDS_MAX_BYTES go to the LDS kernel, with an LDS table of `lds_floats`
    floats (the largest of them, rounded up to 256 bytes); inside it a level whose real table (hsize * C floats) is
    larger than that falls back to direct atomics."""
    n_small, nbytes = 0, 0
    for l in range(geo['L']):
        _, res = hg.level_scale(geo, l)
        b = res ** 3 * C * 4
        if b > K['HG_LDS_MAX_BYTES']:
            break
        nbytes = max(nbytes, b)
        n_small += 1
    lds_floats = ((nbytes + 255) & ~255) // 4
    sizes = [geo['offsets'][l + 1] - geo['offsets'][l] for l in range(n_small)]
    per = _cdiv(B, K['HG_LDS_WGS'])
    return dict(n_small=n_small, lds_floats=lds_floats, fits=[s * C <= lds_floats for s in sizes],
                kinds=[level_kind(geo, l) for l in range(n_small)], per=per,
                empty_wgs=sum(1 for w in range(K['HG_LDS_WGS']) if w * per >= B))


def first_form_chunks(geo, x, C):
    """Per level, the accumulate work items (chunks of HB_CHUNK records) of every bin of the first form: a histogram of the
    slice index of every corner of every in-range point (no run merging in that form)."""
    epb = K['HB_SLICE_FLOATS'] // C
    ok = hg._in_range(x)
    out = []
    for l in range(geo['L']):
        hsize = geo['offsets'][l + 1] - geo['offsets'][l]
        _, res, cell, _, _ = hg._locate(x, geo, l)
        counts = np.zeros(_cdiv(hsize, epb), np.int64)
        for corner in range(8):
            p = cell[ok].clone()
            for d in range(3):
                p[:, d] += (corner >> d) & 1
            counts += np.bincount((hg.grid_index(p, hsize, res) // epb).numpy(), minlength=counts.size)
        out.append(_cdiv(counts, K['HB_CHUNK']))
    return out


# ---- point patterns: placed by index, because point b of a place workgroup is (blk * 4 + p) * 256 + tid ----
def run_table(B):
    """[(first point, length, kind)]: runs of points in one cell.  kind 'same': identical points; 'mixed': one cell,
    fractional positions 0 and 1/2 mixed (the merged values differ); 'cut': identical points, one in the middle out of
    range.  Only the runs that fit into B points are returned; the last one ends at B - 1."""
    runs = [(32, 1, 'same'), (34, 2, 'same'), (40, 3, 'same'), (48, 15, 'same'), (64, 16, 'same'), (80, 17, 'same'),
            (128, 64, 'same'), (300, 130, 'same'),
            (13 * ROW - 1, 4, 'same'),                  # starts at lane 15 of a row
            (15 * ROW - 1, 1, 'same'),                  # a run of one there
            (17 * ROW - 3, 6, 'same'),                  # straddles a row
            (7 * WAVE - 2, 5, 'same'),                  # ... a wave
            (K['HB_THREADS'] - 4, 9, 'same'),           # ... a p boundary (next point of the same thread)
            (WG_POINTS - 5, 11, 'same'),                # ... a workgroup boundary
            (2 * WG_POINTS - 8, 20, 'mixed'),           # ... the next one, with differing values
            (600, 12, 'cut'), (640, 14, 'mixed'), (672, 33, 'mixed')]
    tail = min(19, (B + 1) // 2)
    runs = [r for r in runs if r[0] + r[1] <= B - tail]
    runs.append((B - tail, tail, 'same'))               # ends at B - 1: the lanes past B re-read point B - 1
    return runs


def exact_points(rng, n, B, n_oob=20):
    """int64 [B, 3] numerators m of x = m / 2^(n+1): random cells, then the runs of run_table(), then out-of-range points."""
    top = 2 ** (n + 1)
    m = rng.integers(0, top + 1, size=(B, 3))
    for start, length, kind in run_table(B):
        cell = rng.integers(0, top // 2, size=3)
        if kind == 'mixed':
            m[start:start + length] = 2 * cell + rng.integers(0, 2, size=(length, 3))
        else:
            m[start:start + length] = 2 * cell + rng.integers(0, 2, size=3)
        if kind == 'cut':
            m[start + length // 2, rng.integers(0, 3)] = -1
    covered = np.zeros(B, bool)
    for start, length, _ in run_table(B):
        covered[start:start + length] = True
    free = np.flatnonzero(~covered)
    if free.size:
        pick = rng.choice(free, size=min(n_oob, free.size), replace=False)
        m[pick, rng.integers(0, 3, size=pick.size)] = np.where(rng.integers(0, 2, size=pick.size) == 0, -1, top + 3)
    return m


def table_gradients(geo, x, grad, grad2, gg):
    """The oracle's table gradients (first term, second term) in the dtype of the operands."""
    n = geo['n_entries']
    first = hg.encode_backward_grid(grad, x, geo, n)
    second = hg.second_backward_embedding(grad2, x, gg, geo, n) if grad2 is not None else None
    return first, second


def sum_abs_majorant(geo, x, grad, grad2, gg):
    """Per entry, an upper bound of the sum of |record value| over everything that lands in it: a corner weight is at
    most 1 and so is a product of two, hence every corner value of (point b, level l) is at most
        u = max_c |grad| + scale * sum_d (|gg_d| * smoothstep'_d) * max_c |grad2|
    in magnitude; u is added to the point's eight corners (cells and indices from the oracle)."""
    out = torch.zeros(geo['n_entries'], dtype=torch.float64)
    ok = hg._in_range(x)
    for l in range(geo['L']):
        hsize = geo['offsets'][l + 1] - geo['offsets'][l]
        scale, res, cell, _, dsm = hg._locate(x, geo, l)
        u = grad[l].abs().amax(1)
        if grad2 is not None:
            u = u + scale * (gg.abs() * dsm).sum(1) * grad2[l].abs().amax(1)
        u = (u * ok).double()
        for corner in range(8):
            p = cell.clone()
            for d in range(3):
                p[:, d] += (corner >> d) & 1
            out.index_add_(0, hg.grid_index(p, hsize, res) + geo['offsets'][l], u)
    return out


class ExactCase:
    """geo, the operands (float32 CPU tensors: x [B,3], grad / grad2 [L,B,C], gg [B,3]), the float64 references `first`,
    `second`, `both` ([n_entries, C]; second / both None for C = 1) and the exactness certificate."""

    def __init__(self, seed, n, C, sizes, B, n_oob=20):
        rng = np.random.default_rng(seed)
        self.n, self.C, self.B, self.sizes = n, C, B, list(sizes)
        self.geo = geo = make_geo(n, C, sizes)
        L = geo['L']
        self.m = exact_points(rng, n, B, n_oob)
        self.x = torch.from_numpy(self.m / float(2 ** (n + 1))).float()
        self.grad = torch.from_numpy(rng.integers(-4, 5, size=(L, B, C))).float()
        self.grad2 = torch.from_numpy(rng.integers(-4, 5, size=(L, B, C))).float()
        self.gg = torch.from_numpy(rng.integers(-2, 3, size=(B, 3))).float()
        self.second_order = C > 1                      # the reference has no C = 1 second backward, nor has the library
        x64, g64 = self.x.double(), self.grad.double()
        g2 = self.grad2.double() if self.second_order else None
        self.first, self.second = table_gradients(geo, x64, g64, g2, self.gg.double())
        self.both = self.first + self.second if self.second_order else None
        # the issue's quantity (the oracle on |operands|) and the majorant that bounds every partial sum
        a1, a2 = table_gradients(geo, x64, g64.abs(), None if g2 is None else g2.abs(), self.gg.double().abs())
        self.abs_oracle = a1 + a2.abs() if self.second_order else a1
        self.majorant = sum_abs_majorant(geo, x64, g64, g2, self.gg.double())

    def references(self):
        return [t for t in (self.first, self.second, self.both) if t is not None]

    def certificate(self):
        """{'granular': every reference value is a multiple of 2^-3, 'max_sum_abs': the largest per-entry bound,
        'bounded': it is below 2^21, 'ok'}."""
        granular = all(bool(((t / GRAN).round() * GRAN == t).all()) for t in self.references())
        top = max(float(self.abs_oracle.max()), float(self.majorant.max()))
        covers = all(bool((t.abs().amax(1) <= self.majorant).all()) for t in self.references())
        return dict(granular=granular, max_sum_abs=top, bounded=top < SUM_BOUND, majorant_covers=covers,
                    ok=granular and covers and top < SUM_BOUND)

    def oracle_float32(self):
        """(first, second, both) from the oracle evaluated in float32 (exact inputs: equal to float64 bit for bit)."""
        f, s = table_gradients(self.geo, self.x, self.grad, self.grad2 if self.second_order else None, self.gg)
        return f, s, (f + s if s is not None else None)

    def level_rows(self, level):
        return slice(self.geo['offsets'][level], self.geo['offsets'][level + 1])


def exact_case(seed, n, C, sizes, B, n_oob=20):
    return ExactCase(seed, n, C, sizes, B, n_oob)


# ---- the cases of tests/test_gpu_hash_scatter.py, shared with tests/test_hash_scatter_cpu.py ----
N_EXP = 6                                              # H = 65: scale 64, resolution 65
DENSE = (2 ** N_EXP + 1) ** 3                           # 274,625 entries: odd, so the last slice is partial for every C
B_MULTI = 3109                                         # four place workgroups, the last partial; not a multiple of 16


def sizes_every_entry_point(C):
    """2a: dense with many slices and a partial last one | one full slice, power of two (mask) | three slices, not a
    power of two (modulo): 1 < ns < n_wg, n_wg % ns != 0 | tiny (fewer than 256 floats)."""
    return [DENSE, K['HB_SLICE_FLOATS'] // C, 24334 // C, 25]


SIZES_BATCH_EDGES = [DENSE, 2048, 3001]                 # 2b, C = 2: dense, mask, modulo
BATCH_EDGES = (1, 15, 16, 17, 1023, 1024, 1025, 2049)
SIZES_SECOND_PASS = [2 ** 18 + 8]                       # 2c, C = 8: 257 slices
B_SECOND_PASS = 262144 + 1061                           # 258 place workgroups


def first_form_geometry(C, which):
    """2d, (n, level sizes).  'large' (n = 7, resolution 129: a level of 2^19 + 8 entries is hashed): hsize > 2^19 (place
    kernel without packed ranks; modulo) | one full slice taking every record (chunks > 1, shared flag, atomic flush) |
    C = 8 only: more than HB_MAX_SLICES slices (count kernel without its LDS histogram).  'side' (n = 5, resolution 33): a
    dense level (ds_add_f32 adds) next to a hashed one (compare-and-swap adds)."""
    if which == 'large':
        return 7, [2 ** 19 + 8, K['HB_SLICE_FLOATS'] // C] + ([2 ** 20 + 8] if C == 8 else [])
    assert which == 'side', which
    return 5, [33 ** 3, 24334 // C]


FIRST_FORM_CASES = [(C, which) for C in (1, 2, 8) for which in ('large', 'side')]

# 2f, the atomic form's LDS kernel (H = 17, resolution 17: every level is "small"): the dense level fills the LDS table
# exactly | a dense index with slack, larger than the LDS table (direct atomics from inside the kernel) | tiny, modulo
N_EXP_LDS = 4
SIZES_LDS_ATOMIC = [17 ** 3, 8192, 25]
LDS_ATOMIC_CHANNELS = (1, 2, 4)                        # C = 8: 157 KB, not an LDS level


_CACHE = {}


def cached_case(name, *args):
    """One ExactCase per (name, arguments) and process: the reference is computed once and never modified."""
    key = (name,) + tuple(map(str, args))
    if key not in _CACHE:
        _CACHE[key] = ExactCase(*args)
    return _CACHE[key]


def case_every_entry_point(C):
    return cached_case('entry', 100 + C, N_EXP, C, sizes_every_entry_point(C), B_MULTI)


def case_batch_edge(B):
    return cached_case('edge', 200 + B, N_EXP, 2, SIZES_BATCH_EDGES, B, min(20, B // 8))


def case_second_pass():
    return cached_case('pass2', 300, N_EXP, 8, SIZES_SECOND_PASS, B_SECOND_PASS, 200)


def case_first_form(C, which):
    n, sizes = first_form_geometry(C, which)
    return cached_case('first', 400 + C, n, C, sizes, B_MULTI)


def case_lds_atomic(C):
    return cached_case('lds', 500 + C, N_EXP_LDS, C, SIZES_LDS_ATOMIC, B_MULTI)


# ---- 2e: realistic geometry (S != 0), random float operands: not exact, compared per level ----
REAL_CONFIGS = (dict(num_levels=16, level_dim=2, logmap=19, base_size=16, end_size=2048),
                dict(num_levels=4, level_dim=2, logmap=10, base_size=16, end_size=64),
                dict(num_levels=6, level_dim=4, logmap=12, base_size=8, end_size=128),
                dict(num_levels=3, level_dim=8, logmap=11, base_size=4, end_size=32))
N_RAYS, PER_RAY = 30, 98


class RealCase:
    """One configuration of REAL_CONFIGS at B = 3,109: 30 rays x 98 ray-ordered samples with step sizes from 2e-5 to 5e-3
    (runs of every length on every level), then random points with cell borders and out-of-range points among them.
    float64 oracle references, and per level the deviation of the float32 oracle from them (rel_level)."""

    def __init__(self, index):
        g = torch.Generator().manual_seed(41 + index)
        self.geo = geo = hg.level_geometry(REAL_CONFIGS[index])
        B, L, C = B_MULTI, geo['L'], geo['C']
        self.B = B
        o = torch.rand(N_RAYS, 1, 3, generator=g) * 0.8 + 0.1
        d = torch.nn.functional.normalize(torch.randn(N_RAYS, 1, 3, generator=g), dim=-1)
        step = 2e-5 * (250.0 ** torch.rand(N_RAYS, 1, 1, generator=g))
        t = torch.arange(PER_RAY).view(1, PER_RAY, 1) * step
        x = torch.cat([(o + t * d).reshape(-1, 3), torch.rand(B - N_RAYS * PER_RAY, 3, generator=g)])
        x[-40:-33] = torch.tensor([0.0, 1.0, 0.5])          # cell borders
        x[-30:-26] = torch.tensor([1.2, 0.5, -0.1])         # out of range
        x[5::97] = 1.5                                      # ... breaking runs
        x[1000:1100] = x[1000].clone()                      # 100 identical points across rows, waves and a workgroup
        self.x = x.contiguous()
        self.grad = torch.randn(L, B, C, generator=g)
        self.grad2 = torch.randn(L, B, C, generator=g)
        self.gg = torch.randn(B, 3, generator=g)
        d64 = table_gradients(geo, self.x.double(), self.grad.double(), self.grad2.double(), self.gg.double())
        d32 = table_gradients(geo, self.x, self.grad, self.grad2, self.gg)
        self.ref = dict(first=d64[0], second=d64[1], both=d64[0] + d64[1])
        self.ref32 = dict(first=d32[0], second=d32[1], both=d32[0] + d32[1])
        self.oracle_dev = {k: [rel_level(self.ref32[k], self.ref[k], geo, l) for l in range(L)] for k in self.ref}


def rel_level(a, b, geo, level):
    """max |a - b| / max |b| over the rows of one level."""
    rows = slice(geo['offsets'][level], geo['offsets'][level + 1])
    a, b = a[rows].detach().double().cpu(), b[rows].detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max()).item()


def real_case(index):
    key = ('real', index)
    if key not in _CACHE:
        _CACHE[key] = RealCase(index)
    return _CACHE[key]


def first_difference(got, want, geo):
    """None if equal, else 'level l, entry e (row r of the table), channel c: got g, want w (k entries differ)' for the
    first differing value, level by level."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    for l in range(geo['L']):
        lo, hi = geo['offsets'][l], geo['offsets'][l + 1]
        bad = ~((got[lo:hi] == want[lo:hi]))
        if bad.any():
            e, c = [int(v) for v in bad.nonzero()[0]]
            return 'level %d (%d entries), entry %d (table row %d), channel %d: got %r, want %r; %d values of this level differ' % (
                l, hi - lo, e, lo + e, c, got[lo + e, c].item(), want[lo + e, c].item(), int(bad.sum()))
    return None
