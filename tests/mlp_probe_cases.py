"""Probe networks for the pointwise non-linear code of the fused MLP kernels (csrc/common.h, mlp_core.h, mlp_core_b16.h,
sdf_kernels.h, color_kernels.h), on the CPU only.

tests/mlp_exact_cases.py compares bit for bit and therefore keeps softplus a ReLU, the sigmoid factor 0 or 1 and the
encodings switched off; the parity tests run all of that under 1e-4 of a tensor's maximum.  The networks here route ONE
hidden unit, or ONE encoding slot, into each compared number: all routing weights are 0, +-1 or powers of two and the
inputs lie on dyadic grids, so the routing adds no rounding (certificate()), and each number is compared with a float64
reference under a bound derived from the rounding steps of the kernel's formula.

  softplus probe   ImplicitNetwork(64, 0, 3, 1, [64, 64], no geometric init, no weight norm, multires 0).  Layer 0 is a
                   pass-through: unit j reads channel c(j) = j % 3 with weight 1 and bias 4; x on multiples of 2^-12 in
                   [-2, 2], so a0 = x + 4 in [2, 6] is exact in 15 bits, softplus100 returns a0 itself and its sigmoid
                   factor is exactly 1.  Layer 1 is the probe: diag(2^-k_j), bias -4 2^-k_j, k_j = (j // 3) % 8:
                   a1_j = 2^-k_j x_c(j).  Feature rows of the output layer: the identity; the sdf row depends on what is
                   probed (all ones, one-hot, three-hot)
  encoding probe   the same idea behind the positional encoding: layer 0 selects slot j (weight 1; 1/2 for the raw x
                   slots, whose range is [-1.5, 1.5]) with bias 1.25 -- a pass-through (a0 >= 0.25 > 0.2) with ONE rounding,
                   that of slot + 1.25, which the bounds carry; layer 1 is the identity ('pe_id') or diag(2^-6) with bias
                   -1.25 2^-6 ('pe_probe': 100 a1 in [-1.57, 1.57], where 100 s (1 - s) is between 14 and 25)
  colour probes    RenderingNetwork with one hidden layer: view encoding (hidden unit i = relu(column i + 2), every
                   output row picks one unit, if_hdr) and the sigmoid output (o = relu(f) - relu(-f), if_hdr off)

Restatements (fp32, numpy, one rounding per operation, transcendentals computed in float64 and rounded once):
softplus_restated(), softplus_lean_restated(), sigmoid_restated(), second_order_restated(), pe_slot_restated(),
color_sigmoid_restated().  Each takes mutate = one of MUTANTS: the same formula with one mistake in it;
tests/test_mlp_probe_cases_cpu.py shows that every mutant leaves a bound on some case.

Bounds.  U = 2^-24 is half an ulp relative to the result (the rounding of one plain fp32 operation).  The accuracy of the
transcendentals:
  v_exp_f32, v_log_f32, v_rcp_f32   1 ulp = 2 U relative: the figure of AMD's "CDNA4 Instruction Set Architecture"
                   reference guide for V_EXP_F32, V_LOG_F32 and V_RCP_F32, and of the comment above fast_exp() in
                   csrc/common.h.  v_exp_f32 does not produce subnormals: every bound carries TINY = 2^-126 absolute
  __expf(x)        __builtin_amdgcn_exp2f(0x1.715476p+0f * x) (__clang_hip_math.h): the rounding of the product and of
                   the constant move the exponent by |x| U each, then v_exp_f32
  sincosf          OCML's __ocml_sincos_f32 (__clang_hip_math.h), built to the OpenCL full profile: 4 ulp
The derivations stand in the docstrings of bound_h(), bound_s(), bound_t(), bound_pe() and bound_color_sigmoid().

What these probes cannot see: the threshold select of softplus100 (100 a > 20 returns a).  What it replaces differs
from a by 0.01 log1p(exp(-100 a)) < 2.1e-11, and half an ulp of a >= 0.2 is 7.5e-9: the select is below the rounding of the
value it selects, in any test that looks at h alone.
"""
import collections
import math

import numpy as np
import torch

CORES = ('fp32', 'bf16x3', 'bf16x6')
U = 2.0 ** -24
TINY = 2.0 ** -126
ULP_EXP = ULP_LOG = ULP_RCP = 1
ULP_SINCOS = 4
PLANE2 = 2.0 ** -16                  # bf16x3: a 24-bit operand through two bf16 planes, relative to its magnitude


def plane_lo(v):
    """|v - bf16(v)|: the second plane of an operand.  bf16x3 keeps the pairs (hi, hi), (hi, lo), (lo, hi): where BOTH
    operands of a product have a second plane, (lo, lo) is dropped on top of a 24-bit operand's own 2^-16 -- at most
    2^-8 |x| plane_lo(y), bf16 rounding x's first plane by 2^-8 |x| at most.  In these probes that is the weight-gradient
    product alone (s or t, 24 bits, times a0, 15 bits): every other product has a one-plane weight for one operand."""
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(v, dtype=np.float64))).float()
    return (t - t.bfloat16().float()).abs().double().numpy()


LEAN_THRESHOLD, LEAN_SERIES = 2.1e-11, 6e-10      # the comment of softplus100_lean (mlp_core_b16.h)
f32, f64 = np.float32, np.float64
C144 = f32(144.26950408889634)
LN2F = f32(0.6931471805599453)
SERIES_BELOW = f32(1e-4)
GRID = 2.0 ** -12

MUTANTS = ('select_inverted', 's_wrong_side', 'const_100', 'u_dropped', 's_for_u', 'no_division', 'sincos_swapped',
           'octave_off', 'dval_sign', 'channel_rotated', 'normal_shifted', 'sigmoid_backward_gy')


# the one difference no bound here separates from the correct formula (the module's docstring says why)
UNSEEN = ('threshold_dropped',)


def r32(v):
    """A float64 result rounded once to fp32."""
    return np.asarray(v, dtype=f64).astype(f32)


def ulp32(v):
    """The fp32 ulp at magnitude |v| (float64), 2^-149 at and below the subnormals."""
    v = np.abs(np.asarray(v, dtype=f64))
    ex = np.floor(np.log2(np.maximum(v, 2.0 ** -126)))
    return np.maximum(2.0 ** (ex - 23), 2.0 ** -149)


# ---------------------------------------------------------------------------
# float64 references
# ---------------------------------------------------------------------------
def softplus64(a):
    """nn.Softplus(beta = 100, threshold = 20) in float64."""
    a = np.asarray(a, dtype=f64)
    return np.where(100 * a > 20, a, np.logaddexp(0, 100 * a) / 100)


def sigmoid64(t):
    """1 / (1 + exp(-t)), relatively accurate at both ends."""
    t = np.asarray(t, dtype=f64)
    with np.errstate(over='ignore', under='ignore'):
        e = np.exp(-np.abs(t))
        return np.where(t >= 0, 1 / (1 + e), e / (1 + e))


# ---------------------------------------------------------------------------
# fp32 restatements of the kernels' formulas
# ---------------------------------------------------------------------------
def _exp_part(a, mutate):
    a = np.asarray(a, dtype=f32)
    t = a * (f32(100) if mutate == 'const_100' else C144)
    with np.errstate(under='ignore'):
        e = r32(np.exp2(-np.abs(t.astype(f64))))
    return a, e


def softplus_restated(a, mutate=None):
    """softplus100() of common.h -> (h, takes the series)."""
    a, e = _exp_part(a, mutate)
    ope = f32(1) + e
    with np.errstate(under='ignore'):
        l_series = e * r32(e.astype(f64) * -0.5 + 1.0)
        l_log = r32(np.log2(ope.astype(f64))) * LN2F
        series = e < SERIES_BELOW
        l1p = np.where(~series if mutate == 'select_inverted' else series, l_series, l_log)
        hv = r32(f64(f32(0.01)) * l1p.astype(f64) + np.maximum(a, f32(0)).astype(f64))       # one fma
    return (hv if mutate == 'threshold_dropped' else np.where(a * f32(100) > f32(20), a, hv)), series


def softplus_lean_restated(a, mutate=None):
    """softplus100_lean() of mlp_core_b16.h."""
    a, e = _exp_part(a, mutate)
    lg = r32(np.log2((f32(1) + e).astype(f64)))
    return r32(f64(f32(0.006931471805599453)) * lg.astype(f64) + np.maximum(a, f32(0)).astype(f64))


def sigmoid_restated(h, mutate=None):
    """The sweeps' factor from the saved activation: u = one_minus_sigmoid_from_h(h), s = 1 - u -> (u, s)."""
    h = np.asarray(h, dtype=f32)
    with np.errstate(under='ignore'):
        u = r32(np.exp2((h * (f32(-100) if mutate == 'const_100' else -C144)).astype(f64)))
    s = f32(1) - u
    return (s, u) if mutate == 's_wrong_side' else (u, s)


def second_order_restated(h, pbar, mutate=None):
    """SweepDownHooks::tile with h-bar = 0 and p = s (g = 1): q-bar = s p-bar as the sweep up stores it, p-bar rebuilt as
    q-bar rcp(s), t = 100 u p p-bar, multiplied from the left."""
    u, s = sigmoid_restated(h, mutate)
    pbar = np.asarray(pbar, dtype=f32)
    q = s * pbar
    with np.errstate(divide='ignore', invalid='ignore', under='ignore'):
        rcp = r32(1.0 / s.astype(f64))
        pb = q if mutate == 'no_division' else np.where(s > 0, q * rcp, f32(0))
        first = f32(100) if mutate == 'u_dropped' else f32(100) * (s if mutate == 's_for_u' else u)
        return (first * s) * pb


def pe_slot_restated(j, x, mutate=None):
    """pe_slot() of mlp_core.h for slot j >= 0 of points x [P, 3] (fp32) -> (val, dval, channel); float64 in, float64
    out: the reference."""
    x = np.asarray(x)
    if j < 3:
        return x[:, j].copy(), np.ones(x.shape[0], dtype=x.dtype), j
    m = j - 3
    k, w = divmod(m, 6)
    c = w % 3
    if mutate == 'octave_off':
        k += 1
    fr = x.dtype.type(2.0 ** k)
    arg = (x[:, c] * fr).astype(f64)
    sn, cs = np.sin(arg).astype(x.dtype), np.cos(arg).astype(x.dtype)
    sine = (w < 3) != (mutate == 'sincos_swapped')
    val, dval = (sn, fr * cs) if sine else (cs, -fr * sn)
    if mutate == 'dval_sign':
        dval = -dval
    return val, dval, (c + 1) % 3 if mutate == 'channel_rotated' else c


def color_sigmoid_restated(o, g, mutate=None):
    """Colour output y = 1 / (1 + __expf(-o)) and its backward g y (1 - y), from the stored y."""
    o, g = np.asarray(o, dtype=f32), np.asarray(g, dtype=f32)
    with np.errstate(over='ignore', under='ignore'):
        E = r32(np.exp2((f32(1.4426950408889634) * -o).astype(f64)))
        y = r32(1.0 / (f32(1) + E).astype(f64))
    return y, (g * y if mutate == 'sigmoid_backward_gy' else g * y * (f32(1) - y))


# ---------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------
def _err_e(a):
    T = np.abs(100 * np.asarray(a, dtype=f64))
    with np.errstate(under='ignore'):
        return T, np.exp(-T), (2 * T + 2 * ULP_EXP) * U


def bound_h(a, lean=False, da=0.0):
    """|h - softplus(a)| for h = softplus100(a) (lean: softplus100_lean), a the float64 pre-activation of the reference
    and da what the kernel's own pre-activation may differ from it by (|d softplus / d a| <= 1).

    e = exp2(-|a c32|): the product's rounding moves the exponent by |100 a| U, the constant's by as much, v_exp_f32 adds
    1 ulp: relative error de = (2 |100 a| + 2) U, and TINY where e is below the normal numbers.
    series (e < 1e-4): l = e (1 - e / 2): two roundings (the 0.5 e is exact) and the truncation e^2 / 3 < 0.06 U:
        dl = l (de + 2.1 U)
    log: 1 + e rounds by U absolutely (1 + e in [1, 2]) and d log(1 + e) <= d (1 + e); v_log_f32 1 ulp, ln 2 as an fp32
        constant and the product U each: dl = e de + U + 4 U l.  Where the true e is within de of 1e-4 a correct kernel may
        take either side of the select: the series' bound holds only where e (1 + de) < 1e-4.
    h = fma(0.01f, l, max(a, 0)): the constant's U on 0.01 l, one rounding of the result:
        dh = 0.01 (dl + U l) + U |h| + TINY
    Relative where a <= 0 through the series (h = 0.01 l), dominated by 0.01 U / h through the log; for a > 0 the last
    term is half an ulp of a.  lean adds the two differences its comment states."""
    a = np.asarray(a, dtype=f64)
    T, e, de = _err_e(a)
    l = np.log1p(e)
    dl = np.where(e * (1 + de) < f64(SERIES_BELOW), l * (de + 2.1 * U), e * de + U + (2 * ULP_LOG + 2) * U * l)
    dh = 0.01 * (dl + U * l) + U * np.abs(softplus64(a)) + TINY + da
    return dh + (LEAN_THRESHOLD + LEAN_SERIES if lean else 0.0)


def bound_s(a, lean=False, da=0.0):
    """|s - sigmoid(100 a)| for s = 1 - exp2(-c32 h), h the kernel's softplus.  1 - sigmoid = exp(-100 softplus(a)) =: v.
    The exponent 100 h is off by 100 dh (dh = bound_h without da), by 2 U relative (product and constant), v_exp_f32 adds
    1 ulp: dv = v (100 dh + 200 h U + 2 U); 1 - u rounds by at most U s.  A pre-activation off by da moves the sigmoid by
    100 s (1 - s) da.  ABSOLUTE accuracy only: where a < 0 and s is small, ds stays near 2 U = 2^-23 while s goes to 0.
    Over all a: ds <= 5.82 U (fp32, bf16x6), <= 6.41 U (bf16x3) -- S_MULTIPLE, asserted by the CPU test."""
    a = np.asarray(a, dtype=f64)
    s, v = sigmoid64(100 * a), sigmoid64(-100 * a)
    dv = v * (100 * bound_h(a, lean) + 200 * softplus64(a) * U + 2 * ULP_EXP * U)
    return dv + U * s + 100 * s * v * da


S_MULTIPLE = {False: 5.82, True: 6.41}


def bound_t(a, pbar, lean=False, da=0.0):
    """|t - 100 s (1 - s) p-bar| for t = 100 u p q-bar rcp(s), p = s, q-bar = s p-bar (one rounding), p-bar exact.
    Errors of u and of p, each at most ds = bound_s: 100 |p-bar| (s du + (1 - s) dp) <= 100 |p-bar| ds (where s rounds to
    0 the kernel gives 0 and the true term is below 100 |p-bar| ds as well).  Relative: q-bar U, v_rcp_f32 1 ulp, four
    products U each: 7 U |t|.  da moves s (1 - s) by at most 100 s (1 - s) da."""
    a, pbar = np.asarray(a, dtype=f64), np.abs(np.asarray(pbar, dtype=f64))
    s, v = sigmoid64(100 * a), sigmoid64(-100 * a)
    t = 100 * s * v * pbar
    return 100 * pbar * bound_s(a, lean) + (5 + 2 * ULP_RCP) * U * t + 100 * t * da + TINY


# A sum that the matrix unit forms in its accumulators (slot + bias: the only rounded routing step of the encoding
# probes).  The order of the partial sums and the rounding of a matrix instruction's accumulation are not stated to be
# round-to-nearest, so each accumulation step may cost a whole ulp of the sum: one step on the fp32 core (the product is
# exact), one per plane on the bf16 cores.
ACC_STEPS = {'fp32': 1, 'bf16x3': 2, 'bf16x6': 3}


def acc_rounding(total, core):
    return ACC_STEPS[core] * ulp32(total)


def bound_pe(ref):
    """A sine or cosine of sincosf against the float64 one: the argument 2^k x is exact, the result 4 ulp."""
    return ULP_SINCOS * ulp32(ref)


def bound_color_sigmoid(o, g):
    """-> (dy, d(g y (1 - y))).  E = __expf(-o): relative error dE = (2 |o| + 2) U; 1 + E and the division round by U each:
    dy = y ((1 - y) dE + 2 U) + TINY.  Backward from the stored y: 1 - y rounds by U (1 - y), two products:
    |g| (dy |1 - 2 y| + 3 U y (1 - y)) + TINY."""
    o, g = np.asarray(o, dtype=f64), np.abs(np.asarray(g, dtype=f64))
    y, v = sigmoid64(o), sigmoid64(-o)
    dE = (2 * np.abs(o) + 2 * ULP_EXP) * U
    dy = y * (v * dE + 2 * U) + TINY
    return dy, g * (dy * np.abs(1 - 2 * y) + 3 * U * y * v) + TINY


# ---------------------------------------------------------------------------
# softplus probe
# ---------------------------------------------------------------------------
WIDTH = 64
UNIT_CHANNEL = np.arange(WIDTH) % 3
UNIT_K = (np.arange(WIDTH) // 3) % 8
UNIT_SCALE = 2.0 ** -UNIT_K.astype(f64)
T_SERIES = -math.log(float(SERIES_BELOW))          # e = 1e-4                   |100 a| = 9.2103
T_ONE = 24 * math.log(2.0)                         # 1 + e rounds to 1          |100 a| = 16.636
T_SG = 25 * math.log(2.0)                          # a < 0: s rounds to 0       |100 a| = 17.329
T_THRESHOLD = 20.0
SWITCHES = collections.OrderedDict([('series', T_SERIES), ('one_plus_e', T_ONE), ('sg', T_SG), ('threshold', T_THRESHOLD)])
SUBNORMAL_T = (87.0, 126 * math.log(2.0), 88.0, 95.0, 149 * math.log(2.0), 104.0, 110.0, 150.0)


def _around(t):
    """The two grid values x (multiples of 2^-12, |x| <= 2) and the k for which 100 2^-k x lies on either side of t, at
    the finest scale that reaches t."""
    for k in range(7, -1, -1):
        x = t / 100 * 2.0 ** k
        if abs(x) <= 2 - GRID:
            lo = math.floor(x / GRID) * GRID
            return (lo, lo + GRID) if lo != x else (lo - GRID, lo + GRID)
    raise AssertionError(t)


def softplus_values():
    """-> (sorted x values, the special ones among them).  0 and both signs of the grid step; both sides of every switch
    and of the subnormal / underflow range of e, both signs; +-2 (100 a = +-200 at k = 0); a sweep of 257 values."""
    special = {0.0, GRID, -GRID, 2.0, -2.0}
    for t in list(SWITCHES.values()) + list(SUBNORMAL_T) + [18.0]:
        for sgn in (1, -1):
            special.update(_around(sgn * t))
    sweep = set(np.linspace(-2, 2, 257).tolist())
    return np.array(sorted(special | sweep)), np.array(sorted(special))


def softplus_points(vals):
    """x [n, 3]: every channel sees every value."""
    n = len(vals)
    i = np.arange(n)
    return np.stack([vals[i], vals[(i + n // 3) % n], vals[(i + 2 * n // 3) % n]], 1)


SP_VALUES, SP_SPECIAL = softplus_values()
SP_X = softplus_points(SP_VALUES)                         # [P, 3] float64, on the grid
# hot points of the double backward: every special value in channel 0 (the other two channels carry sweep values) and
# every 16th point
SP_HOT = np.array(sorted(set(np.nonzero(np.isin(SP_VALUES, SP_SPECIAL))[0][::2].tolist()) |
                         set(range(0, len(SP_VALUES), 16))))


def sp_preactivations(x):
    """a0 [P, 64] and a1 [P, 64] of points x [P, 3], float64 (exact)."""
    xc = np.asarray(x, dtype=f64)[:, UNIT_CHANNEL]
    return xc + 4.0, xc * UNIT_SCALE


def sp_state(sdf_row):
    """State dict of the softplus probe with the given sdf row [64]."""
    W0 = torch.zeros(WIDTH, 3)
    W0[torch.arange(WIDTH), torch.from_numpy(UNIT_CHANNEL)] = 1.0
    scale = torch.from_numpy(UNIT_SCALE).float()
    W2 = torch.cat([torch.as_tensor(sdf_row, dtype=torch.float32)[None], torch.eye(WIDTH)], 0)
    return {'lin0.weight': W0, 'lin0.bias': torch.full((WIDTH,), 4.0), 'lin1.weight': torch.diag(scale),
            'lin1.bias': -4.0 * scale, 'lin2.weight': W2, 'lin2.bias': torch.zeros(1 + WIDTH)}


def one_hot(j, n=WIDTH):
    v = np.zeros(n, dtype=np.float32)
    v[j] = 1.0
    return v


ONE_HOT_UNITS = tuple(range(0, 24, 3))             # channel 0, k = 0 .. 7
THREE_HOT = tuple((3 * m, 3 * m + 1, 3 * m + 2) for m in (0, 3, 5, 7, 9, 12, 14, 18))      # one unit per channel; k = m % 8


def three_hot(units):
    v = np.zeros(WIDTH, dtype=np.float32)
    v[list(units)] = 1.0
    return v


def sp_certificate():
    """Reasons why the routing of the softplus probe is NOT exact (empty: it is): a0 and a1 recomputed in numpy fp32
    equal the float64 values, a0 needs 15 bits at most (two bf16 planes hold it), the pass-through layer returns a0 itself
    with u = 0 exactly, and the products 2^-k a0, the bias sum and the output layer's 1 * h are exact by construction."""
    why = []
    x32 = SP_X.astype(f32)
    if not np.array_equal(x32.astype(f64), SP_X) or np.abs(SP_X).max() > 2 or not np.array_equal(SP_X / GRID, np.round(SP_X / GRID)):
        why.append('x is not on the grid')
    a0, a1 = sp_preactivations(SP_X)
    a0_32 = x32[:, UNIT_CHANNEL] * f32(1) + f32(4)
    scale32 = UNIT_SCALE.astype(f32)
    a1_32 = a0_32 * scale32 + f32(-4) * scale32
    if not np.array_equal(a0_32.astype(f64), a0) or not np.array_equal(a1_32.astype(f64), a1):
        why.append('a0 or a1 is rounded in fp32')
    if a0.min() < 2 or a0.max() > 6 or not np.array_equal(a0 * 2.0 ** 12, np.round(a0 * 2.0 ** 12)):
        why.append('a0 is not 15 bits in [2, 6]')
    bf = torch.from_numpy(a0_32)
    p1 = bf.bfloat16().float()
    if not torch.equal(p1 + (bf - p1).bfloat16().float(), bf):
        why.append('a0 does not fit two bf16 planes')
    h0, _ = softplus_restated(a0_32)
    u0, s0 = sigmoid_restated(h0)
    if not np.array_equal(h0, a0_32) or u0.any() or not (s0 == 1).all():
        why.append('layer 0 is no pass-through')
    return why


# ---------------------------------------------------------------------------
# positional-encoding probe (SDF network)
# ---------------------------------------------------------------------------
PE_MULTIRES = (6, 7, 1)
PE_WIDTH = 48
PE_BIAS = 1.25
PE_K = 6                             # the probe layer behind the selector: a1 = 2^-6 slot


def pe_slots(multires):
    return 3 + 6 * multires


def pe_weight(j):
    return 0.5 if j < 3 else 1.0


def pe_points(multires):
    """x [96, 3] on multiples of 2^-12 in [-1.5, 1.5]: the origin, the axes, values where 2^k x is next to a multiple of
    pi / 2 at the top octave, a sweep."""
    top = 2.0 ** (multires - 1)
    near = [round(n * math.pi / 2 / top / GRID) * GRID for n in range(1, 200) if n * math.pi / 2 / top <= 1.5]
    near = near[:: max(1, len(near) // 12)][:12]
    rows = [(0, 0, 0), (1, 0, 0), (0, -1, 0), (0, 0, 1.5), (-1.5, 0, 0)]
    for i, v in enumerate(near):
        rows.append((v, -near[(i + 5) % len(near)], near[(i + 7) % len(near)] - GRID))
    sweep = np.round(np.linspace(-1.5, 1.5, 96 - len(rows)) / GRID) * GRID
    n = len(sweep)
    for i in range(n):
        rows.append((sweep[i], sweep[(i + n // 3) % n], sweep[(i * 7 + 3) % n]))
    return np.array(rows, dtype=f64)


PE_X = {m: pe_points(m) for m in PE_MULTIRES}
PE_HOT = np.arange(0, 96, 4)


def pe_state(multires, sdf_row, probe):
    """probe False: layer 1 the identity; True: diag(2^-6) with bias -1.25 2^-6."""
    n = pe_slots(multires)
    W0 = torch.zeros(PE_WIDTH, n)
    for j in range(n):
        W0[j, j] = pe_weight(j)
    sc = 2.0 ** -PE_K if probe else 1.0
    W2 = torch.cat([torch.as_tensor(sdf_row, dtype=torch.float32)[None], torch.eye(PE_WIDTH)], 0)
    return {'lin0.weight': W0, 'lin0.bias': torch.full((PE_WIDTH,), PE_BIAS), 'lin1.weight': sc * torch.eye(PE_WIDTH),
            'lin1.bias': torch.full((PE_WIDTH,), -PE_BIAS * sc if probe else 0.0), 'lin2.weight': W2,
            'lin2.bias': torch.zeros(1 + PE_WIDTH)}


PeSlot = collections.namedtuple('PeSlot', 'j val dval c a0 val32 dval32 a0_32')


def pe_reference(multires, j, mutate=None):
    """Slot j of the points PE_X[multires]: float64 val, dval, channel and a0 = w val + 1.25; the fp32 restatement of the
    same."""
    x = PE_X[multires]
    val, dval, c = pe_slot_restated(j, x)
    v32, d32, c32 = pe_slot_restated(j, x.astype(f32), mutate)
    w = pe_weight(j)
    a0 = w * val + PE_BIAS
    a0_32 = r32(v32.astype(f64) * w + PE_BIAS)
    return PeSlot(j, val, dval, c, a0, v32, d32, a0_32), c32


def pe_da0(s, core):
    """What the kernel's a0 may differ from the reference's by: nothing for a raw coordinate (x / 2 + 1.25 is exact in 14
    bits); else 4 ulp of the sine, the accumulation of slot + 1.25, and on bf16x3 the slot through two planes."""
    if s.j < 3:
        return np.zeros_like(s.a0)
    return bound_pe(s.val) + acc_rounding(s.a0, core) + (PLANE2 * np.abs(s.val) if core == 'bf16x3' else 0.0)


def pe_certificate(multires):
    """Reasons why the routing of the encoding probe is NOT what it claims: x on the grid, 2^k x exact in fp32, every a0
    above 0.2 and a pass-through with s = 1 exactly, a0 - (w slot + 1.25) bounded by the single rounding."""
    why = []
    x = PE_X[multires]
    if np.abs(x).max() > 1.5 or not np.array_equal(x / GRID, np.round(x / GRID)):
        why.append('x is not on the grid')
    top = f32(2.0 ** (multires - 1))
    if not np.array_equal((x.astype(f32) * top).astype(f64), x * 2.0 ** (multires - 1)):
        why.append('2^k x is rounded')
    for j in range(pe_slots(multires)):
        s, _ = pe_reference(multires, j)
        if s.a0_32.min() <= 0.2:
            why.append('slot %d: a0 = %g' % (j, s.a0_32.min()))
        h, _ = softplus_restated(s.a0_32)
        u, sg = sigmoid_restated(h)
        if not np.array_equal(h, s.a0_32) or not (sg == 1).all():       # (u <= exp(-25) is not 0, but 1 - u rounds to 1)
            why.append('slot %d is no pass-through' % j)
        if (np.abs(s.a0_32.astype(f64) - s.a0) > pe_da0(s, 'fp32')).any():
            why.append('slot %d: a0 is off by more than its rounding' % j)
        if j < 3 and not np.array_equal(s.a0_32.astype(f64), s.a0):
            why.append('slot %d: a raw coordinate is rounded' % j)
    return why


# ---------------------------------------------------------------------------
# colour probes
# ---------------------------------------------------------------------------
COLOR_P, COLOR_SPR, COLOR_F, COLOR_BIAS = 217, 7, 16, 2.0
VIEW_CASES = collections.OrderedDict((('%s_m%d' % (mode, m)), (mode, m)) for mode in ('idr', 'nerf') for m in (4, 2))


def view_lead(mode, m):
    return (9 if mode == 'idr' else 3) + 6 * m


def view_states(mode, m):
    return -(-view_lead(mode, m) // 3)


def view_inputs(m):
    """points, normals [217, 3] and one direction per ray [31, 3], all on multiples of 2^-12 in [-1.5, 1.5]; the
    directions hold the axes, the origin, values next to multiples of pi / 2 at the top octave and a sweep."""
    g = np.random.RandomState(7)
    pts = g.randint(-6144, 6145, (COLOR_P, 3)) * GRID
    nrm = g.randint(-6144, 6145, (COLOR_P, 3)) * GRID
    n_rays = COLOR_P // COLOR_SPR
    top = 2.0 ** (m - 1)
    rows = [(0, 0, 0), (1, 0, 0), (0, -1, 0), (0, 0, 1)]
    near = [round(n * math.pi / 2 / top / GRID) * GRID for n in range(1, 40) if n * math.pi / 2 / top <= 1.5]
    for i in range(6):
        rows.append((near[i % len(near)], -near[(i + 2) % len(near)], near[(i + 4) % len(near)] + GRID))
    sweep = np.round(np.linspace(-1.5, 1.5, n_rays - len(rows)) / GRID) * GRID
    n = len(sweep)
    for i in range(n):
        rows.append((sweep[i], sweep[(i + n // 3) % n], sweep[(5 * i + 2) % n]))
    return pts, nrm, np.array(rows, dtype=f64)


def view_state(mode, m, st):
    """Hidden unit i < lead: relu(column i + 2); output row r picks unit 3 st + r (none beyond the lead)."""
    lead = view_lead(mode, m)
    W0 = torch.zeros(WIDTH, lead + COLOR_F)
    for i in range(lead):
        W0[i, i] = 1.0
    W1 = torch.zeros(3, WIDTH)
    for r in range(3):
        if 3 * st + r < lead:
            W1[r, 3 * st + r] = 1.0
    return {'lin0.weight': W0, 'lin0.bias': torch.full((WIDTH,), COLOR_BIAS), 'lin1.weight': W1, 'lin1.bias': torch.zeros(3)}


VIEW_G = np.array([1.0, -2.0, 0.5])           # upstream gradient of the three colour rows


def view_columns(mode, m, mutate=None):
    """Every lead column at every point as [217, lead] arrays: float64 value, fp32 restatement, float64 and restated
    pre-activation, the bound of the value itself (0: an exact column), and n0, the first normal column (None for nerf)."""
    pts, nrm, dirs = view_inputs(m)
    ray = np.arange(COLOR_P) // COLOR_SPR
    v = dirs[ray]
    cols, cols32, bnd = [], [], []
    if mode == 'idr':
        for c in range(3):
            cols.append(pts[:, c]); cols32.append(pts[:, c].astype(f32)); bnd.append(np.zeros(COLOR_P))
    for j in range(3 + 6 * m):
        val = pe_slot_restated(j, v)[0]
        cols.append(val)
        cols32.append(pe_slot_restated(j, v.astype(f32), mutate)[0])
        bnd.append(bound_pe(val) if j >= 3 else np.zeros(COLOR_P))
    n0 = None
    if mode == 'idr':
        n0 = len(cols)
        for c in range(3):
            cols.append(nrm[:, c]); cols32.append(nrm[:, c].astype(f32)); bnd.append(np.zeros(COLOR_P))
    val, val32, bnd = np.stack(cols, 1), np.stack(cols32, 1), np.stack(bnd, 1)
    pre, pre32 = val + COLOR_BIAS, r32(val32.astype(f64) + COLOR_BIAS)
    return val, val32, pre, pre32, bnd, n0


def view_bound(val, pre, bnd, core):
    """Bound of rgb = column + 2: exact columns 0 (14 bits, any order); else the sine's 4 ulp, the accumulation of slot
    + 2 and on bf16x3 the slot through two planes."""
    return np.where(bnd > 0, bnd + acc_rounding(pre, core) + (PLANE2 * np.abs(val) if core == 'bf16x3' else 0.0), 0.0)


def view_g_nrm(mode, m, st, mutate=None):
    """d <VIEW_G, rgb> / d normal [3] (the same at every point) for state st: the gradient of the lead columns is
    VIEW_G[r] at column 3 st + r (every pre-activation is positive); the normal's three columns of it."""
    lead = view_lead(mode, m)
    g = np.zeros(lead + 4)
    for r in range(3):
        if 3 * st + r < lead:
            g[3 * st + r] = VIEW_G[r]
    n0 = 6 + 6 * m + (1 if mutate == 'normal_shifted' else 0)
    return g[n0:n0 + 3]


def view_certificate(mode, m):
    why = []
    val, val32, pre, pre32, bnd, n0 = view_columns(mode, m)
    if pre32.min() <= 0:
        why.append('a pre-activation is not positive')
    exact = bnd == 0
    if not np.array_equal(pre32[exact].astype(f64), pre[exact]):
        why.append('an exact column is rounded')
    if (np.abs(pre32.astype(f64) - pre) > view_bound(val, pre, bnd, 'fp32')).any():
        why.append('a pre-activation is off by more than its bound')
    return why


SIG_SPECIAL = (0.0, 2.0 ** -20, -2.0 ** -20, 88.0, -88.0, 89.0, -89.0, 110.0, -110.0)


def sigmoid_inputs():
    """feat [n, 16] with the o values in columns 0 .. 2 (every column sees every value) and the upstream gradient [n, 3]."""
    vals = np.array(sorted(set(SIG_SPECIAL) | set(np.linspace(-20, 20, 161).tolist())))
    n = len(vals)
    i = np.arange(n)
    o = np.stack([vals[i], vals[(i + n // 3) % n], vals[(i + 2 * n // 3) % n]], 1)
    feat = np.zeros((n, COLOR_F))
    feat[:, :3] = o
    return feat, o, np.tile(VIEW_G, (n, 1))


def sigmoid_state():
    """nerf, multires_view 0: unit 2 r = relu(f_r), unit 2 r + 1 = relu(-f_r), row r = unit 2 r - unit 2 r + 1 = f_r."""
    W0 = torch.zeros(WIDTH, 3 + COLOR_F)
    W1 = torch.zeros(3, WIDTH)
    for r in range(3):
        W0[2 * r, 3 + r], W0[2 * r + 1, 3 + r] = 1.0, -1.0
        W1[r, 2 * r], W1[r, 2 * r + 1] = 1.0, -1.0
    return {'lin0.weight': W0, 'lin0.bias': torch.zeros(WIDTH), 'lin1.weight': W1, 'lin1.bias': torch.zeros(3)}


def sigmoid_certificate():
    """o is exact through two bf16 planes and the routing relu(f) - relu(-f) gives f back."""
    feat, o, g = sigmoid_inputs()
    t = torch.from_numpy(o).float()
    p1 = t.bfloat16().float()
    why = []
    if not torch.equal(t.double(), torch.from_numpy(o)) or not torch.equal(p1 + (t - p1).bfloat16().float(), t):
        why.append('o does not fit two bf16 planes')
    o32 = o.astype(f32)
    if not np.array_equal(np.maximum(o32, 0) - np.maximum(-o32, 0), o32):
        why.append('the routing does not return f')
    return why


_CERT = {}


def certificate(kind, *args):
    """The certificate of a probe, computed once: 'softplus', ('pe', multires), ('view', mode, m), 'sigmoid'."""
    key = (kind,) + args
    if key not in _CERT:
        _CERT[key] = {'softplus': sp_certificate, 'pe': pe_certificate, 'view': view_certificate,
                      'sigmoid': sigmoid_certificate}[kind](*args)
    return _CERT[key]
