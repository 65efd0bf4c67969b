"""The argument contract of the fused-MLP entry points (include/monosdf_hip.h): which code every refusal gives and in
which order the checks come.  Every call here is refused, or is the empty call P == 0, before anything is launched or any
pointer is read, so this runs without a GPU; the non-NULL pointers are host buffers nobody looks at."""
import ctypes as C

from monosdf_amd import _lib

OK, ARG, UNSUPPORTED = 0, 1, 3
F32, BF16X3, BF16X6 = 0, 1, 2
FORWARDS = ('msdf_sdf_forward', 'msdf_sdf_forward_if', 'msdf_sdf_forward_lm')
STRUCTS = {'msdf_sdf_fwd_grad': _lib.FgArgs, 'msdf_sdf_backward': _lib.BwArgs, 'msdf_color_forward': _lib.ColorFwdArgs,
           'msdf_color_backward': _lib.ColorBwdArgs}
ENTRY_POINTS = FORWARDS + tuple(STRUCTS)
AUX = ('msdf_sdf_forward_lm', 'msdf_sdf_fwd_grad', 'msdf_sdf_backward')      # the ones that take aux_C / aux_LC


def _plan(precision=F32, aux_tiles=2):
    p = _lib.Plan()
    p.n_layers, p.e_tiles, p.aux_tiles, p.precision = 2, 3, aux_tiles, precision
    return p


def test_mlp_entry_point_return_codes():
    lib = _lib.load()
    buf = (C.c_float * 16)()
    some = C.cast(buf, C.c_void_p)

    def status(name, plan, P=100, P_pad=128, aux=some, aux_C=0, aux_LC=0, dy_dx=None, r_aux=some, spr=1, args=True):
        pp = C.byref(plan) if plan is not None else None
        if name in FORWARDS:
            head = (pp, None, None, None, aux)
            tail = (P, 0.0, 1.0, None) + {'msdf_sdf_forward': (), 'msdf_sdf_forward_if': (None,)}.get(name, (None,))
            mid = (aux_C, aux_LC) if name == 'msdf_sdf_forward_lm' else ()
            return getattr(lib, name)(*(head + mid + tail), None)
        a = STRUCTS[name]()
        a.P, a.P_pad = P, P_pad
        if name in AUX:
            a.aux_C, a.aux_LC, a.dy_dx = aux_C, aux_LC, dy_dx
        if name == 'msdf_sdf_fwd_grad':
            a.aux, a.r_aux = aux, r_aux
        if name == 'msdf_color_forward':
            a.spr = spr
        return getattr(lib, name)(pp, C.byref(a) if args else None, None)

    def each(names, code, plan, **kw):
        for name in names:
            assert status(name, plan, **kw) == code, (name, kw, code)

    for prec in (F32, BF16X3, BF16X6, 7):
        plan = _plan(prec)
        # 1: no plan, no argument block, a negative point count (colour forward: samples per ray < 1)
        each(ENTRY_POINTS, ARG, None, P=0)
        each(STRUCTS, ARG, plan, P=0, args=False)
        each(ENTRY_POINTS, ARG, plan, P=-1)
        each(('msdf_color_forward',), ARG, plan, P=0, spr=0)
        # 2: no points -- OK before any pointer, the padded count, the layout or the precision is looked at
        each(ENTRY_POINTS, OK, plan, P=0, P_pad=7, aux=None, aux_C=5, r_aux=None)
        # 3: the padded point count (workspace rows): at least P, whole workgroups of 64 points
        each(STRUCTS, ARG, plan, P_pad=100)
        each(STRUCTS, ARG, plan, P_pad=64)
        each(STRUCTS, ARG, plan, P_pad=7, aux_C=2, aux_LC=32)
        # 4: a plan with extra input features and no features
        each(FORWARDS + ('msdf_sdf_fwd_grad',), ARG, plan, aux=None)
        # 5: the layout of the features: rows (0) or the encoder's level-major tensor with two channels
        for c, lc in ((1, 16), (4, 32), (8, 32), (-2, 32), (2, 0), (2, 31), (2, 34)):
            each(AUX, ARG, plan, aux_C=c, aux_LC=lc)
        # 6: the encoder's Jacobian goes with the level-major form (forward + gradient: and with r_aux)
        each(('msdf_sdf_fwd_grad', 'msdf_sdf_backward'), ARG, plan, dy_dx=some)
        each(('msdf_sdf_fwd_grad',), ARG, plan, aux_C=2, aux_LC=32, dy_dx=some, r_aux=None)
    # 7: the matrix core.  An unknown one is refused; the bf16 cores take rows only
    each(ENTRY_POINTS, ARG, _plan(7))
    each(AUX, ARG, _plan(7), aux_C=2, aux_LC=32)
    for prec in (BF16X3, BF16X6):
        each(AUX, UNSUPPORTED, _plan(prec), aux_C=2, aux_LC=32)
        each(('msdf_sdf_fwd_grad', 'msdf_sdf_backward'), UNSUPPORTED, _plan(prec), aux_C=2, aux_LC=32, dy_dx=some)


def test_pack_weights_return_codes():
    lib = _lib.load()
    assert lib.msdf_pack_weights(None, None, None, None, None, None, None, None) == ARG
    for prec in (F32, BF16X3, BF16X6, 7):
        for n in (0, -1, _lib.MAX_LAYERS + 1):
            plan = _plan(prec)
            plan.n_layers = n
            assert lib.msdf_pack_weights(C.byref(plan), None, None, None, None, None, None, None) == ARG
    assert lib.msdf_pack_weights(C.byref(_plan(7)), None, None, None, None, None, None, None) == ARG
