"""Shared helpers for the parity tests (load a golden case, rebuild its inputs, the error measure and its bars).  What a
test does with a whole MonoSDFNetwork -- build it, make the oracle's state, run a pass, compare parameter gradients or
whole training steps -- is in the harness next to this file, tests/harness.py."""
import ast
import os

import numpy as np
import torch

from oracle import config, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def conf_from_spec(spec):
    kind = spec['kind']
    if kind == 'mlp':
        c = config.mlp_config(spec['width'], spec.get('depth', 8), spec.get('beta', 0.1))
    elif kind == 'gridless':
        c = config.gridless_config(spec['width'], spec.get('depth', 8), spec.get('beta', 0.1))
    else:
        c = config.grid_config(spec['width'], spec.get('beta', 0.1), spec.get('num_levels', 16),
                               spec.get('level_dim', 2), spec.get('logmap', 19),
                               spec.get('base_size', 16), spec.get('end_size', 2048))
    if spec.get('white_bkgd', False):
        c['white_bkgd'] = True
    if spec.get('per_image_code', False):
        c['rendering_network']['per_image_code'] = True
    if spec.get('render_mode', 'idr') == 'nerf':
        c['rendering_network']['mode'] = 'nerf'
        c['rendering_network']['d_in'] = 3
    return c


class Case:
    """One tests/golden/<name>.npz: spec, rebuilt conf/state, recorded inputs/noise/outputs."""

    def __init__(self, name):
        z = np.load(os.path.join(GOLDEN, name + '.npz'))
        self.name = name
        self.spec = dict(ast.literal_eval(bytes(z['spec']).decode()))
        self.conf = conf_from_spec(self.spec)
        self.state = synth.make_state(self.conf, seed=self.spec.get('weight_seed', 0),
                                      jitter=self.spec['jitter'], sdf_scale=self.spec.get('sdf_scale', 1.0))
        self.rounds = int(z['rounds'])
        self.indices = torch.from_numpy(z['indices'])
        self.training = self.spec['training']
        self.pixel = not self.spec.get('image_mode', False)
        pick = lambda p: {k[len(p):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(p)}
        self.inputs, self.noise, self.out = pick('in.'), pick('noise.'), pick('out.')
        self.grads, self.gdig = pick('grad.'), pick('gdig.')
        # fingerprints of table gradients too large to commit (synth.table_fingerprint): {param: {field: array}}
        self.gtab = {}
        for k, v in pick('gtab.').items():
            n, field = k.rsplit('.', 1)
            self.gtab.setdefault(n, {})[field] = v
        self.loss = float(z['loss']) if 'loss' in z.files else None
        self.converged = bool(z['converged']) if 'converged' in z.files else None
        # per-round intermediates recorded inside the reference's sampler (cases generated with trace=True)
        self.trace = []
        while ('smp.r%d.z' % len(self.trace)) in z.files:
            r = len(self.trace)
            self.trace.append(pick('smp.r%d.' % r))


def digest(t):
    a = t.detach().double().flatten().cpu()
    idx = torch.linspace(0, a.numel() - 1, min(16, a.numel())).long()
    return torch.cat([torch.stack([a.sum(), a.abs().sum(), (a * a).sum()]), a[idx]])


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


# full-forward cases (oracle/make_golden.py); the other fixtures have generators and tests of their own
_OTHER = ('stages', 'loss_', 'volume_', 'traj_', 'plumbing_', 'raytable_')
ALL_CASES = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith('.npz') and not f.startswith(_OTHER))


# ---- tolerances -----------------------------------------------------------------------------------------------
# Every GPU parity comparison is held to TOL, 1e-4 of the reference tensor's max-abs (BASELINE.json north_star:
# "within 1e-4 rel fp32") unless tests/golden/tolerances.json lists it.  That table is FROZEN, reviewed data: it changes
# only through scripts/parity_table.py (`tighten` lowers entries, `add` accepts a new one only within 2 x the reference's
# own deviation on that tensor -- profiles/r03_reference_sensitivity.json -- or with a hand-written cause);
# tests/test_host_logic.py enforces the rule on the CPU.  MSDF_PARITY_MEASURE=1 only records the errors.
TOL = 1e-4
_TABLE = None


def tolerance(test, case, key, default=TOL):
    global _TABLE
    if _TABLE is None:
        import json
        path = os.path.join(GOLDEN, 'tolerances.json')
        _TABLE = json.load(open(path))['tolerances'] if os.path.exists(path) else {}
    ent = _TABLE.get('%s|%s|%s' % (test, case, key))
    if ent is None and '.bf16x6' in test:
        # the bf16x6 core is held to the fp32 core's rows (a row of its own needs a hand-written cause)
        ent = _TABLE.get('%s|%s|%s' % (test.replace('.bf16x6', '.fp32'), case, key)) or \
            _TABLE.get('%s|%s|%s' % (test.replace('.bf16x6', ''), case, key))
    return default if ent is None else float(ent['tol'])


def check(errlog, test, case, key, err, default=TOL):
    tol = tolerance(test, case, key, default)
    errlog(test, case, key, err, tol)
    if os.environ.get('MSDF_PARITY_MEASURE') == '1':
        return
    assert err <= tol, (test, case, key, err, tol)


def hash_table_gradients(emb, offs, S, H, x, grad, grad2, gg, forms, pitch=0, pad=0.0, prefill=None, guard=0):
    """The hash grid's table-gradient entry points through raw ctypes: the forward for dy_dx, then every form named in
    `forms`, each into a fresh buffer (zeros; NaN for the "=" forms 'fused_out' and 'node'), returned by name.  'atomic' /
    'ws': msdf_hash_encode_backward / _ws of `grad` (also '<form>_inputs'); 'atomic_second' / 'ws_second': the second
    backward of (`grad2`, gg) (also '<form>_grad'); 'fused' / 'fused_out': both terms; 'node': msdf_hash_node_scatter,
    both terms, "=".  Also 'dy_dx', 'workspace', 'nbytes'.
    pitch > 0: 'node' reads its two operands as point-major rows [B, pitch] (level l, channel c at column l C + c), the
    columns from L C on filled with `pad`.  prefill: what the "+=" forms start from instead of zeros ([n, C]; the "="
    forms ignore it).  guard > 0: every buffer has that many rows after the table, filled with 1234.5, returned as
    '<form>_guard' (the table itself is r[form], [n, C], as without)."""
    from monosdf_amd import _lib
    P, st = _lib.ptr, _lib.stream_ptr()
    (L, B, C), n = grad.shape, emb.shape[0]
    dy = torch.empty(B, L * 3 * C, device='cuda')
    out = torch.empty(L, B, C, device='cuda')
    _lib.call('msdf_hash_encode_forward', P(x), P(emb), P(offs), P(out), B, 3, C, L, S, H, 1, P(dy), st)
    nbytes = _lib.load().msdf_hash_scatter_workspace_bytes(B, C, L, n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    r = {'dy_dx': dy, 'workspace': ws, 'nbytes': nbytes}

    def rows(t):                         # [L, B, C] -> [B, pitch]
        m = torch.full((B, pitch), float(pad), device='cuda')
        m[:, :L * C] = t.permute(1, 0, 2).reshape(B, L * C)
        return m.contiguous()

    for f in forms:
        buf = torch.empty(n + guard, C, device='cuda')
        if f in ('fused_out', 'node'):
            buf[:n] = float('nan')
        elif prefill is not None:
            buf[:n] = prefill
        else:
            buf[:n] = 0.0
        if guard:
            buf[n:] = 1234.5
            r[f + '_guard'] = buf[n:]
        t = r[f] = buf[:n]
        tail = (st,) if f.startswith('atomic') else (n, P(ws), nbytes, st)
        sfx = '' if f.startswith('atomic') else '_ws'
        if f in ('atomic', 'ws'):
            gi = r[f + '_inputs'] = torch.zeros_like(x)
            _lib.call('msdf_hash_encode_backward' + sfx, P(grad), P(x), P(emb), P(offs), P(t), B, 3, C, L, S, H, 1,
                      P(dy), P(gi), *tail)
        elif f in ('atomic_second', 'ws_second'):
            ggrad = r[f + '_grad'] = torch.zeros(L, B, C, device='cuda')
            _lib.call('msdf_hash_encode_second_backward' + sfx, P(grad2), P(x), P(emb), P(offs), B, 3, C, L, S, H, 1,
                      P(dy), P(gg), P(ggrad), P(t), *tail)
        elif f == 'node':
            g1, g2 = (rows(grad), rows(grad2)) if pitch else (grad, grad2)
            r['node_operands'] = (g1, g2)                 # alive until the caller has synchronised
            _lib.call('msdf_hash_node_scatter', P(g1), P(g2), pitch, P(x), P(offs), P(t), B, C, L, S, H, P(gg), *tail)
        else:
            _lib.call('msdf_hash_encode_backward_' + f, P(grad), P(grad2), P(x), P(offs), P(t), B, 3, C, L, S, H,
                      P(gg), *tail)
    return r
