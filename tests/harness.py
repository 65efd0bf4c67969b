"""The harness of the tests that drive a whole MonoSDFNetwork: build the model, make the oracle's state, run one pass,
compare parameter gradients, record and compare a training step.  Plain functions and context managers (no fixtures);
seeds, sizes, case tables and the `test` / `case` / `key` strings of every comparison stay with the tests."""
import contextlib
from unittest import mock

import torch

from helpers import TOL, check, rel_err

# switched(obj, name, value) is unittest.mock.patch.object: obj.name = value in the block, what it was on every way out
switched = mock.patch.object


def build_model(conf, state=None, training=True, device='cuda', precision=None, if_hdr=False):
    """MonoSDFNetwork(conf) with `state` loaded (load_state_dict copies: the model never aliases `state`; None keeps the
    random initialisation), then train(training), the device (None: the CPU) and the matrix core (None: the default)."""
    from monosdf_amd.conf import ConfigTree
    from monosdf_amd.model.network import MonoSDFNetwork
    m = MonoSDFNetwork(ConfigTree.from_dict(conf), if_hdr=if_hdr)
    if state is not None:
        m.load_state_dict(state, strict=True)
    m.train(training)
    m = m if device is None else m.to(device)
    return m if precision is None else m.set_precision(precision)


def case_model(case, training=None, precision=None, device='cuda'):
    """build_model for a helpers.Case: its conf, state and if_hdr, its own training mode unless one is given."""
    return build_model(case.conf, case.state, case.training if training is None else training, device, precision,
                       case.spec.get('if_hdr', False))


def oracle_state(state, grad=False):
    """Clones of `state` for the oracle; grad: every floating-point tensor requires a gradient (never the `offsets`)."""
    return {k: v.clone().requires_grad_(grad and v.dtype.is_floating_point) for k, v in state.items()}


def to_device(d, device='cuda'):
    return {k: v.to(device) for k, v in d.items()}


def run_pass(model, inputs, indices, noise=None, pixel=True, loss=None):
    """One forward pass on device copies of the inputs, the indices and the injected draws (None: the model draws its own;
    a training pass is never given an empty set); loss: a function of the output dict whose value is backpropagated.
    Gradients accumulate: no zero_grad here."""
    if model.training and noise is not None:
        assert len(noise) > 0, 'a training pass with an empty set of injected draws'
    model._noise = to_device(noise) if noise else None
    out = model(to_device(inputs), indices.cuda(), if_pixel_input=pixel)
    if loss is not None:
        loss(out).backward()
    return out


def oracle_grads(st, ref):
    """Gradients of the probe loss of the oracle's outputs `ref` by the leaves of `st`: name -> tensor, None if unused."""
    from oracle import monosdf_oracle as mo
    names = [k for k, v in st.items() if v.requires_grad]
    return dict(zip(names, torch.autograd.grad(mo.probe_loss(ref), [st[k] for k in names], allow_unused=True)))


def check_param_grads(errlog, test, case, model, ref, names=None, allow_missing=False, transform=None, default=TOL):
    """check(errlog, test, case, <name>, rel_err(<parameter>.grad, ref[<name>])) for the parameters `names`: None -- every
    one whose reference is not None, in named_parameters() order; a string -- those of them with that prefix; a list --
    exactly these, in its order.  A parameter without a gradient fails, unless allow_missing (then it is left out).
    transform(name, grad, ref) -> (grad, ref) is applied before the comparison."""
    params = dict(model.named_parameters())
    if names is None or isinstance(names, str):
        names = [n for n in params if n.startswith(names or '') and ref.get(n) is not None]
    for n in names:
        g, r = params[n].grad, ref[n]
        if g is None and allow_missing:
            continue
        assert g is not None, (test, case, n, 'no gradient')
        check(errlog, test, case, n, rel_err(*(transform(n, g, r) if transform else (g, r))), default)


def step_record(model, out, loss=None, keys=None):
    """One training step as a record: detached clones of out[keys] (None: all), of the loss and of every parameter
    gradient there is, the sampler's rounds and repeated passes."""
    return {'out': {k: out[k].detach().clone() for k in (out if keys is None else keys)},
            'loss': None if loss is None else loss.detach().clone(),
            'grads': {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None},
            'rounds': model.ray_sampler.last_rounds, 'repeats': model.ray_sampler.stats['repeats']}


def assert_same_step(a, b):
    """Two step records hold the same outputs, loss and parameter gradients: same keys, bit for bit."""
    assert sorted(a['out']) == sorted(b['out']) and sorted(a['grads']) == sorted(b['grads'])
    assert (a['loss'] is None) == (b['loss'] is None) and (a['loss'] is None or torch.equal(a['loss'], b['loss']))
    for part in ('out', 'grads'):
        for k in a[part]:
            assert torch.equal(a[part][k], b[part][k]), (part, k)


@contextlib.contextmanager
def shared_weights(net, device):
    """net.share(device) inside the block, net.unshare() on every way out."""
    net.share(device)
    try:
        yield
    finally:
        net.unshare()
