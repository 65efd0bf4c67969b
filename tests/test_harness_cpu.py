"""The harness of the model-level tests (tests/harness.py) on the CPU: each of its rules has a mutant that would quietly
weaken every test built on it -- a model that aliases the state, an oracle state without clones, a gradient comparison
that skips what it should report, a step comparison that overlooks a bit, a switch that stays flipped."""
import pytest
import torch

import harness
from oracle import config, synth


def _conf_state(kind):
    conf = config.mlp_config(64) if kind == 'mlp' else config.grid_config(64, 0.1, 4, 2, 11, 8, 64)
    return conf, synth.make_state(conf, seed=1, jitter=0.3)


@pytest.mark.parametrize('kind', ['mlp', 'grid'])
def test_model_and_oracle_state_are_copies_of_the_state(kind):
    conf, state = _conf_state(kind)
    for grad in (True, False):
        kept = harness.oracle_state(state, grad=grad)
        for k, v in kept.items():
            assert v.requires_grad == (grad and v.dtype.is_floating_point), k
            assert torch.equal(v, state[k]) and v.data_ptr() != state[k].data_ptr(), k
    assert kept.keys() == state.keys() and any(not v.dtype.is_floating_point for v in kept.values()) == (kind == 'grid')
    m = harness.build_model(conf, state, training=False, device=None, precision='bf16x6')
    assert not m.training and m.implicit_network.precision == m.rendering_network.precision == 'bf16x6'
    for n, p in m.named_parameters():
        assert torch.equal(p.detach().flatten(), state[n].flatten()), n     # (density.beta: [] from the state's [1])
        with torch.no_grad():
            p.add_(1.0)
        assert p.data_ptr() != state[n].data_ptr() and torch.equal(state[n], kept[n]), n
    m = harness.build_model(conf, device=None)
    assert m.training and m.implicit_network.precision is None and m.state_dict().keys() == state.keys()
    case = type('Case', (), dict(conf=conf, state=state, training=False, spec={'if_hdr': True}))
    m = harness.case_model(case, device=None)
    assert not m.training and m.if_hdr and harness.case_model(case, training=True, device=None).training


@pytest.fixture
def graded(monkeypatch):
    """A CPU model with hand-made gradients, references one part in 1e6 from them, and check_param_grads bound to them
    and to a list in the place of errlog (returned: the keys it logged); asserting, whatever the environment says."""
    monkeypatch.delenv('MSDF_PARITY_MEASURE', raising=False)
    m = harness.build_model(*_conf_state('mlp'), device=None)
    ref, rows = {}, []
    for i, (n, p) in enumerate(m.named_parameters()):
        p.grad = torch.full_like(p, float(i + 1))
        ref[n] = p.grad * (1.0 + 1e-6)

    def run(**kw):
        del rows[:]
        harness.check_param_grads(lambda *a: rows.append(a[:3]), 'harness_cpu', 'c', m, ref, **kw)
        assert all(r[:2] == ('harness_cpu', 'c') for r in rows)
        return [r[2] for r in rows]
    return dict(m.named_parameters()), ref, list(ref), run


def test_gradient_comparison_visits_the_referenced_parameters_in_order(graded):
    params, ref, names, run = graded
    assert run() == names and len(names) >= 20
    ref[names[2]] = None                        # a parameter the oracle's loss does not reach, and one it does not know
    del ref[names[5]]
    assert run() == [n for n in names if n not in (names[2], names[5])]
    colour = [n for n in names if n.startswith('rendering_network.')]
    ref[colour[1]] = None
    assert run(names='rendering_network.') == colour[:1] + colour[2:]
    assert run(names=[names[7], names[0], names[3]]) == [names[7], names[0], names[3]]


def test_gradient_comparison_refuses_an_error_and_a_missing_gradient_and_applies_the_transform(graded):
    params, ref, names, run = graded
    ref[names[4]] = ref[names[4]].clone()
    ref[names[4]][0] += 1.0                                          # row 0 is off ...
    with pytest.raises(AssertionError):
        run()
    assert run(transform=lambda n, g, r: (g[1:], r[1:]) if n == names[4] else (g, r)) == names    # ... and left out
    del ref[names[4]]
    params[names[1]].grad = None
    for kw in ({}, {'names': [names[1]]}):
        with pytest.raises(AssertionError, match='no gradient'):
            run(**kw)
    assert run(allow_missing=True) == [n for n in names if n not in (names[1], names[4])]


def _record():
    m = torch.nn.Linear(3, 2)
    m.ray_sampler = type('Sampler', (), {'last_rounds': 1, 'stats': {'repeats': 0}})
    m.weight.grad, m.bias.grad = torch.ones(2, 3), None              # a parameter without a gradient is not recorded
    out = {'a': torch.arange(4.0), 'b': torch.ones(2, 2), 'c': torch.zeros(1)}
    rec = harness.step_record(m, out, torch.tensor(0.5), keys=('a', 'b'))
    assert sorted(harness.step_record(m, out)['out']) == ['a', 'b', 'c'] and harness.step_record(m, out)['loss'] is None
    out['a'] += 1.0                                                  # the record holds clones
    m.weight.grad += 1.0
    assert torch.equal(rec['out']['a'], torch.arange(4.0)) and torch.equal(rec['grads']['weight'], torch.ones(2, 3))
    assert (sorted(rec['out']), sorted(rec['grads']), rec['rounds'], rec['repeats']) == (['a', 'b'], ['weight'], 1, 0)
    return rec


@pytest.mark.parametrize('change', ['bit', 'key'])
@pytest.mark.parametrize('where', ['out', 'loss', 'grads'])
def test_assert_same_step_sees_one_flipped_bit_and_a_one_sided_key(where, change):
    a, b = _record(), _record()
    harness.assert_same_step(a, b)
    if change == 'bit':
        t = b['loss'] if where == 'loss' else next(iter(b[where].values()))
        t.view(torch.int32).view(-1)[0] ^= 1
    elif where == 'loss':
        b['loss'] = None
    else:
        b[where]['extra'] = torch.zeros(1)
    for x, y in ((a, b), (b, a)):
        with pytest.raises(AssertionError):
            harness.assert_same_step(x, y)


def test_switched_and_shared_weights_undo_on_every_exit():
    class Net:
        FLAG, calls = 'was', []
        share = lambda self, device: self.calls.append(('share', device))
        unshare = lambda self: self.calls.append('unshare')
    for fail in (False, True):
        del Net.calls[:]
        try:
            with harness.switched(Net, 'FLAG', 'now'), harness.shared_weights(Net(), 'dev'):
                assert Net.FLAG == 'now' and Net.calls == [('share', 'dev')]
                if fail:
                    raise KeyError
        except KeyError:
            assert fail
        assert Net.FLAG == 'was' and Net.calls == [('share', 'dev'), 'unshare']
