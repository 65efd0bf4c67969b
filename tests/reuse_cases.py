"""The networks, states, rays and draws that test_gpu_sdf_reuse.py and test_gpu_fg_dispatch_order.py share."""
import functools

from harness import build_model
from oracle import config, synth

NETS = {'w64_skip': (64, True), 'w64_noskip': (64, False), 'w256_skip': (256, True)}       # width, skip layer
N_EVAL, N_EXTRA = 128, 32
OUT_KEYS = ('rgb', 'rgb_values', 'depth_values', 'z_vals', 'depth_vals', 'sdf', 'weights', 'grad_theta',
            'grad_theta_nei', 'normal_map')


@functools.lru_cache(maxsize=None)
def conf_state(net, beta):
    width, skip = NETS[net]
    conf = config.mlp_config(width, 8, beta=beta)
    if not skip:
        conf['implicit_network']['skip_in'] = []
    return conf, synth.make_state(conf, seed=5, jitter=0.3)


def model(net, beta):
    return build_model(*conf_state(net, beta))


@functools.lru_cache(maxsize=None)
def inputs(net, n, beta, table):
    conf, _ = conf_state(net, beta)
    # the rays of the sharp state (`table`) are seeds at which the oracle's sampler needs exactly two rounds for every
    # (net, n) of both files, the first round's largest beta 1.8 to 4 times the target (with most seeds the 256-wide state
    # converges in one round for 2 or 3 rays)
    rays = synth.make_rays(n, seed=(50 if table else 3) + n, random_pose=True)
    noise = synth.make_noise_table(conf, n, seed=7) if table else synth.make_noise(conf, n, N_EVAL, seed=7)
    return rays, noise
