"""Ray samplers (reference: code/model/ray_sampler.py).  ``UniformSampler.get_z_vals`` and
``ErrorBoundSampler.get_z_vals`` keep the reference's signatures; the algorithms run in csrc/sampler.hip
(one wave per ray) with the SDF evaluations done by the fused forward kernel.

The batch-global convergence test (``beta.max() > beta0``, reference ray_sampler.py:179) is evaluated on the
device: the kernels of a round return at once when the previous round did not ask for them, so the host may
enqueue rounds without reading the flags back (``speculate``), and only has to check afterwards that it
enqueued enough of them."""
import collections
import math

import torch

from .. import _lib


class RaySampler:
    def __init__(self, near, far):
        self.near, self.far = near, far


def _need_gpu(t):
    if not t.is_cuda:
        raise RuntimeError('monosdf_amd: the samplers run on the GPU only (no CPU fallback)')
    return t.detach().float().contiguous()


# -- what one sampler call points at: every pointer field of msdf_sampler_args_t, stated once -------------------------
# The sizes of a call: N rays, n_eval new samples per round, n_final importance samples, n_extra columns of the dense
# set, K = max_total_iters rounds at the most; S is the width of the final set (with near and far).
class _Sizes(collections.namedtuple('_Sizes', 'N n_eval n_final n_extra K training want_points')):
    S = property(lambda d: d.n_final + d.n_extra + 2)


_F32, _I32 = torch.float32, torch.int32
# buffers the call allocates: field -> (shape from the _Sizes, dtype); a shape of None: this call has no such buffer and
# the field is NULL
ALLOCATED = {
    'z': (lambda d: (d.N, d.n_eval * d.K), _F32),
    'sdf': (lambda d: (d.N, d.n_eval * d.K), _F32),
    'new_z': (lambda d: (d.N, d.n_eval), _F32),
    'new_pos': (lambda d: (d.N, d.n_eval), _I32),
    'pts': (lambda d: (d.N * d.n_eval, 3), _F32),
    'beta': (lambda d: (d.N,), _F32),
    'flags': (lambda d: (2 * d.K,), _I32),                # zeroed by msdf_sampler_init
    'final_z': (lambda d: (d.N, d.n_final), _F32),
    'z_out': (lambda d: (d.N, d.S), _F32),
    'z_eik': (lambda d: (d.N, 1), _F32),
    # the ray samples' points and, in training, the four eikonal points of every ray behind them
    'pts_out': (lambda d: (d.N * d.S + (4 * d.N if d.training else 0), 3) if d.want_points else None, _F32),
    'far_out': (lambda d: (d.N, 1), _F32),                # UniformSampler only
}
# inputs the caller supplies: the rays, beta0, the draws, the dense-set columns, the pass's SdfReuse, a round's SDF
# values
SUPPLIED = ('ray_o', 'ray_d', 'beta0', 'new_sdf', 'jitter', 'u_final', 'extra_idx', 'eik_idx', 'eik_u', 'eik_uniform',
            'nei_rand', 'row_map', 'h_saved')
# outputs of the kernels that only tests ask for
LEFT_NULL = ('dbg_dstar', 'dbg_err0', 'dbg_cdf', 'rounds_out')


class _SamplerCall(_lib.Binder):
    """The msdf_sampler_args_t of one call and every tensor whose address sits in it: they live as long as this does.
    A call is filled in stages: every pointer field starts out NULL, the scalars of a round 0, and bind() gives them
    their values as the call goes on."""

    def __init__(self, sizes, device, **scalars):
        self.sizes, self.device, self.stream = sizes, device, _lib.stream_ptr()
        super().__init__(_lib.SamplerArgs, N=sizes.N, n_eval=sizes.n_eval, n_final=sizes.n_final, n_extra=sizes.n_extra,
                         max_rounds=sizes.K, m_max=sizes.n_eval * sizes.K, training=int(sizes.training), M=0,
                         round_idx=0, eik_unit=0, **dict.fromkeys((*ALLOCATED, *SUPPLIED, *LEFT_NULL)), **scalars)

    def alloc(self, *names):
        """The call's own buffers, from the table, bound; returns them in the order asked for."""
        new = {}
        for name in names:
            shape, dtype = ALLOCATED[name]
            shape = shape(self.sizes)
            new[name] = None if shape is None else torch.empty(*shape, device=self.device, dtype=dtype)
        self.bind(**new)
        return list(new.values())

    def launch(self, entry):
        super().launch(entry, stream=self.stream)


class UniformSampler(RaySampler):
    """reference ray_sampler.py:16-83: N_samples equidistant depths between near and far (far = the exit of the
    cube [-R, R]^3 clipped to 2 R 1.75 with take_sphere_intersection, else that constant), stratified jitter in
    training mode.  Returns (z_vals [N, N_samples], near [N,1], far [N,1])."""

    def __init__(self, scene_bounding_sphere, near, N_samples, take_sphere_intersection=False, far=-1):
        super().__init__(near, 2.0 * scene_bounding_sphere * 1.75 if far == -1 else far)
        self.N_samples = N_samples
        self.scene_bounding_sphere = scene_bounding_sphere
        self.take_sphere_intersection = take_sphere_intersection

    def get_z_vals(self, ray_dirs, cam_loc, model, jitter=None):
        ray_dirs, cam_loc = _need_gpu(ray_dirs), _need_gpu(cam_loc)
        dev = ray_dirs.device
        N, n = ray_dirs.shape[0], self.N_samples
        if model.training and jitter is None:
            jitter = torch.rand(N, n, device=dev, dtype=torch.float32)
        # the first step of an error-bound call of one round with no final set: its n_eval samples are the result
        bound = float(self.scene_bounding_sphere) if self.take_sphere_intersection else 0.0
        call = _SamplerCall(_Sizes(N, n, 0, 0, 1, False, False), dev, near=float(self.near), far=float(self.far),
                            bound=bound, lemma=1.0, beta_iters=0, eps=0.0, add_tiny=0.0)
        call.bind(ray_o=cam_loc, ray_d=ray_dirs, jitter=None if jitter is None else _need_gpu(jitter))
        z, far = call.alloc('z', 'far_out')
        call.alloc('new_z', 'new_pos', 'pts', 'beta')        # msdf_sampler_init writes them too: not returned
        call.launch('msdf_sampler_init')
        return z, torch.full((N, 1), float(self.near), device=dev, dtype=torch.float32), far


class ErrorBoundSampler(RaySampler):
    def __init__(self, scene_bounding_sphere, near, N_samples, N_samples_eval, N_samples_extra, eps, beta_iters,
                 max_total_iters, inverse_sphere_bg=False, N_samples_inverse_sphere=0, add_tiny=1.0e-6):
        super().__init__(near, 2.0 * scene_bounding_sphere * 1.75)
        if inverse_sphere_bg:
            raise NotImplementedError('monosdf_amd: inverse_sphere_bg is not used by any conf of the reference fork')
        self.N_samples = N_samples
        self.N_samples_eval = N_samples_eval
        self.uniform_sampler = UniformSampler(scene_bounding_sphere, near, N_samples_eval,
                                              take_sphere_intersection=True)
        self.N_samples_extra = N_samples_extra
        self.eps = eps
        self.beta_iters = beta_iters
        self.max_total_iters = max_total_iters
        self.scene_bounding_sphere = scene_bounding_sphere
        self.add_tiny = add_tiny
        self._last_rounds = 0
        # rounds of the last HISTORY calls and the calls left in which all max_total_iters rounds are enqueued (see
        # guess_rounds) -- kept twice: [0] for this rank's own calls, [1] for the calls whose round decision was
        # all-reduced over a rank group (global_rounds).  The second one is a function of the all-reduced flags alone,
        # so it is the same on every rank of the group, and so is the number of rounds (= collectives) guessed from it
        self._hist = [[], []]
        self._miss = [0, 0]
        self._pending = None
        self._eval_columns = {}
        # speculation bookkeeping (bench.py reports it): calls, passes repeated because too few rounds were
        # enqueued, rounds enqueued beyond the ones that ran
        self.stats = {'calls': 0, 'repeats': 0, 'idle_rounds': 0}
        # a torch.distributed group (or True = the default group): the convergence test takes the maximum beta over
        # all ranks, so that a batch split over ranks runs the rounds the whole batch would run on one GPU
        # (SURVEY 8(e)); None = every rank decides for its own rays, as under the reference's DDP
        self.global_rounds = None
        # Lemma-2 constant, formed in fp32 like the reference does (ray_sampler.py:119)
        self._lemma = float(1.0 / (4.0 * torch.log(torch.tensor(self.eps + 1.0))))

    def get_z_vals(self, ray_dirs, cam_loc, model):
        z, z_eik, _ = self.sample(ray_dirs, cam_loc, model, want_points=False)
        return z, z_eik

    def get_error_bound(self, beta, model, sdf, z_vals, dists, d_star):
        """reference ray_sampler.py:264-272 (dists is z_vals' difference, recomputed in the kernel)."""
        z = _need_gpu(z_vals)
        N, M = z.shape
        sdf = _need_gpu(sdf).reshape(N, M)
        d_star = _need_gpu(d_star).reshape(N, M - 1)
        beta = _need_gpu(beta if torch.is_tensor(beta) else torch.tensor(beta, device=z.device)).reshape(-1)
        if beta.numel() not in (1, N):
            raise RuntimeError('monosdf_amd: beta must hold one value or one per ray')
        out = torch.empty(N, device=z.device, dtype=torch.float32)
        _lib.call('msdf_sampler_error_bound', _lib.ptr(z), _lib.ptr(sdf), _lib.ptr(d_star), _lib.ptr(beta),
                  int(beta.numel() == N and N > 1), N, M, _lib.ptr(out), _lib.stream_ptr())
        return out

    # -- the columns of the dense sample set that join the final set (ray_sampler.py:242-247) ------------------
    @staticmethod
    def column_slots(row0, n_eval):
        """The inverse of the first row of the extra_idx table: [n_eval] int32, entry c = the position of column c
        in row0, -1 for a column that is not in it.  None when row0 is not a set of distinct columns of the first
        round (then its points are not one saved row each)."""
        row0 = row0.reshape(-1).to(torch.int64)
        n = row0.numel()
        if n == 0 or int(row0.min()) < 0 or int(row0.max()) >= n_eval or torch.unique(row0).numel() != n:
            return None
        slots = torch.full((n_eval,), -1, dtype=torch.int32)
        slots[row0] = torch.arange(n, dtype=torch.int32)
        return slots

    def _extra_columns(self, training, noise, dev, want_slots=False):
        """(columns, slots).  columns: [max_total_iters, N_samples_extra] int64 on the device, row k-1 is used when k
        rounds ran.  Training: a random subset per size, drawn on the CPU generator as the reference does; eval: its
        linspace.  slots (want_slots): column_slots() of row 0 on the device, or None."""
        n_extra, n_eval, K = self.N_samples_extra, self.N_samples_eval, self.max_total_iters
        if n_extra <= 0:
            return torch.zeros(K, 1, device=dev, dtype=torch.int64), None
        if training:
            given = noise.get('extra_idx')
            if given is not None:
                given = given.to(device=dev, dtype=torch.int64)
                # a test's table, one row per possible size, or its draw for the size the loop will end with: the
                # same row for all sizes
                table = given.contiguous() if given.dim() == 2 else \
                    given.reshape(1, n_extra).expand(K, n_extra).contiguous()
                slots = self.column_slots(table[0].cpu(), n_eval) if want_slots else None
                return table, (slots.to(dev) if slots is not None else None)
            # the table and its slots in one pinned buffer: one copy to the device
            words = K * n_extra + (n_eval + 1) // 2
            host = torch.empty(words, dtype=torch.int64, pin_memory=True)
            table = host[:K * n_extra].view(K, n_extra)
            for k in range(K):
                table[k] = torch.randperm(n_eval * (k + 1))[:n_extra]
            host[K * n_extra:].view(torch.int32)[:n_eval] = self.column_slots(table[0], n_eval)
            on_dev = host.to(dev, non_blocking=True)
            return on_dev[:K * n_extra].view(K, n_extra), on_dev[K * n_extra:].view(torch.int32)[:n_eval]
        key = (str(dev), n_eval, K, n_extra)
        if key not in self._eval_columns:
            rows = [torch.linspace(0, n_eval * (k + 1) - 1, n_extra).long() for k in range(K)]
            slots = self.column_slots(rows[0], n_eval)
            self._eval_columns[key] = (torch.stack(rows).to(dev), slots.to(dev) if slots is not None else None)
        return self._eval_columns[key]

    @property
    def last_rounds(self):
        """Rounds the last call ran (waits for its flags if they have not been read back yet)."""
        self._resolve()
        return self._last_rounds

    @last_rounds.setter
    def last_rounds(self, value):
        self._resolve()
        self._last_rounds = int(value)

    def _resolve(self):
        """Read the flags of the last speculative call (copied to pinned memory behind the sampler kernels).
        Returns False if its last enqueued round asked for one more."""
        if self._pending is None:
            return True
        ev, host, k, which = self._pending
        self._pending = None
        ev.synchronize()
        ran = 1
        while ran <= k and int(host[2 * (ran - 1) + 1]):
            ran += 1
        if ran > k:
            self.stats['repeats'] += 1
            self._note_rounds(k + 1, which)
            self._miss[which] = self.HISTORY
            return False
        self.stats['idle_rounds'] += k - ran
        self._note_rounds(ran, which)
        return True

    def confirm(self):
        """After a speculative sample(): False if the last round that was enqueued asked for another one (the
        pass has to be repeated with more rounds); otherwise the result is exact, however many were enqueued.
        With max_total_iters rounds enqueued that cannot happen, and nothing is read back here."""
        if self._pending is None or self._pending[2] >= self.max_total_iters:
            return True
        return self._resolve()

    HISTORY = 32

    def _note_rounds(self, rounds, which=0):
        self._last_rounds = rounds
        self._hist[which] = (self._hist[which] + [rounds])[-self.HISTORY:]

    def guess_rounds(self):
        """Rounds to enqueue for the next call without reading a flag back.  An idle round costs three empty
        launches (~15 us), a round too few costs the whole forward pass again (~10 ms at 1024 rays), so the guess
        errs upwards: the most demanding of the last HISTORY calls, and all max_total_iters rounds for HISTORY calls
        after every miss (small beta: most steps need 2 rounds, one in seven needs 5 -- bench.py, sharp_state)."""
        which = 1 if self.global_rounds is not None else 0
        if self._miss[which] > 0:
            self._miss[which] -= 1
            return self.max_total_iters
        return max(self._hist[which]) if self._hist[which] else 1

    @staticmethod
    def _draws(noise, d, device):
        """The random numbers of a training call: (name -> fp32 tensor, whether 'eik_uniform' is still U[0,1)).
        ONE launch for every draw of the call: stratified jitter, inverse-CDF u, neighbour jitter, the eikonal sample's
        column ('eik_u'; floor(u S) in the finish kernel: the reference's randint, ray_sampler.py:254) and the uniform
        eikonal points ((2u - 1) R in the finish kernel: the reference's uniform_(-R, R), network.py:587).  A draw that
        model._noise injects takes its name's place and no part of the pool; an injected 'eik_idx' is a column already
        and stays in the noise."""
        f32 = dict(device=device, dtype=torch.float32)
        # in the order the pool is cut
        shapes = {'jitter': (d.N, d.n_eval), 'final_u': (d.N, d.n_final), 'nei_rand': (2 * d.N, 3), 'eik_idx': (d.N,),
                  'eik_uniform': (d.N, 3)}
        if not d.want_points:
            del shapes['nei_rand'], shapes['eik_uniform']
        need = [k for k in shapes if noise.get(k) is None]
        pool = torch.rand(sum(math.prod(shapes[k]) for k in need), **f32) if need else None
        draws, off = {}, 0
        for k, shape in shapes.items():
            if k in need:
                n = math.prod(shape)
                draws['eik_u' if k == 'eik_idx' else k] = pool[off:off + n].view(shape)
                off += n
            elif k != 'eik_idx':
                draws[k] = noise[k].to(**f32).contiguous()
        return draws, 'eik_uniform' in need

    def _finish_inputs(self, call, noise, draws, extra_idx):
        """Everything the finish kernel needs -- none of it depends on the number of rounds -- issued while the
        GPU is still busy with the first round, so that after a host sync only the launch is left.  Returns the
        kernel's outputs (z_out, z_eik, pts_out or None)."""
        d, dev = call.sizes, call.device
        eik_idx = noise.get('eik_idx')
        if eik_idx is None and 'eik_u' not in draws:
            eik_idx = torch.randint(d.S, (d.N,), device=dev)
        if eik_idx is not None:
            eik_idx = eik_idx.to(device=dev, dtype=torch.int64).contiguous()
        if extra_idx is None:
            extra_idx = self._extra_columns(d.training, noise, dev)[0]
        call.bind(eik_idx=eik_idx, eik_u=draws.get('eik_u'), eik_uniform=draws.get('eik_uniform'),
                  nei_rand=draws.get('nei_rand'), extra_idx=extra_idx)
        return call.alloc('z_out', 'z_eik', 'pts_out')

    def _round(self, call, k, net, speculate, save_for):
        """Round k of the call: the SDF at the new points, beta and the convergence flag, the next samples."""
        pts, flags = call.held['pts'], call.held['flags']
        # fused forward kernel on the new points, [N*n_eval, 1]; in a speculated round it returns at once when the
        # previous round did not ask for this one
        run_flag = flags.data_ptr() + 4 * (2 * k - 1) if (speculate > 0 and k > 0) else None
        call.bind(new_sdf=net._sdf_only(pts, run_flag=run_flag, save_for=save_for), M=call.sizes.n_eval * (k + 1),
                  round_idx=k)
        call.launch('msdf_sampler_beta')
        group = self.global_rounds
        if group is not None:
            # bits of a positive float order like the float: an integer MAX over ranks is the batch's max beta
            import torch.distributed as dist
            dist.all_reduce(flags[2 * k:2 * k + 1], op=dist.ReduceOp.MAX, group=None if group is True else group)
        call.launch('msdf_sampler_resample')

    def sample(self, ray_dirs, cam_loc, model, want_points=True, speculate=0, beta0=None, sdf_reuse=None):
        """get_z_vals plus (optionally) the 3-D points of the ray samples and, in training, the eikonal
        points appended behind them -- written by the finish kernel instead of ~15 small tensor ops.

        speculate = k > 0: enqueue exactly k rounds WITHOUT reading the batch-global convergence flag back (the
        one host sync per round, during which the GPU would drain); rounds beyond the ones the flags ask for do
        nothing.  The caller enqueues the rest of its work and then calls confirm(), which tells whether k was
        enough.

        sdf_reuse: the ops.SdfReuse of the pass (needs want_points).  The finish kernel writes its row_map; and when
        exactly one round is enqueued (speculate == 1) or the rounds are decided one by one (speculate == 0), the SDF
        evaluation of the first round saves the hidden activations of the dense-set columns for the SDF node.  With
        more rounds enqueued the final columns come from a merged set: nothing is saved, nothing is paid for."""
        dev = ray_dirs.device
        ray_dirs, cam_loc = _need_gpu(ray_dirs), _need_gpu(cam_loc)
        self._resolve()               # bookkeeping of the previous call (its flags arrived long ago)
        K = self.max_total_iters
        d = _Sizes(ray_dirs.shape[0], self.N_samples_eval, self.N_samples, self.N_samples_extra, K,
                   bool(model.training), bool(want_points))
        noise = getattr(model, '_noise', None) or {}
        beta0 = (model.density.get_beta() if beta0 is None else beta0).detach().float().reshape(1).contiguous()
        call = _SamplerCall(d, dev, beta_iters=self.beta_iters, near=float(self.near), far=float(self.far),
                            bound=float(self.scene_bounding_sphere), eps=float(self.eps),
                            add_tiny=float(self.add_tiny), lemma=self._lemma)
        draws, eik_unit = self._draws(noise, d, dev) if d.training else ({}, False)
        call.bind(ray_o=cam_loc, ray_d=ray_dirs, beta0=beta0, jitter=draws.get('jitter'), u_final=draws.get('final_u'),
                  eik_unit=eik_unit)
        pts, flags = call.alloc('pts', 'flags')
        call.alloc('z', 'sdf', 'new_z', 'new_pos', 'beta', 'final_z')
        extra_idx = save_for = None
        if sdf_reuse is not None:
            assert want_points and (sdf_reuse.N, sdf_reuse.S, sdf_reuse.n_extra) == (d.N, d.S, d.n_extra)
            assert sdf_reuse.P == d.N * d.S + (4 * d.N if d.training else 0)
            sdf_reuse.attach_sampler(flags, pts)
            call.bind(row_map=sdf_reuse.row_map, h_saved=sdf_reuse.h_saved)
            if sdf_reuse.n_reuse > 0 and speculate in (0, 1):
                extra_idx, col_slot = self._extra_columns(d.training, noise, dev, want_slots=True)
                if col_slot is not None:
                    save_for = (sdf_reuse, col_slot, d.n_eval)
        call.launch('msdf_sampler_init')
        # one all-reduce is enqueued per enqueued round, so the count must be the same on every rank of the group: the
        # caller's guess comes from guess_rounds(), which in this mode looks only at the history of all-reduced
        # decisions -- identical on every rank as long as the ranks make their group calls in lockstep (they must:
        # each one is a collective).  Round 3 enqueued all max_total_iters rounds here: K - 1 idle rounds and
        # collectives per call in the usual one-round state.
        which = 1 if self.global_rounds is not None else 0
        with torch.no_grad():
            self._round(call, 0, model.implicit_network, speculate, save_for)
            # behind the first round's launches, before any host read of the flags (see _finish_inputs)
            z_out, z_eik, x_all = self._finish_inputs(call, noise, draws, extra_idx)
            rounds = 1
            # speculating: as many rounds as asked for; else the one host sync of the round
            while (rounds < min(speculate, K)) if speculate > 0 else bool(flags[2 * rounds - 1].item()):
                self._round(call, rounds, model.implicit_network, speculate, None)
                rounds += 1
        self._pending = None
        self.stats['calls'] += 1
        if speculate > 0:
            host = torch.empty(flags.shape, dtype=flags.dtype, pin_memory=True)
            host.copy_(flags, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._pending = (ev, host, rounds, which)
        else:
            self._note_rounds(rounds, which)
        # final set: 64 importance samples + near + far + 32 columns of the dense set
        call.launch('msdf_sampler_finish')
        return z_out, z_eik, x_all
