"""PPO on the fused HIP path (reference: torchrl/algo/on_policy/ppo.py:10-160).

Per epoch (`update_per_epoch`, ppo.py:27-39):
  1. last_value + GAE scan over the rollout (kernels, on_rl_algo.py:22-33);
  2. linear LR decay for both optimisers, `target_pf <- pf` (utils.py:23-32);
  3. `opt_epochs` permutations of the time rows from the global numpy RNG -- the
     reference's index stream, one permutation per pass (on_policy.py:76-78);
  4. advantage statistics of EVERY minibatch in one launch (trl_adv_stats_f64);
  5. per minibatch, three launches: fused gradient (critic + actor, fp32 MFMA,
     row gather fused in), partial fold, global-norm clip + Adam for both nets.
     Critic and actor are independent networks, so computing both gradients
     before either step is the same arithmetic as the reference's
     critic-then-actor order (ppo.py:149-150).
Nothing is read back until the epoch ends; then one copy fetches the statistics
of all minibatches and the logger receives the same info dicts, in order.

`update(batch)` keeps the reference's single-minibatch entry point (ppo.py:124-152).
"""
import copy
import ctypes as C
import os
import math

import numpy as np
import torch
import torch.optim as optim

from ... import _C
from ... import dist
from ...networks import ZeroNet, flatten_into
from ...policies.continuous_policy import HEAD_CAT, HEAD_GAUSS, HEAD_NAME, HEAD_SD, HEAD_TAG, head_kind, is_state_std  # noqa: F401
from .. import _optim
from .. import utils as atu
from .._graphs import GraphCache, LastGraph
from .a2c import A2C

_HALF_LOG_2PI_PLUS_HALF = 0.5 + 0.5 * math.log(2 * math.pi)


def _hyper(algo):
    """(clip_para, entropy_coeff, clipped_value_loss, tanh_action): what a loss kernel takes besides the data."""
    return (float(getattr(algo, "clip_para", 0.0)), float(algo.entropy_coeff),
            int(bool(getattr(algo, "clipped_value_loss", False))), int(bool(algo.pf.tanh_action)))


def _critic(algo):
    """The value network, or None for a vacant critic (`networks.ZeroNet`: the rule the collector uses)."""
    return None if isinstance(algo.vf, ZeroNet) else algo.vf


def _stat_views(block, K):
    """raw (K, 4) f64 | info (K, 24) f64 | norms (K, 2) f32 of a 29 K statistics block, on the device or its host twin."""
    return block[:4 * K].view(K, 4), block[4 * K:28 * K].view(K, 24), block[28 * K:].view(torch.float32).view(K, 2)


class PPO(A2C):
    loss_mode = _C.LOSS_PPO_CLIP

    def __init__(self, pf, clip_para=0.2, opt_epochs=10, clipped_value_loss=False, **kwargs):
        self.target_pf = copy.deepcopy(pf)
        super().__init__(pf=pf, **kwargs)
        self.clip_para = clip_para
        self.opt_epochs = opt_epochs
        self.clipped_value_loss = clipped_value_loss
        self.sample_key = ["obs", "acts", "advs", "estimate_returns", "values"]
        self._engine = None

    @property
    def networks(self):
        return [self.pf, self.vf, self.target_pf]

    def engine(self):
        if self._engine is None:
            self._engine = make_engine(self)
        return self._engine

    # ---- epoch ----
    def _fill_old_logp(self):
        """log pi_old of every stored (obs, act) under target_pf (ppo.py:54-56), computed once per
        epoch; update_per_epoch skips it when the collector kernel already wrote it with the same parameters."""
        buf = self.replay_buffer
        rows, n = buf._max_replay_buffer_size, buf.env_nums
        tgt = self.target_pf
        kind = head_kind(tgt)
        if kind == HEAD_CAT:                                           # categorical head: MLP forward + trl_cat_logp_f32
            with torch.no_grad():
                _C.cat_logp(tgt.logits(buf._obs.reshape(rows * n, -1)).contiguous(), buf._acts.reshape(rows * n),
                            out=buf._ensure_key("old_logp", (n, 1)).view(rows * n))
            return
        if kind == HEAD_SD:                                            # [mean | log_std] head: MLP forward + trl_gauss_sd_logp_f32
            from ... import ops
            with torch.no_grad():
                layers, code = ops.net_layers(tgt)
                head, _ = ops.mlp_forward(layers, buf._obs.reshape(rows * n, -1), code, keep=False)
                _C.gauss_sd_logp(head, buf._acts.reshape(rows * n, -1), bool(tgt.tanh_action),
                                 out=buf._ensure_key("old_logp", (n, 1)).view(rows * n))
            return
        with torch.no_grad():                                          # kernels only: MLP forward + trl_gauss_logp_f32
            mean, _, log_std = tgt.forward(buf._obs.reshape(rows * n, -1))
            _C.gauss_logp(mean.contiguous(), buf._acts.reshape(rows * n, -1), log_std.float().contiguous(),
                          bool(tgt.tanh_action), out=buf._ensure_key("old_logp", (n, 1)).view(rows * n))

    def update_per_epoch(self):
        """ppo.py:27-39.  Everything the host decides -- the linear LR decay and the `opt_epochs` permutations of the
        time rows (global numpy stream, one per pass) -- is done first; everything on the device -- last value + GAE
        scan (on_rl_algo.py:22-33), `target_pf <- pf`, log pi_old, then all minibatch updates -- is handed to the engine
        as ONE launch sequence, which a single process replays as one HIP graph from its third visit on."""
        atu.update_linear_schedule(self.pf_optimizer, self.current_epoch, self.num_epochs, self.plr)
        atu.update_linear_schedule(self.vf_optimizer, self.current_epoch, self.num_epochs, self.vlr)
        buf = self.replay_buffer
        buf._scan_inputs()                                             # advs / estimate_returns exist before they are named
        buf._ensure_key("old_logp", (buf.env_nums, 1))
        passes = [buf.epoch_row_indices(self.batch_size, self.shuffle) for _ in range(self.opt_epochs)]
        row_idx = np.concatenate(passes, axis=0)                       # (E * n_mb, B // N)
        tensors = {"obs": buf._obs, "acts": buf._acts, "advs": buf._advs, "rets": buf._estimate_returns,
                   "old_values": buf._values, "old_logp": buf._old_logp}
        fresh = bool(getattr(buf, "_old_logp_fresh", False))          # the collector kernel wrote log pi_old already
        buf._old_logp_fresh = False

        def device_prologue():
            self.process_epoch_samples()
            self.engine().sync_target_pf(in_prologue=True)             # target_pf <- pf (utils.py:23-26)
            if not fresh:
                self._fill_old_logp()
        self._run_and_log(tensors, row_idx, buf.env_nums, pre=device_prologue,
                          pre_key=(fresh, self.gae, bool(getattr(buf, "_boot_fresh", False))))

    # ---- single minibatch (reference entry point) ----
    def update(self, batch):
        self.training_update_num += 1
        dev = self.device
        as_t = lambda x: (x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))) \
            .to(device=dev, dtype=torch.float32).contiguous()
        obs, acts = as_t(batch['obs']), as_t(batch['acts'])
        B = obs.shape[0]
        if "old_logp" in batch:
            old_lp = as_t(batch["old_logp"]).reshape(B, 1)
        else:
            with torch.no_grad():
                old_lp = self.target_pf.update(obs, acts)["log_prob"].reshape(B, 1).contiguous()
        tensors = {"obs": obs.reshape(1, B, -1), "acts": acts.reshape(1, B, -1),
                   "advs": as_t(batch['advs']).reshape(1, B, 1), "rets": as_t(batch['estimate_returns']).reshape(1, B, 1),
                   "old_values": as_t(batch['values']).reshape(1, B, 1), "old_logp": old_lp.reshape(1, B, 1)}
        return self.engine().run(tensors, np.zeros((1, 1), dtype=np.int64), B)[0]


class _FusedPPO:
    """Flat parameter / optimiser-state buffers and the per-minibatch launch sequence."""

    def __init__(self, algo):
        self.algo = algo
        pf, vf = algo.pf, _critic(algo)
        ps, vs = pf.mlp2_spec(), None if vf is None else vf.mlp2_spec()
        # a vacant critic (vf None): the policy alone in the flat buffers, every gradient workgroup the policy's
        # a categorical head (policies.CategoricalDisPolicy): the gradient kernel's HEAD_CAT instantiations and their folds
        # (trl_ppo_cat_*); no logstd in the flat vector, the entropy arrives through info slot 20
        # a state-dependent-std head (policies.GuassianContPolicy): the network emits [mean | log_std]; the gradient kernel's
        # HEAD_SD instantiations and their folds (trl_ppo_sd_*); no logstd in the flat vector either, `self.A` = half the head's
        # width, entropy and the per-element log_std / std statistics arrive through info slots 20, 8-11 and 16-19
        needs = "fused PPO needs MLP2 nets and a GuassianContPolicyBasicBias, GuassianContPolicy or CategoricalDisPolicy policy"
        if ps is None or (vf is not None and vs is None):
            raise _C.TrlError(needs)
        self.head = head_kind(pf, refuse=needs)
        self.categorical, self.state_std = self.head == HEAD_CAT, self.head == HEAD_SD
        if self.head != HEAD_GAUSS:
            ps = _head_spec(self.head, ps)
            why = _fused_head_refusal(self.head, ps)
            if why:
                raise _C.TrlError(why)
        if vf is not None and (vs[0] != ps[0] or vs[1] != ps[1] or vs[2] != 1 or vs[3] != ps[3]):
            raise _C.TrlError("policy %s and value %s must share input, width and activation" % (ps, vs))
        self.D, self.H, self.A, self.act = ps
        self.dev = next(pf.parameters()).device
        if self.dev.type != "cuda":
            raise _C.TrlError("PPO networks live on %s: the fused path needs a GPU (no CPU path exists)" % self.dev)
        tail = (lambda net: []) if (self.categorical or self.state_std) else (lambda net: [net.logstd])
        pf_list = pf._mlp2_param_list() + tail(pf)
        vf_list = [] if vf is None else vf._mlp2_param_list()
        tgt = getattr(algo, "target_pf", None)
        self._home(pf_list, vf_list, None if tgt is None else tgt._mlp2_param_list() + tail(tgt))
        if tgt is not None and (self.categorical or self.state_std):   # (its forward must find THIS storage, see _GenericPPO)
            tgt._flat = self.target_flat
        lib = _C.lib()
        sfx = HEAD_TAG[self.head]
        kernel = lambda name: (getattr(lib, name), name)
        self._k_grad = kernel("trl_ppo_%sminibatch_grad_f32" % sfx)
        self._k_fold, self._k_fold_net = kernel("trl_ppo_%sreduce_adam_f32" % sfx), kernel("trl_ppo_%sreduce_adam_net_f32" % sfx)
        # (the folds that carry the gradient SUM over ranks exist for the shared-std Gaussian head only)
        self._k_fold_x, self._k_fold_net_x = kernel("trl_ppo_reduce_adam_xrank_f32"), kernel("trl_ppo_reduce_adam_xrank_net_f32")
        self.p_stride = getattr(_C, "ppo_%spartial_stride" % sfx)(self.D, self.H, self.A)
        # doubles of scalar statistics per workgroup (SD: a second block of rows behind the n_wg x 8 of every head)
        self.scal_w = _C.ppo_sd_scalar_stride() if self.state_std else 8
        self.n_cu = torch.cuda.get_device_properties(self.dev).multi_processor_count
        self.max_wg = 2 * max(1, self.n_cu // 2)
        self.partial = torch.zeros(self.max_wg, self.p_stride, device=self.dev)
        self.scal = torch.zeros(self.max_wg, self.scal_w, dtype=torch.float64, device=self.dev)
        n_ws = getattr(lib, "trl_ppo_%sreduce_adam_workspace" % sfx)(self.D, self.H, self.A)
        self.red_ws = torch.zeros(n_ws, device=self.dev)              # Adam header + norm granules of the fold / clip / Adam launch
        # One process: the critic's and the actor's updates of an epoch (ppo.py:93-122 / 41-91: separate networks, optimisers,
        # clips and statistics) run as TWO launch sequences on two streams (`_run_chains`); TRL_PPO_CHAINS=joint keeps the
        # single sequence in which every gradient launch carries both networks.  Same bits either way.
        self.two_chains = os.environ.get("TRL_PPO_CHAINS", "two") != "joint"
        self.red_ws_v = torch.zeros(n_ws, device=self.dev)            # the value chain's own Adam header + norm granules
        self.red_ws_v[4:8].view(torch.float64).fill_(1.0)
        self._side, self._value_done, self._hdr_owner, self._chain_graphs = None, None, "joint", {}
        self._joint = LastGraph()                                      # the joint sequence's graph (`_graph`)
        self._pending, self._chain_pend, self._chain_seen = None, [], set()         # deferred statistics; shapes already run eagerly
        self._stats2_key = self._chain_rows = self._pro_ws = None                    # (allocated by the first run of a shape)
        self.red_ws[4:8].view(torch.float64).fill_(1.0)               # beta1^0, beta2^0 (device-side Adam state)

    eps = 1e-5                                                       # Adam's, of A2C's two optimisers (a2c.py:30-31)

    def _home(self, pf_list, vf_list, target_list):
        """The networks' home: `flat` = [pf | vf] with the parameters views of it (nets that are MLP2 blocks hand their
        own flat view to the fused inference kernel, Net.flat_params: it must be THIS storage, or the first forward after
        the engine exists would re-home the parameters away from it), the moments and gradients beside it, `target_flat`
        mirroring the policy block, and each optimiser's state bound to the moments.  An empty `vf_list` is a vacant
        critic: `P_vf = 0`, `flat` is the policy's alone, there is no `vf_optimizer`, and `eps` is the one optimiser's own."""
        algo = self.algo
        self.P_pf = sum(p.numel() for p in pf_list)
        self.P_vf = sum(p.numel() for p in vf_list)
        self.flat = flatten_into(pf_list + vf_list)
        self.m, self.v, self.grads = torch.zeros_like(self.flat), torch.zeros_like(self.flat), torch.zeros_like(self.flat)
        self.step_count = 0
        self.target_flat = None if target_list is None else flatten_into(target_list)
        # the step both optimisers take (`_optim.step_spec`).  Adam: m = exp_avg, v = exp_avg_sq; RMSprop: m = square_avg,
        # v = momentum_buffer, c = grad_avg (centered only); SGD: m = momentum_buffer -- bound under torch's names for the class
        self.opt_spec = _optim.step_spec(algo.pf_optimizer)
        if self.opt_spec[0] not in self.step_kinds:
            raise _C.TrlError("%s implements torch.optim.Adam only (got %s)"
                              % (type(self).__name__, type(algo.pf_optimizer).__name__))
        if vf_list and _optim.step_spec(algo.vf_optimizer) != self.opt_spec:
            raise _C.TrlError("the policy's and the value function's optimisers must take the same step (%r / %r)"
                              % (self.opt_spec, _optim.step_spec(algo.vf_optimizer)))
        self.c = torch.zeros_like(self.flat) if _optim.needs_third([self.opt_spec]) else None
        if not vf_list:
            self.eps = float(algo.pf_optimizer.param_groups[0].get('eps', self.eps))
        for net, plist, opt, lo in ((algo.pf, pf_list, "pf_optimizer", 0), (algo.vf, vf_list, "vf_optimizer", self.P_pf)):
            if plist:
                if getattr(net, "mlp2_spec", lambda: None)() is not None:
                    net._flat = self.flat[lo:lo + sum(p.numel() for p in plist)]
                self._alias_optimizer_state(getattr(algo, opt), plist, lo)

    step_kinds = ("adam",)                                           # what `_optim.step_spec` may name for this engine
    c = None                                                         # the third state buffer: a centered RMSprop's alone

    def _alias_optimizer_state(self, opt, plist, offset):
        self._opt_steps = getattr(self, "_opt_steps", [])
        self._opt_steps += _optim.bind_state(opt, self.opt_spec, plist, offset, (self.m, self.v, self.c))

    def sync_target_pf(self, in_prologue=False):
        """target_pf <- pf.  in_prologue (called from an epoch's device prologue): the copy rides in the launch that
        computes the advantage statistics (`_C.ppo_epoch_prologue`) instead of being a launch of its own."""
        if self.target_flat is not None and in_prologue:
            self._copy_in_prologue = True
        elif self.target_flat is not None:
            self.target_flat.copy_(self.flat[:self.P_pf])
        else:
            atu.copy_model_params_from_to(self.algo.pf, self.algo.target_pf)

    def _n_wg(self, n_samples):
        """(workgroups to launch, how many of them run the policy) for one minibatch."""
        tiles = (n_samples + 15) // 16
        n_wg = 2 * max(1, min(self.max_wg // 2, (tiles + 3) // 4))
        n_pf = _C.lib().trl_ppo_wg_split(self.D, self.H, self.A, tiles, n_wg)
        if not 0 < n_pf < n_wg:
            raise _C.TrlError("trl_ppo_wg_split(%d tiles, %d workgroups) returned %d" % (tiles, n_wg, n_pf))
        if n_wg >= self.n_cu and n_wg % 8 == 0 and n_wg >= 16:
            # A full-chip grid: workgroup i runs on XCD i % 8, one workgroup per CU.  When the two networks' workgroups are
            # launched as SEPARATE kernels (two chains), a split that is not a multiple of 8 puts 33 workgroups on some XCDs
            # and 31 on others (147 + 109: 19 + 14 on XCDs 0-2) -- the 33rd waits a whole pass for a CU (round 6: 4.5-6 us
            # per launch).  The neighbouring multiples of 8 are compared with the cost model of trl_ppo_wg_split (a tile of
            # the policy costs 1.3 of the value net's; both counts of tiles per wave are what matters): 152 + 104 here.
            waves = lambda x: -(-tiles // (4 * x))
            cost = lambda x: max(waves(x) * 15.3, waves(n_wg - x) * 11.8)
            cands = [x for x in (n_pf // 8 * 8, -(-n_pf // 8) * 8) if 0 < x < n_wg]
            if cands:
                n_pf = min(cands, key=lambda x: (cost(x), abs(x - n_pf)))
        return n_wg, n_pf

    def _buffers(self, K, rows_mb):
        """Persistent per-shape buffers: minibatch row indices and the statistics block
        raw (K,4) f64 | info (K,24) f64 | norms (K,2) f32 on the device (stable addresses, so that a captured launch
        sequence can be replayed), plus their page-locked host twins: the per-epoch H2D of the indices and D2H of the
        statistics are asynchronous copies, the only host wait of an update is the one at its end."""
        key = (K, rows_mb)
        if getattr(self, "_buf_key", None) != key:
            self._buf_key = key
            self._idx_buf = torch.zeros(K * rows_mb, dtype=torch.int64, device=self.dev)
            self._stats = torch.zeros(29 * K, dtype=torch.float64, device=self.dev)
            # page-locked slab: the epoch's row indices, then one 8-byte slot for the two learning rates
            self._slab_host = torch.zeros(K * rows_mb + 1, dtype=torch.int64).pin_memory()
            self._idx_host = self._slab_host[:K * rows_mb]
            self._hyper_host = self._slab_host[K * rows_mb:].view(torch.float32)
            self._hyper = None
            self._stats_host = torch.zeros(29 * K, dtype=torch.float64).pin_memory()
            if self._joint is not None:
                self._joint.clear()                                    # (its graph carries the old addresses)
        return self._idx_buf, self._stats

    @property
    def _graph(self):
        """The joint sequence's captured graph, or None."""
        return None if self._joint is None else self._joint.graph

    def _set_device_hyper(self, lr_pf, lr_vf, upload=True):
        """The learning rates into their page-locked slot; upload=False: the epoch prologue launch copies them (and the
        row indices) itself, reading the slab in place."""
        hyper = (float(lr_pf), float(lr_vf))
        if getattr(self, "_hyper", None) != hyper or not upload:
            self._hyper = hyper if upload else None
            self._hyper_host[0], self._hyper_host[1] = hyper
            if upload:
                self.red_ws[2:4].copy_(self._hyper_host, non_blocking=True)

    # ---- the launch builder: what the joint sequence and the two chains enqueue, called from their launch closures only
    # (eager visits and captures; a replayed visit builds nothing) ----
    def _lrs(self):
        """(the policy's, the value function's) learning rate, 0.0 for a network that does not exist."""
        lr = lambda opt: float(getattr(self.algo, opt).param_groups[0]['lr'])
        return lr("pf_optimizer"), lr("vf_optimizer") if self.P_vf else 0.0

    def _adam_args(self, lrs=(0.0, 0.0), **kw):
        """clip_grad_norm_(0.5) + Adam(`eps`) over the groups of the flat buffers: one per network that exists."""
        return self._step_args(("adam", self.eps), lrs, **kw)

    def _step_args(self, spec, lrs=(0.0, 0.0), **kw):
        """`_adam_args` for the step `spec` names: an AdamArgs, or the OptArgs of an RMSprop / SGD launch."""
        groups = [(n, lr) for n, lr in zip((self.P_pf, self.P_vf), lrs) if n]
        return _optim.step_args(spec, self.flat, self.grads, (self.m, self.v, self.c), [n for n, _ in groups],
                                [lr for _, lr in groups], max_norm=0.5, **kw)

    def _batch_args(self, t, hyper, loss_mode, rows_mb, N, n_global, partial, scal, n_wg, n_wg_pf):
        """trl_ppo_batch_t of a gradient launch over `n_wg` workgroups that leave their rows in `partial` / `scal`."""
        g = _C.PpoBatchArgs()
        for k in ("obs", "acts", "advs", "rets", "old_values", "old_logp"):
            setattr(g, k, _C.dev_ptr(t[k], name=k).value if t.get(k) is not None else None)
        g.loss_mode = loss_mode
        g.rows_mb, g.N, g.n_global = rows_mb, N, n_global
        g.pf_params, g.vf_params = self.flat.data_ptr(), self.flat.data_ptr() + 4 * self.P_pf if self.P_vf else None
        g.D, g.H, g.A, g.act = self.D, self.H, self.A, self.act
        g.clip_para, g.entropy_coeff, g.clipped_value_loss, g.tanh_action = hyper
        g.partial, g.scal_partial, g.n_wg, g.n_wg_pf = partial.data_ptr(), scal.data_ptr(), n_wg, n_wg_pf
        return g

    def _prologue(self, pre, advs, idx, raw, zero, copies):
        """`pre`, then ONE launch: the advantage statistics of all K minibatches (rows `idx` (K, rows_mb) of `advs`) into
        `raw`, `zero` cleared, and the copies -- target_pf <- pf when `pre` asked for it, then the route's `copies`."""
        self._copy_in_prologue = False
        if pre is not None:
            pre()
        if self._pro_ws is None or self._pro_ws_k != tuple(idx.shape):  # (its counters assume one slicing)
            self._pro_ws, self._pro_ws_k = _C.ppo_epoch_prologue_workspace(idx.shape[0], self.dev), tuple(idx.shape)
        if self._copy_in_prologue:
            copies = [(self.target_flat, self.flat[:self.P_pf])] + copies
        _C.ppo_epoch_prologue(advs, idx, raw, self._pro_ws, zero=zero, copies=copies)
        dist.reduce_adv_raw_(raw)                                      # C2 (identity in one process)

    def _fold(self, kernel, partial, scal, n_wg, which, info, ws, comm=False):
        """fold(k, g, a): the fused reduce / clip / Adam launch `kernel` behind minibatch k's gradient launch, its
        statistics into row k of `info`.  `which`: the policy's workgroup count (joint) or the network (a chain); `comm`:
        the xrank kernels, which take the peer transport's handle."""
        fn, name = kernel
        head = (partial.data_ptr(), scal.data_ptr(), n_wg, which, self.D, self.H, self.A, self.grads.data_ptr())
        tail = (ws.data_ptr(),) + ((dist.comm_handle(),) if comm else ()) + (_C.stream_ptr(self.dev),)
        info_base = info.data_ptr()
        return lambda k, g, a: _C.check(fn(*head, info_base + 192 * k, C.byref(a), *tail), name)

    def _minibatches(self, K, g, a, idx_dev, raw, norms, fold, probe=None):
        """K x {gradient launch, `fold(k, g, a)`} on the current stream."""
        stream = _C.stream_ptr(self.dev)
        idx_base, raw_base, norm_base = idx_dev.data_ptr(), raw.data_ptr(), norms.data_ptr()
        for k in range(K):
            g.row_idx = idx_base + 8 * g.rows_mb * k
            g.adv_raw = raw_base + 32 * k
            a.step_count = self.step_count + k + 1
            a.norms_out = norm_base + 8 * k
            if probe is not None:
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record()
            _C.check(self._k_grad[0](C.byref(g), stream), self._k_grad[1])
            if probe is not None:
                ev[1].record()
                probe.append(ev)
            fold(k, g, a)

    def _stepped(self, K):
        """End of a run: K optimiser steps taken (host bookkeeping under the device's shadow)."""
        self.step_count += K
        for s in self._opt_steps:
            s.fill_(float(self.step_count))

    defers = True                                                    # run(..., defer=True) is implemented
    one_rank = None                                                  # (the refusal's text, where an engine runs on one rank only)

    def run(self, t, row_idx, N, pre=None, pre_key=None, defer=False):
        """t: dict of (rows, N, feat) device tensors; row_idx: (K, rows_mb) host int64.
        Runs K minibatch updates back to back; returns K info dicts (one host sync at the end).
        `defer=True`: returns a `_PendingInfos` right after the launches instead -- the wait for the statistics and the
        assembly of the K dicts happen when somebody asks for them (the logger at its next row) or at the start of the
        next `run`, by which time the next rollout is already running on the device: the host never idles the GPU
        between two iterations.
        `pre` (optional): a callable that enqueues device work which must precede the updates (PPO: last value + GAE
        scan, target_pf copy); it becomes part of the same launch sequence.
        Single process: the whole sequence -- `pre`, the statistics memset, the advantage statistics and the
        K x {gradient kernel, fused reduce/clip/Adam} launches -- is captured into a HIP graph the second time a shape
        is seen and replayed afterwards (dependent launches start ~2.5 us earlier each inside a graph on this machine,
        and the host issues one call instead of ~90); the Adam step count and learning rates live on the device so no
        launch argument changes between replays."""
        algo, dev = self.algo, self.dev
        K, rows_mb = row_idx.shape
        world = dist.world_size()
        n_local = rows_mb * N
        n_global = float(n_local * world)
        n_wg, n_wg_pf = self._n_wg(n_local)
        loss_mode = int(getattr(algo, "loss_mode", _C.LOSS_PPO_CLIP))
        probe = getattr(self, "probe", None)                           # bench.py: HIP events around the grad kernel
        fused = not dist.collectives_active()
        if self.one_rank and not fused:
            raise _C.TrlError(self.one_rank)
        if (self.categorical or self.state_std) and not fused:
            raise _C.TrlError("the fused %s update runs on one rank (no cross-rank fold exists for this head)"
                              % ("categorical" if self.categorical else "state-dependent-std"))
        # (env shards on several ranks: the two chains need the in-launch gradient exchange of the peer transport, whose
        # granules and exchange counts are per network; over all-reduce CALLS the joint sequence stays.  A launch whose
        # workgroups are all one network's -- a vacant critic -- has no second chain: the joint sequence carries it)
        xrank_chains = not fused and self.chains_across_ranks()
        if (fused or xrank_chains) and probe is None and self.two_chains and n_wg_pf >= 1 and n_wg - n_wg_pf >= 1:
            return self._run_chains(t, row_idx, N, pre, pre_key, defer, n_wg, n_wg_pf, loss_mode, n_global, xrank=not fused)
        for last in [self._pending] + list(self._chain_pend):
            if last is not None:                                       # its statistics still sit in the host twin this
                last.land()                                            # run is about to reuse: wait + snapshot (the dicts are
        self._pending, self._chain_pend = None, []                     # assembled when somebody reads them)
        idx_dev, stats = self._buffers(K, rows_mb)
        self._idx_host.numpy()[:] = row_idx.reshape(-1)
        rows_total = t["advs"].shape[0]
        raw, info, norms = _stat_views(stats, K)
        # Env shards on several ranks with the peer transport up (dist.init_comm): the gradient SUM over ranks happens
        # INSIDE the fold / clip / Adam launch (trl_ppo_reduce_adam_xrank_f32) and the statistics go through the
        # one-kernel all-reduce -- plain launches, so the sequence is graph-replayed exactly like the single-process one.
        xrank = not fused and dist.peer_ready()
        self._settle_value_chain()                                     # (a joint launch sequence after a two-chain one)
        if self._value_done is not None:
            from ...networks import nets as _nets
            _nets.set_pending(algo.vf, None)
            self._value_done = None
        self._hdr_owner = "joint"                                      # (its Adam header is red_ws, which the policy chain kept current)
        # TRL_GRAPH_COLLECTIVES=1 (opt-in, RCCL route): capture the multi-rank sequence -- RCCL all-reduces included -- into
        # the HIP graph as well; the Adam step count and learning rates then live on the device like in the fused launch.
        graph_coll = not fused and not xrank and os.environ.get("TRL_GRAPH_COLLECTIVES") == "1"
        lr_pf, lr_vf = self._lrs()
        # One process: no copy command for the epoch's row indices and learning rates -- the prologue launch reads the
        # page-locked slab in place and leaves the device copies the update kernels use.  (The slab is rewritten only after
        # the previous run's statistics have landed, see `last.resolve()` above: that run's launches are done by then.)
        in_place = fused and probe is None
        if not in_place:
            idx_dev.copy_(self._idx_host, non_blocking=True)
        if fused or xrank:
            self._set_device_hyper(lr_pf, lr_vf, upload=not in_place)
        elif graph_coll:
            if getattr(self, "step_state", None) is None:
                n = float(self.step_count)
                self.step_state = torch.tensor([n, 0.9 ** n, 0.999 ** n, 0.0], dtype=torch.float64, device=dev)
                self.lr_dev = torch.zeros(2, device=dev)
            if getattr(self, "_lr_host", None) != (lr_pf, lr_vf):
                self._lr_host = (lr_pf, lr_vf)
                self.lr_dev.copy_(torch.tensor(self._lr_host, dtype=torch.float32), non_blocking=True)
        hyper = _hyper(algo)
        use_graph = (fused or xrank or graph_coll) and probe is None and os.environ.get("TRL_NO_GRAPH") != "1"
        key = (n_wg, n_wg_pf, loss_mode, n_global, rows_total, N, pre_key, pre is not None, xrank, in_place) + hyper + tuple(
            0 if t.get(k) is None else t[k].data_ptr() for k in ("obs", "acts", "advs", "rets", "old_values", "old_logp"))

        def launch_all():
            g = self._batch_args(t, hyper, loss_mode, rows_mb, N, n_global, self.partial, self.scal, n_wg, n_wg_pf)
            a = self._adam_args((lr_pf, lr_vf), device_state=int(fused or xrank))   # step count / lr from the workspace header
            slab = [(idx_dev, self._idx_host), (self.red_ws[2:4], self._hyper_host)] if in_place else []
            self._prologue(pre, t["advs"].reshape(rows_total, N), (self._idx_host if in_place else idx_dev).view(K, rows_mb),
                           raw, stats[4 * K:], slab)
            if fused:                                                  # one process: reduce + clip + Adam in one launch --
                kernel, which = (self._k_fold, n_wg_pf) if self.P_vf else (self._k_fold_net, 0)     # both nets', or the policy's
                fold = self._fold(kernel, self.partial, self.scal, n_wg, which, info, self.red_ws)
            elif xrank:                                                # the same launch with the cross-rank SUM inside
                fold = self._fold(self._k_fold_x, self.partial, self.scal, n_wg, n_wg_pf, info, self.red_ws, comm=True)
            else:
                lib, stream = _C.lib(), _C.stream_ptr(dev)

                def fold(k, g, a):
                    _C.check(lib.trl_ppo_reduce_f32(self.partial.data_ptr(), self.scal.data_ptr(), n_wg, n_wg_pf, self.D,
                                                    self.H, self.A, self.flat.data_ptr(), self.grads.data_ptr(),
                                                    info.data_ptr() + 192 * k, stream), "trl_ppo_reduce_f32")
                    dist.all_reduce_sum_(self.grads)                   # C1: gradient SUM over ranks
                    if graph_coll:
                        a.step_count, a.step_state, a.device_lr = 0, self.step_state.data_ptr(), self.lr_dev.data_ptr()
                    _C.check(lib.trl_clip_adam_f32(C.byref(a), stream), "trl_clip_adam_f32")
            self._minibatches(K, g, a, idx_dev, raw, norms, fold, probe)

        # eager on the first visit of a key, captured on the second, replayed afterwards; a new key starts over
        self._joint.run(key, launch_all, eager=not use_graph)
        dist.reduce_info_(info)
        self._stats_host.copy_(stats, non_blocking=True)
        landed = torch.cuda.Event()
        landed.record()
        self._stepped(K)
        host = self._stats_host
        make = self._info_builder(loss_mode)

        def build(host):
            if xrank:
                dist.check_comm(peek=True)                             # a rank that never delivered: raise, do not hang
            return make(*(v.numpy() for v in _stat_views(host, K)), n_global)
        pending = _PendingInfos(K, landed, host, build)
        if defer:
            self._pending = pending
            return pending
        return pending.resolve()                                       # the only host wait of the update

    def chains_across_ranks(self):
        """Env shards on several ranks: do the updates run as two chains?  Needs the peer transport (the in-launch exchange
        is per network).  Default: yes with one rank per GPU -- each device then runs what a single process runs, plus the
        waits; no when ranks SHARE a device (tests, bench.py's device map): four or more chains and as many waiting fold
        launches on one chip form convoys (two ranks on one MI355X: 5.9 ms per iteration against 5.5 joint, round 6).
        TRL_PPO_CHAINS_XRANK=1 / 0 forces either."""
        if not (self.two_chains and dist.collectives_active() and dist.peer_ready()):
            return False
        want = os.environ.get("TRL_PPO_CHAINS_XRANK")
        return want == "1" if want in ("0", "1") else dist.ranks_per_device() == 1

    def _settle_value_chain(self):
        """The current stream waits for the value chain of the last two-chain run (a no-op when it was waited for already,
        e.g. by the value pass of a fused rollout)."""
        if self._value_done is not None:
            torch.cuda.current_stream(self.dev).wait_event(self._value_done)

    def _sync_headers(self, owner):
        """The joint sequence keeps its Adam header (step count, beta powers, learning rates) in `red_ws`; of the two chains
        the policy's uses `red_ws` and the value's `red_ws_v`.  Both chains step once per update, so the headers agree
        after every run -- a change of route just hands the current one over."""
        if self._hdr_owner != owner:
            if owner == "two":
                self.red_ws_v[:8].copy_(self.red_ws[:8])
            self._hdr_owner = owner

    def _run_chains(self, t, row_idx, N, pre, pre_key, defer, n_wg, n_wg_pf, loss_mode, n_global, xrank=False):
        """K minibatch updates as TWO launch sequences (one process): after the epoch's prologue on the current stream
        (`pre`, advantage statistics, target copy, uploads) the POLICY chain -- K x {gradient launch of the policy's
        workgroups, its fold / clip / Adam} -- stays on the current stream and the VALUE chain -- the same for the value
        function's workgroups -- goes to a side stream.  Critic and actor updates are independent given the epoch's
        advantages (ppo.py:93-122 / 41-91), so the results are those of the joint sequence, bit for bit (same tiles per
        workgroup, same fold order, same Adam arithmetic) -- but the NEXT ROLLOUT, which reads only the policy, starts as
        soon as the policy chain is through, on the CUs that chain frees, while the value chain (whose ten-tile
        workgroups make it the longer one) is still stepping: the rollout's 0.2 ms latency chain disappears under it.
        The value pass behind that rollout waits for the value chain's end event (trl_rollout_t.value_wait_event); every
        other reader of the value function's parameters settles through networks.nets.settle.
        `xrank` (env shards on several ranks, peer transport): each chain's fold launch carries its network's gradient SUM
        over ranks (trl_ppo_reduce_adam_xrank_net_f32: own exchange count, own granules); the advantage statistics are
        reduced in the head, the logged statistics of both chains behind the value chain, on its stream."""
        algo, dev = self.algo, self.dev
        K, rows_mb = row_idx.shape
        main = torch.cuda.current_stream(dev)
        if self._side is None:
            self._side = torch.cuda.Stream(dev)
        side = self._side
        # The host may be ONE run ahead of the device: this run's launches are issued while the previous run's value chain
        # (which ends about when the rollout between the two does) may still be running -- waiting for it here would leave
        # the device waiting for the host right after the value pass.  Everything the host writes per run therefore exists
        # TWICE (page-locked index / learning-rate slab, which the prologue reads in place, and the statistics' host twin),
        # used in turn; the run before the previous one has to have landed before its set is reused.
        last = self._pending                                           # (a joint run before this one)
        if last is not None:
            last.land()
            self._pending = None
        pend = self._chain_pend
        while len(pend) > (0 if os.environ.get("TRL_CHAIN_HOST_AHEAD") == "0" else 1):   # (=0: development A/B, wait for the previous run)
            pend.pop(0).land()
        self._settle_value_chain()                                     # device-side order (normally long satisfied: the value pass waited)
        self._sync_headers("two")
        idx_dev, _ = self._buffers(K, rows_mb)
        if self._stats2_key != (K, rows_mb):
            for q in pend:
                q.land()
            del pend[:]
            self._stats2_key = (K, rows_mb)
            self._stats2 = torch.zeros(2, 29 * K, dtype=torch.float64, device=dev)        # [policy chain | value chain]
            self._chain_host = [(torch.zeros(K * rows_mb + 1, dtype=torch.int64).pin_memory(),
                                 torch.zeros(2, 29 * K, dtype=torch.float64).pin_memory()) for _ in range(2)]
            self._chain_graphs, self._chain_turn = {}, 0
        stats2 = self._stats2
        turn = self._chain_turn = 1 - self._chain_turn
        slab, stats_host = self._chain_host[turn]
        idx_host, hyper_host = slab[:K * rows_mb], slab[K * rows_mb:].view(torch.float32)
        idx_host.numpy()[:] = row_idx.reshape(-1)
        rows_total = t["advs"].shape[0]
        raw = stats2[0, :4 * K].view(K, 4)
        lr_pf, lr_vf = self._lrs()
        hyper_host[0], hyper_host[1] = lr_pf, lr_vf
        self._hyper = None                                             # (the joint route uploads its own copy when it runs next)
        hyper = _hyper(algo)
        n_wg_vf = n_wg - n_wg_pf
        if self._chain_rows is None:
            self._chain_rows = (torch.zeros(self.max_wg, self.p_stride, device=dev),
                                torch.zeros(self.max_wg, self.scal_w, dtype=torch.float64, device=dev))
        partial_v, scal_v = self._chain_rows                           # (the policy chain uses self.partial / self.scal)
        shape_key = (n_wg, n_wg_pf, loss_mode, n_global, rows_total, N, pre_key, pre is not None, xrank) + hyper
        key = shape_key + (turn,) + tuple(
            0 if t.get(k) is None else t[k].data_ptr() for k in ("obs", "acts", "advs", "rets", "old_values", "old_logp"))

        def head():
            self._prologue(pre, t["advs"].reshape(rows_total, N), idx_host.view(K, rows_mb), raw, stats2.view(-1)[4 * K:],
                           [(idx_dev, idx_host), (self.red_ws[2:4], hyper_host), (self.red_ws_v[2:4], hyper_host)])

        def chain(net):
            part, scal, ws, wgs, wgs_pf = (self.partial, self.scal, self.red_ws, n_wg_pf, n_wg_pf) if net == 0 else \
                (partial_v, scal_v, self.red_ws_v, n_wg_vf, -1)
            g = self._batch_args(t, hyper, loss_mode, rows_mb, N, n_global, part, scal, wgs, wgs_pf)
            a = self._adam_args((lr_pf, lr_vf), device_state=1)
            _, info, norms = _stat_views(stats2[net], K)
            # (xrank: the network's gradient SUM over ranks inside the fold launch)
            fold = self._fold(self._k_fold_net_x if xrank else self._k_fold_net, part, scal, wgs, net, info, ws, comm=xrank)
            self._minibatches(K, g, a, idx_dev, raw, norms, fold)

        # (graphs by key, a few of them: the stored observations alternate between the ring's tensor and its shadow, see
        # collector/on_policy.py::_launch, so a steady run replays TWO captured sets in turn)
        use_graph = os.environ.get("TRL_NO_GRAPH") != "1"
        cache, seen = self._chain_graphs, self._chain_seen
        graphs = cache.get(key) if use_graph else None
        if use_graph and graphs is None and shape_key in seen and len(cache) < 8:
            # a shape's first run is eager (kernels load, attributes are set); every set of addresses after that is captured
            # on its first visit -- the two sets of a steady run are both replaying from the fourth iteration on
            g0, _ = _C.capture_graph(head)
            gp, _ = _C.capture_graph(lambda: chain(0))
            with torch.cuda.stream(side):
                gv, _ = _C.capture_graph(lambda: chain(1))
            graphs = cache[key] = (g0, gp, gv)
        elif graphs is None:
            seen.add(shape_key)                                        # first visit of a shape: eager (warm-up)
        run_head, run_p, run_v = (head, lambda: chain(0), lambda: chain(1)) if graphs is None else \
            (graphs[0].replay, graphs[1].replay, graphs[2].replay)
        only = os.environ.get("TRL_CHAIN_ONLY")                        # development aid (tools/time_chains.py): one chain alone
        if only == "v":
            run_p = lambda: None
        if only == "p":
            run_v = lambda: None
        run_head()
        forked = torch.cuda.Event()
        forked.record(main)
        run_p()                                                        # policy chain: the current stream (the next rollout follows it)
        if not xrank:
            stats_host[0].copy_(stats2[0], non_blocking=True)
        landed_p = torch.cuda.Event()
        landed_p.record(main)
        with torch.cuda.stream(side):                                  # value chain: beside it, and beside the next rollout
            side.wait_event(forked)
            if getattr(self, "_test_value_chain_delay", 0):            # tests: hold the value chain back (device spin) so that the
                torch.cuda._sleep(int(self._test_value_chain_delay))   # next rollout really runs beside / ahead of it
            run_v()
            if xrank:
                # C3 for both chains' statistics, here: the current stream goes on to the rollout without another
                # collective, and the next one it issues (the next head's C2) comes after its value pass has waited for
                # this stream -- every rank issues the small all-reduces in the same order
                side.wait_event(landed_p)
                for st_ in (stats2[0], stats2[1]):
                    dist.reduce_info_(st_[4 * K:28 * K].view(K, 24))
                stats_host[0].copy_(stats2[0], non_blocking=True)
            stats_host[1].copy_(stats2[1], non_blocking=True)
            done_v = torch.cuda.Event()
            done_v.record(side)
        self._value_done = done_v
        from ...networks import nets as _nets
        _nets.set_pending(algo.vf, done_v)
        self._stepped(K)
        make = self._info_builder(loss_mode)

        class _Both:
            @staticmethod
            def synchronize():
                landed_p.synchronize()
                done_v.synchronize()

        def build(host):
            if xrank:
                dist.check_comm(peek=True)                             # a rank that never delivered: raise, do not hang
            (raw, info, norms), (_, info_v, norms_v) = _stat_views(host[0], K), _stat_views(host[1], K)
            info, norms = info.clone(), norms.clone()
            for col in (7, 12, 13, 14, 15):                             # the value chain's entries of the statistics row
                info[:, col] = info_v[:, col]
            norms[:, 1] = norms_v[:, 1]
            return make(raw.numpy(), info.numpy(), norms.numpy(), n_global)
        pending = _PendingInfos(K, _Both, stats_host, build)
        if defer:
            pend.append(pending)
            return pending
        out = pending.resolve()
        self._settle_value_chain()                                     # a caller that reads in place gets settled parameters too
        return out

    def _info_builder(self, loss_mode):
        """What turns a landed statistics block into the K info dicts, by the loss the kernels ran (`_infos_reinforce` is
        the policy-only engines' own: algo/on_policy/reinforce.py)."""
        names = {_C.LOSS_PPO_CLIP: "_infos", _C.LOSS_A2C: "_infos_a2c", _C.LOSS_REINFORCE: "_infos_reinforce"}
        return getattr(self, names[loss_mode])

    def _infos_a2c(self, raw, info, norms, n):
        """The info dict of A2C.update (a2c.py:86-105); `std` is (B, A) there, each dim repeated B times."""
        out = []
        c_ent = float(self.algo.entropy_coeff)
        A = self.A
        categorical, state_std = self.categorical, self.state_std
        for r, i, g in zip(raw, info, norms):
            v_var = max((i[13] - i[12] * i[12] / n) / (n - 1), 0.0)
            if categorical or state_std:                                # the kernel's entropy sum; SD: per-element statistics
                ent, std_std = i[20] / n, i[17]                         # over all n * A values, as logged
            else:
                ent = A * _HALF_LOG_2PI_PLUS_HALF + A * i[8]
                std_ss = (i[17] ** 2) * (A - 1) if A > 1 else 0.0        # sum over dims of (std - mean)^2
                std_std = math.sqrt(n * std_ss / (n * A - 1))
            d = {'Training/policy_loss': i[0] / n - c_ent * ent, 'Training/vf_loss': i[7] / n,
                 'v_pred/mean': i[12] / n, 'v_pred/std': math.sqrt(v_var), 'v_pred/max': i[14], 'v_pred/min': -i[15]}
            if not categorical:                                         # (no `std` in a categorical policy's dict: a2c.py:62-63, 96-101)
                d.update({'std/mean': i[16], 'std/std': std_std, 'std/max': i[18], 'std/min': i[19]})
            d['ent'], d['log_prob'] = ent, i[1] / n
            out.append(d)
        return out

    def _infos(self, raw, info, norms, n):
        """K info dicts with the keys of PPO.update (ppo.py:76-90, 120-122, 141-146), assembled column-wise."""
        c_ent = float(self.algo.entropy_coeff)
        r, i = raw, info
        adv_var = np.maximum((r[:, 1] - r[:, 0] * r[:, 0] / n) / (n - 1), 0.0)
        lp_var = np.maximum((i[:, 2] - i[:, 1] * i[:, 1] / n) / (n - 1), 0.0)
        categorical = self.categorical                                 # entropy: the kernel's sum; no log_std/* keys
        ent = i[:, 20] / n if (categorical or self.state_std) else \
            self.A * _HALF_LOG_2PI_PLUS_HALF + self.A * i[:, 8]
        cols = (('advs/mean', r[:, 0] / n), ('advs/std', np.sqrt(adv_var)), ('advs/max', r[:, 2]), ('advs/min', -r[:, 3]),
                ('Training/vf_loss', i[:, 7] / n), ('grad_norm/vf', norms[:, 1].astype(np.float64)),
                ('Training/policy_loss', i[:, 0] / n - c_ent * ent),
                ('logprob/mean', i[:, 1] / n), ('logprob/std', np.sqrt(lp_var)), ('logprob/max', i[:, 3]),
                ('logprob/min', -i[:, 4]), ('log_std/mean', i[:, 8]), ('log_std/std', i[:, 9]), ('log_std/max', i[:, 10]),
                ('log_std/min', i[:, 11]), ('ratio/max', i[:, 5]), ('ratio/min', -i[:, 6]),
                ('grad_norm/pf', norms[:, 0].astype(np.float64)))
        if categorical:
            cols = tuple(c for c in cols if not c[0].startswith('log_std/'))
        keys = [k for k, _ in cols]
        table = np.stack([v for _, v in cols], axis=1).tolist()
        return [dict(zip(keys, row)) for row in table]


class _PendingInfos:
    """The K info dicts of a launched update sequence: `resolve()` waits for the statistics' D2H copy (an event, not the
    whole stream) and assembles them, once.  `land()` is the wait alone plus a snapshot of the page-locked block: the
    next run calls it before it reuses that block, and leaves the assembly of the dicts (~0.1 ms of host time) to whoever
    reads them -- after the next launch sequence is on its way instead of in front of it."""

    def __init__(self, count, landed, host, build):
        self.count, self._landed, self._host, self._build, self._snap, self._infos = count, landed, host, build, None, None

    def __len__(self):
        return self.count

    def land(self):
        if self._snap is None and self._infos is None:
            self._landed.synchronize()
            self._snap, self._host = self._host.clone(), None

    def resolve(self):
        if self._infos is None:
            self.land()
            self._infos, self._build, self._snap = self._build(self._snap), None, None
        return self._infos


_HEAD_OPT_IN = {HEAD_CAT: "TRL_CAT_FUSED_UPDATE", HEAD_SD: "TRL_SD_FUSED_UPDATE"}


def _head_spec(kind, ps):
    """(D, H, A, act) as the head's kernels count A: a [mean | log_std] head of width 2A has A action dimensions."""
    return (ps[0], ps[1], ps[2] // 2, ps[3]) if kind == HEAD_SD else tuple(ps)


def _fused_head_refusal(kind, ps):
    """Why the fused update does not carry a categorical / state-dependent-std policy of `_head_spec` ps here, or None."""
    if not getattr(_C.lib(), "trl_ppo_%ssupported" % HEAD_TAG[kind])(*ps):
        return "the fused %s update carries H == 64, 2 <= D <= 32, %d <= A <= 8, Tanh / ReLU; got %s" \
            % (HEAD_NAME[kind], 2 if kind == HEAD_CAT else 1, ps)
    if dist.collectives_active():
        return "the fused %s update runs on one rank (no cross-rank fold exists for this head)" % HEAD_NAME[kind]
    return None


def plain_layer_refusals(name, pf, vf, env):
    """What TRPO and V-MPO refuse before anything touches a device -- their engines walk the plain Linear + activation layer
    lists themselves, take the gathered-batch route over several ranks for the Gaussian head only, and read a categorical
    policy's actions as indices and a [mean | log_std] policy's as vectors, so the env's action space has to be of the head's
    kind.  Returns the head kind."""
    kind = head_kind(pf)
    for net in (pf, vf):
        if getattr(getattr(net, "base", None), "add_ln", False):
            raise _C.TrlError("%s does not carry LayerNorm nets (add_ln=True): its own passes walk Linear + activation layer "
                              "lists; PPO and A2C run them" % name)
    if kind in (HEAD_CAT, HEAD_SD) and dist.collectives_active():
        raise _C.TrlError("%s with a %s policy runs on one rank: the gathered-batch route over several ranks is exercised "
                          "for the Gaussian head only" % (name, HEAD_NAME[kind]))
    want = {HEAD_CAT: "Discrete", HEAD_SD: "Box"}.get(kind)
    space = getattr(env, "action_space", None)
    # (by what the space carries, not by its class: the CPU twins of the device envs bring Box classes of their own)
    have = None if space is None else ("Discrete" if hasattr(space, "n") else ("Box" if len(getattr(space, "shape", None) or ()) else None))
    if want is not None and have != want:
        raise _C.TrlError("%s with a %s policy is not built for %s: it takes an env whose action space is a %s"
                          % (name, HEAD_NAME[kind], "no env" if env is None else "the action space %r" % (space,), want))
    return kind


class _GenericPPO(_FusedPPO):
    defers = False                                                     # (its run returns the dicts)
    step_kinds = ("adam", "rmsprop", "sgd")                            # trl_clip_adam_f32 / trl_clip_step_f32 behind `run`
    carries_layernorm = True                                           # `add_ln` nets run here (ops.net_plan, k_layernorm.hip)
    """PPO / A2C minibatch loop for ARBITRARY MLP shapes (any observation / action size, width, depth): the layers run
    on the generic dense-layer kernels (k_gemm.hip, through ops.mlp_forward / mlp_backward), the loss half on
    trl_ppo_generic_losses_f32, clip + Adam on trl_clip_adam_f32.  Same interface, statistics block and info dicts
    as the fused engine, same per-sample arithmetic; ~25 launches per minibatch instead of 2 (TRL_GENERIC_PPO=1
    forces this engine for the benchmark shape too, which is how it is tested against the fused one)."""

    def sync_target_pf(self, in_prologue=False):
        super().sync_target_pf(False)                                  # (this engine's launch sequence has no fused prologue)

    def __init__(self, algo):
        from ... import ops
        self.algo, self.ops = algo, ops
        pf, vf = algo.pf, _critic(algo)
        # a vacant critic (vf None): `vf_layers` is empty -- no value forward, backward, pointers or optimiser group
        # a categorical head (policies.CategoricalDisPolicy): no logstd in the flat vector, trl_cat_losses_f32 for the loss half
        # a state-dependent-std head (policies.GuassianContPolicy): the network emits [mean | log_std]; no logstd in the flat
        # vector either, trl_gauss_sd_losses_f32 for the loss half, `self.A` = half the head's width
        self.head = head_kind(pf, refuse="PPO / A2C kernels need a GuassianContPolicyBasicBias, a GuassianContPolicy or a "
                                         "CategoricalDisPolicy")
        self.categorical, self.state_std = self.head == HEAD_CAT, self.head == HEAD_SD
        if self.state_std:
            head_w = int(ops.linear_layers(pf)[-1][0].shape[0])
            if not 1 <= head_w // 2 <= 32:
                raise _C.TrlError("a state-dependent-std policy emits [mean | log_std] with 1 <= A <= 32 action dimensions, "
                                  "got a head of %d" % head_w)
        if self.state_std and dist.collectives_active():
            raise _C.TrlError("PPO / A2C with a state-dependent-std policy runs on one rank (the per-element log_std "
                              "statistics have no cross-rank columns)")
        self.dev = next(pf.parameters()).device
        if self.dev.type != "cuda":
            raise _C.TrlError("PPO networks live on %s: the HIP path needs a GPU (no CPU path exists)" % self.dev)
        # `add_ln` nets: the layer lists carry their post-ops (ops.net_plan) and gamma / beta of every LayerNorm join the flat
        # vector, the gradient views and the Adam moments behind their layer's W, b; the two nets may differ in `add_ln`
        # (TRPO / V-MPO build on this engine and walk the plain layer lists themselves: they keep refusing LayerNorm nets)
        layers_of = ops.net_layers if self.carries_layernorm else (lambda net: (ops.linear_layers(net), ops.act_code(net)))
        (self.pf_layers, self.act), (self.vf_layers, vf_act) = layers_of(pf), ([], None) if vf is None else layers_of(vf)
        if vf is not None and vf_act != self.act:
            raise _C.TrlError("policy and value network must use the same activation")
        tail = (lambda net: []) if (self.categorical or self.state_std) else (lambda net: [net.logstd])
        pf_list = ops.plan_params(self.pf_layers) + tail(pf)
        vf_list = ops.plan_params(self.vf_layers)
        self.D, self.A = int(self.pf_layers[0][0].shape[1]), int(self.pf_layers[-1][0].shape[0])
        if self.state_std:
            self.A //= 2
        tgt = getattr(algo, "target_pf", None)
        self._home(pf_list, vf_list, None if tgt is None else ops.plan_params(layers_of(tgt)[0]) + tail(tgt))
        if tgt is not None and getattr(tgt, "mlp2_spec", lambda: None)() is not None:
            tgt._flat = self.target_flat                               # (same storage for its fused forward, as for pf / vf)
        self.gviews, off = [], 0
        for layers in (self.pf_layers, self.vf_layers):
            views = []
            for layer in layers:
                view = []
                for p in ops.plan_params([layer]):                     # W, b (, gamma, beta)
                    view.append(self.grads[off:off + p.numel()].view(p.shape)); off += p.numel()
                views.append(tuple(view))
            self.gviews.append(views)
            if layers is self.pf_layers and not self.categorical and not self.state_std:
                self.g_logstd = self.grads[off:off + self.A]; off += self.A
        self.step_state = torch.tensor([0.0, 1.0, 1.0, 0.0], dtype=torch.float64, device=self.dev)
        self.lr_dev = torch.zeros(2, device=self.dev)
        self._graphs, self._joint = GraphCache(4), None
        self.workspace = None

    def _spec(self):
        """The step as the policy's optimiser holds it now (Adam: the engine's own `eps`); which state buffers exist was
        settled at the home."""
        spec = _optim.step_spec(self.algo.pf_optimizer)
        if _optim.state_names(spec) != _optim.state_names(self.opt_spec):
            raise _C.TrlError("the optimiser's momentum / centered options changed after the engine was built")
        return ("adam", self.eps) if spec[0] == "adam" else spec

    def _ws(self, B):
        need = max(_C.lib().trl_linear_bwd_weight_workspace(B, int(w.shape[1]), int(w.shape[0]))
                   for w in (l[0] for l in self.pf_layers + self.vf_layers))
        if self.workspace is None or self.workspace.numel() < need:
            self.workspace = torch.empty(need, device=self.dev)
        return self.workspace

    def _losses(self, mean, acts, advs, old_lp, v, rets, v_old, raw_k, info_k, n_global, hyper):
        """The loss half of one minibatch on the head's kernel: (d loss / d head, d loss / d v).  `old_lp`, `v`, `rets` and
        `v_old` are None where the loss mode takes none; `hyper` is `_hyper(algo) + (loss_mode,)`."""
        flat = lambda x: None if x is None else x.view(-1)
        advs, old_lp, v, rets, v_old = flat(advs), flat(old_lp), flat(v), flat(rets), flat(v_old)
        if self.categorical:                                           # `mean` holds the logits, acts (n_local, 1) the indices
            return _C.cat_losses(mean, acts.view(-1), advs, old_lp, v, rets, v_old, raw_k, n_global, *hyper[:3], hyper[4], info_k)
        if self.state_std:                                             # `mean` holds the head [mean | log_std]
            return _C.gauss_sd_losses(mean, acts, advs, old_lp, v, rets, v_old, raw_k, n_global, *hyper, info_k)
        return _C.ppo_generic_losses(mean, self.algo.pf.logstd.detach(), acts, advs, old_lp, v, rets, v_old, raw_k, n_global,
                                     *hyper, self.g_logstd, info_k)

    def run(self, t, row_idx, N, pre=None, pre_key=None):
        algo, dev, ops = self.algo, self.dev, self.ops
        if self.one_rank and dist.collectives_active():
            raise _C.TrlError(self.one_rank)
        K, rows_mb = row_idx.shape
        world = dist.world_size()
        n_local = rows_mb * N
        n_global = float(n_local * world)
        idx_dev, stats = self._buffers(K, rows_mb)
        idx_dev.copy_(torch.from_numpy(np.ascontiguousarray(row_idx).reshape(-1)), non_blocking=True)
        rows_total = t["advs"].shape[0]
        raw, info, norms = _stat_views(stats, K)
        loss_mode = int(getattr(algo, "loss_mode", _C.LOSS_PPO_CLIP))
        ws = self._ws(n_local)
        idx2d = idx_dev.view(K, rows_mb)
        lrs = self._lrs()
        if getattr(self, "_lr_host", None) != lrs:                     # learning rates live on the device: the linear
            self._lr_host = lrs                                        # schedule changes no launch argument
            self.lr_dev.copy_(torch.tensor(lrs, dtype=torch.float32), non_blocking=True)
        gather = lambda key, k: None if t.get(key) is None else \
            _C.gather_rows(t[key].reshape(rows_total, N, -1), idx2d[k]).reshape(n_local, -1)
        hyper = _hyper(algo) + (loss_mode,)
        spec = self._spec()

        def launch_all():
            if pre is not None:
                pre()
            stats.zero_()
            _C.adv_stats(t["advs"].reshape(rows_total, N), idx2d, raw)
            dist.reduce_adv_raw_(raw)
            for k in range(K):
                obs, acts, advs, rets = gather("obs", k), gather("acts", k), gather("advs", k), gather("rets", k)
                v_old, old_lp = gather("old_values", k), gather("old_logp", k)
                mean, tape_pf = ops.mlp_forward(self.pf_layers, obs, self.act)
                v, tape_vf = ops.mlp_forward(self.vf_layers, obs, self.act) if self.vf_layers else (None, None)
                d_mean, d_v = self._losses(mean, acts, advs, old_lp, v, rets, v_old, raw[k], info[k], n_global, hyper)
                ops.mlp_backward(tape_pf, d_mean, grads=self.gviews[0], workspace=ws)
                if self.vf_layers:
                    ops.mlp_backward(tape_vf, d_v, grads=self.gviews[1], workspace=ws)
                dist.all_reduce_sum_(self.grads)                       # C1: gradient SUM over ranks
                _optim.clip_step(self._step_args(spec, norms_out=norms[k].data_ptr(), step_state=self.step_state.data_ptr(),
                                                 device_lr=self.lr_dev.data_ptr()), dev)  # device-side step count / lr

        # eager on the first visit of a configuration, captured into a HIP graph on the second, replayed afterwards
        key = (K, rows_mb, N, rows_total, n_global, idx_dev.data_ptr(), stats.data_ptr(), pre_key, pre is not None, spec) + hyper + tuple(
            0 if t.get(k_) is None else t[k_].data_ptr() for k_ in ("obs", "acts", "advs", "rets", "old_values", "old_logp"))
        self._graphs.run(key, launch_all)
        self._stepped(K)
        ent_sum = None
        if self.categorical and dist.collectives_active():             # slot 20 (entropy SUM) is not among the columns
            ent_sum = info[:, 20].contiguous()                         # reduce_info_ sums: its own all-reduce, put back below
            dist.all_reduce_sum_(ent_sum)
        dist.reduce_info_(info)
        if ent_sum is not None:
            info[:, 20] = ent_sum
        host = stats.cpu()                                             # the only host sync of the update
        return self._info_builder(loss_mode)(*(v.numpy() for v in _stat_views(host, K)), n_global)


def make_engine(algo, fused=_FusedPPO, generic=_GenericPPO):
    """The `fused` engine when the networks -- the policy and, unless the critic is vacant, the value function -- have the
    shape its kernels are instantiated for, the `generic` one otherwise."""
    pf, vf = algo.pf, _critic(algo)
    ps = pf.mlp2_spec() if hasattr(pf, "mlp2_spec") else None
    vs = vf.mlp2_spec() if hasattr(vf, "mlp2_spec") else None
    blocks = ps is not None and (vf is None or vs is not None)         # every network there is is an MLP2 block
    forced = os.environ.get("TRL_GENERIC_PPO") == "1"
    kind = head_kind(pf)
    opt = getattr(algo, "pf_optimizer", None)
    if opt is not None and type(opt) is not optim.Adam:
        return generic(algo)                                           # RMSprop / SGD: the fused fold / clip / Adam launches are Adam's
    if kind in _HEAD_OPT_IN:
        # categorical / [mean | log_std] head: the generic engine, unless the fused update is asked for (TRL_CAT_FUSED_UPDATE=1 /
        # TRL_SD_FUSED_UPDATE=1, opt-in) AND the nets have a shape the head's instantiations carry, the optimiser is Adam and
        # this is the only rank
        if os.environ.get(_HEAD_OPT_IN[kind]) == "1" and not forced and blocks \
                and _fused_head_refusal(kind, _head_spec(kind, ps)) is None \
                and (vf is None or tuple(vs) == (ps[0], ps[1], 1, ps[3])) and getattr(algo, "optimizer_class", None) is optim.Adam:
            return fused(algo)
        return generic(algo)
    if blocks and hasattr(pf, "logstd") and _C.lib().trl_ppo_partial_stride(ps[0], ps[1], ps[2]) > 0 and not forced:
        return fused(algo)
    return generic(algo)
