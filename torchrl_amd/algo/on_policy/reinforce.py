"""REINFORCE (torchrl/algo/on_policy/reinforce.py:7-81): a policy, its one Adam optimiser (torch's default eps 1e-8,
no learning-rate schedule), a vacant critic (`networks.ZeroNet`, V == 0) and plain discounted returns (`gae = False`).

`update(batch)` is L = mean(-log pi(a|s) * adv_normalised) - c_ent * mean(ent), clip_grad_norm_(0.5), one Adam step
(reinforce.py:33-75) -- the policy half of the A2C launch sequence with `loss_mode = TRL_LOSS_REINFORCE`: no value
forward, no value loss, no value reduction, one optimiser group.  `update_per_epoch` keeps OnRLAlgo's single pass of
`one_iteration` minibatches (on_rl_algo.py:35-40), through the row indices on the device-resident buffer.

The two engines are the policy-only forms of algo/on_policy/ppo.py's: `_FusedReinforce` (64-wide two-layer shapes of
the fused gradient kernel: one all-policy gradient launch + the policy's fold / clip / Adam launch per minibatch,
graph-replayed) and `_GenericReinforce` (any MLP, `add_ln` included, on the dense-layer kernels).  Routing mirrors
`ppo.make_engine`.  With V == 0 the rollout needs no value pass either: the collector stores zeros (one launch on the
fused route, trl_rollout_t.vf_params = NULL) and `advs == estimate_returns`."""
import math
import os

import numpy as np
import torch
import torch.optim as optim

from ... import _C
from ... import dist
from ...networks import ZeroNet, flatten_into
from ...policies.continuous_policy import HEAD_CAT, HEAD_GAUSS, HEAD_NAME, HEAD_SD, HEAD_TAG, head_kind
from .._graphs import GraphCache, LastGraph
from .a2c import A2C
from .on_rl_algo import OnRLAlgo
from .ppo import (_FusedPPO, _GenericPPO, _HEAD_OPT_IN, _HALF_LOG_2PI_PLUS_HALF, _PendingInfos, _fused_head_refusal,
                  _head_spec, _hyper, _stat_views)

_ONE_RANK = "Reinforce runs on one rank (several ranks are not built: no cross-rank fold of a policy-only update exists)"


class Reinforce(OnRLAlgo):
    loss_mode = _C.LOSS_REINFORCE
    sample_key = ("obs", "acts", "advs")

    def __init__(self, pf=None, plr=None, optimizer_class=optim.Adam, entropy_coeff=0.001, **kwargs):
        if pf is None or plr is None:
            raise _C.TrlError("Reinforce without a policy (`pf`, `plr`) is not built: pass the policy network and its "
                              "learning rate (reference: torchrl/algo/on_policy/reinforce.py)")
        super().__init__(**kwargs)
        self.pf = pf
        self.vf = ZeroNet()                                            # a vacant critic keeps the collector's interface
        self.to(self.device)
        self.plr = plr
        self.optimizer_class = optimizer_class
        self.pf_optimizer = optimizer_class(self.pf.parameters(), lr=self.plr)
        self.entropy_coeff = entropy_coeff
        self.gae = False
        self._engine = None

    def engine(self):
        if self._engine is None:
            if self.optimizer_class is not optim.Adam:
                raise _C.TrlError("the Reinforce step implements torch.optim.Adam only")
            self._engine = make_engine(self)
        return self._engine

    _run_and_log = A2C._run_and_log

    def update_per_epoch(self):
        self.process_epoch_samples()
        buf = self.replay_buffer
        row_idx = buf.epoch_row_indices(self.batch_size, self.shuffle)      # one pass (on_rl_algo.py:37-40)
        tensors = {"obs": buf._obs, "acts": buf._acts, "advs": buf._advs}
        self._run_and_log(tensors, row_idx, buf.env_nums)

    def update(self, batch):
        self.training_update_num += 1
        dev = self.device
        as_t = lambda x: (x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))) \
            .to(device=dev, dtype=torch.float32).contiguous()
        obs, acts = as_t(batch['obs']), as_t(batch['acts'])
        B = obs.shape[0]
        tensors = {"obs": obs.reshape(1, B, -1), "acts": acts.reshape(1, B, -1), "advs": as_t(batch['advs']).reshape(1, B, 1)}
        return self.engine().run(tensors, np.zeros((1, 1), dtype=np.int64), B)[0]

    @property
    def snapshot_networks(self):
        return [("pf", self.pf)]


def make_engine(algo):
    """ppo.make_engine for one network: the fused engine for the shared-std Gaussian shapes of the fused gradient kernel
    (and, under their opt-ins, the categorical / state-dependent-std ones), the generic engine otherwise."""
    if dist.collectives_active() or dist.world_size() > 1:
        raise _C.TrlError(_ONE_RANK)
    pf = algo.pf
    ps = pf.mlp2_spec() if hasattr(pf, "mlp2_spec") else None
    kind = head_kind(pf)
    generic = os.environ.get("TRL_GENERIC_PPO") == "1"
    if kind in _HEAD_OPT_IN:
        if os.environ.get(_HEAD_OPT_IN[kind]) == "1" and not generic and ps is not None \
                and _fused_head_refusal(kind, _head_spec(kind, ps)) is None:
            return _FusedReinforce(algo)
        return _GenericReinforce(algo)
    if ps is not None and hasattr(pf, "logstd") and _C.lib().trl_ppo_partial_stride(ps[0], ps[1], ps[2]) > 0 and not generic:
        return _FusedReinforce(algo)
    return _GenericReinforce(algo)


def _infos_reinforce(engine, raw, info, n):
    """The info dict of Reinforce.update (reinforce.py:42-73), in its order.  `advs/*` are numpy statistics of the float64
    batch there, so `advs/std` is the POPULATION std (A2C / PPO log torch's unbiased one); `logprob/std` is unbiased."""
    c_ent = float(engine.algo.entropy_coeff)
    out = []
    for r, i in zip(raw, info):
        adv_var = max((r[1] - r[0] * r[0] / n) / n, 0.0)
        lp_var = max((i[2] - i[1] * i[1] / n) / (n - 1), 0.0)
        ent = i[20] / n if (engine.categorical or engine.state_std) else \
            engine.A * _HALF_LOG_2PI_PLUS_HALF + engine.A * i[8]
        out.append({'advs/mean': r[0] / n, 'advs/std': math.sqrt(adv_var), 'advs/max': r[2], 'advs/min': -r[3],
                    'Training/policy_loss': i[0] / n - c_ent * ent, 'ent': ent,
                    'logprob/mean': i[1] / n, 'logprob/std': math.sqrt(lp_var), 'logprob/max': i[3], 'logprob/min': -i[4]})
    return [{k: float(v) for k, v in d.items()} for d in out]


class _PolicyOnly:
    """What the two engines share: ONE network in the flat buffers -- `flat` = [pf (| logstd)], `P_vf = 0` --, one
    optimiser group whose eps is the optimiser's own (torch's 1e-8: reinforce.py:25-28 passes none), no value chain."""

    def _home(self, pf_list, vf_list, target_list):
        assert not vf_list and target_list is None
        self.P_pf, self.P_vf = sum(p.numel() for p in pf_list), 0
        self.flat = flatten_into(pf_list)
        if getattr(self.algo.pf, "mlp2_spec", lambda: None)() is not None:
            self.algo.pf._flat = self.flat                              # (its fused forward must find THIS storage)
        self.m, self.v, self.grads = torch.zeros_like(self.flat), torch.zeros_like(self.flat), torch.zeros_like(self.flat)
        self.step_count = 0
        self.target_flat = None
        self._alias_optimizer_state(self.algo.pf_optimizer, pf_list, 0)

    def _adam_args(self, lrs=(0.0,), **kw):
        """clip_grad_norm_(0.5) + Adam over the policy's single group of the flat buffers."""
        eps = float(self.algo.pf_optimizer.param_groups[0]['eps'])
        return _C.adam_args(self.flat, self.grads, self.m, self.v, (self.P_pf,), lrs[:1], max_norm=0.5, eps=eps, **kw)

    def _infos_reinforce(self, raw, info, norms, n):
        return _infos_reinforce(self, raw, info, n)


class _FusedReinforce(_PolicyOnly, _FusedPPO):
    """Per minibatch two launches: the all-policy gradient launch (trl_ppo_*minibatch_grad_f32, n_wg_pf == n_wg,
    TRL_LOSS_REINFORCE: no returns, old values, log pi_old or value parameters) and the policy's fold / clip / Adam
    (trl_ppo_*reduce_adam_net_f32, net 0, one optimiser group).  The epoch's sequence -- prologue launch, K x the two --
    is captured into a HIP graph on the second visit of a shape and replayed afterwards, like `_FusedPPO.run`'s."""

    def __init__(self, algo):
        self.algo = algo
        pf = algo.pf
        ps = pf.mlp2_spec()
        needs = "fused Reinforce needs an MLP2 GuassianContPolicyBasicBias, GuassianContPolicy or CategoricalDisPolicy policy"
        if ps is None:
            raise _C.TrlError(needs)
        self.head = head_kind(pf, refuse=needs)
        self.categorical, self.state_std = self.head == HEAD_CAT, self.head == HEAD_SD
        if self.head != HEAD_GAUSS:
            ps = _head_spec(self.head, ps)
            why = _fused_head_refusal(self.head, ps)
            if why:
                raise _C.TrlError(why)
        self.D, self.H, self.A, self.act = ps
        self.dev = next(pf.parameters()).device
        if self.dev.type != "cuda":
            raise _C.TrlError("Reinforce networks live on %s: the fused path needs a GPU (no CPU path exists)" % self.dev)
        tail = [] if (self.categorical or self.state_std) else [pf.logstd]
        self._home(pf._mlp2_param_list() + tail, [], None)
        lib = _C.lib()
        sfx = HEAD_TAG[self.head]
        kernel = lambda name: (getattr(lib, name), name)
        self._k_grad = kernel("trl_ppo_%sminibatch_grad_f32" % sfx)
        self._k_fold_net = kernel("trl_ppo_%sreduce_adam_net_f32" % sfx)
        self.p_stride = getattr(_C, "ppo_%spartial_stride" % sfx)(self.D, self.H, self.A)
        if self.p_stride <= 0:
            raise _C.TrlError("fused Reinforce: shape %s is not instantiated in the gradient kernel" % (ps,))
        self.scal_w = _C.ppo_sd_scalar_stride() if self.state_std else 8
        self.n_cu = torch.cuda.get_device_properties(self.dev).multi_processor_count
        self.max_wg = 2 * max(1, self.n_cu // 2)
        self.partial = torch.zeros(self.max_wg, self.p_stride, device=self.dev)
        self.scal = torch.zeros(self.max_wg, self.scal_w, dtype=torch.float64, device=self.dev)
        n_ws = getattr(lib, "trl_ppo_%sreduce_adam_workspace" % sfx)(self.D, self.H, self.A)
        self.red_ws = torch.zeros(n_ws, device=self.dev)              # Adam header + norm granules of the fold launch
        self.red_ws[4:8].view(torch.float64).fill_(1.0)               # beta1^0, beta2^0 (device-side Adam state)
        self._joint = LastGraph()
        self._pending = None
        self._pro_ws = None

    def _n_wg(self, n_samples):
        """Workgroups of one minibatch's gradient launch, all of them the policy's: one 16-sample tile per wave while the
        chip has room."""
        tiles = (n_samples + 15) // 16
        return max(1, min(self.max_wg, (tiles + 3) // 4))

    def sync_target_pf(self, in_prologue=False):
        raise _C.TrlError("Reinforce has no target policy")

    def run(self, t, row_idx, N, pre=None, pre_key=None, defer=False):
        """K minibatch updates back to back; returns K info dicts (one host wait at the end), or with `defer=True` a
        `_PendingInfos` right after the launches.  See `_FusedPPO.run`."""
        algo, dev = self.algo, self.dev
        if dist.collectives_active():
            raise _C.TrlError(_ONE_RANK)
        K, rows_mb = row_idx.shape
        n_local = rows_mb * N
        n_global = float(n_local)
        n_wg = self._n_wg(n_local)
        if self._pending is not None:                                  # its statistics still sit in the host twin this run
            self._pending.land()                                       # is about to reuse
            self._pending = None
        idx_dev, stats = self._buffers(K, rows_mb)
        self._idx_host.numpy()[:] = row_idx.reshape(-1)
        rows_total = t["advs"].shape[0]
        raw, info, norms = _stat_views(stats, K)
        lr_pf = float(algo.pf_optimizer.param_groups[0]['lr'])
        self._set_device_hyper(lr_pf, 0.0, upload=False)               # (the prologue launch copies the slab in place)
        hyper = _hyper(algo)
        use_graph = os.environ.get("TRL_NO_GRAPH") != "1"
        key = (n_wg, n_global, rows_total, N, pre_key, pre is not None) + hyper + tuple(
            t[k].data_ptr() for k in ("obs", "acts", "advs"))

        def launch_all():
            g = self._batch_args(t, hyper, _C.LOSS_REINFORCE, rows_mb, N, n_global, self.partial, self.scal, n_wg, n_wg)
            g.vf_params = None
            a = self._adam_args((lr_pf,), device_state=1)              # step count / lr from the workspace header
            slab = [(idx_dev, self._idx_host), (self.red_ws[2:4], self._hyper_host)]
            self._prologue(pre, t["advs"].reshape(rows_total, N), self._idx_host.view(K, rows_mb), raw, stats[4 * K:], slab)
            fold = self._fold(self._k_fold_net, self.partial, self.scal, n_wg, 0, info, self.red_ws)
            self._minibatches(K, g, a, idx_dev, raw, norms, fold)

        self._joint.run(key, launch_all, eager=not use_graph)
        self._stats_host.copy_(stats, non_blocking=True)
        landed = torch.cuda.Event()
        landed.record()
        self._stepped(K)
        build = lambda host: _infos_reinforce(self, *(v.numpy() for v in _stat_views(host, K)[:2]), n_global)
        pending = _PendingInfos(K, landed, self._stats_host, build)
        if defer:
            self._pending = pending
            return pending
        return pending.resolve()                                       # the only host wait of the update


class _GenericReinforce(_PolicyOnly, _GenericPPO):
    """The minibatch loop for ARBITRARY policy MLPs (`add_ln` included): the layers on the dense-layer kernels, the loss
    half on trl_ppo_generic_losses_f32 / trl_cat_losses_f32 / trl_gauss_sd_losses_f32 in TRL_LOSS_REINFORCE mode (no value
    pointers), clip + Adam on trl_clip_adam_f32 with one group."""

    def __init__(self, algo):
        from ... import ops
        self.algo, self.ops = algo, ops
        pf = algo.pf
        self.head = head_kind(pf, refuse="Reinforce kernels need a GuassianContPolicyBasicBias, a GuassianContPolicy or a "
                                         "CategoricalDisPolicy")
        self.categorical, self.state_std = self.head == HEAD_CAT, self.head == HEAD_SD
        if self.state_std:
            head_w = int(ops.linear_layers(pf)[-1][0].shape[0])
            if not 1 <= head_w // 2 <= 32:
                raise _C.TrlError("a state-dependent-std policy emits [mean | log_std] with 1 <= A <= 32 action dimensions, "
                                  "got a head of %d" % head_w)
        self.dev = next(pf.parameters()).device
        if self.dev.type != "cuda":
            raise _C.TrlError("Reinforce networks live on %s: the HIP path needs a GPU (no CPU path exists)" % self.dev)
        self.pf_layers, self.act = ops.net_layers(pf)
        self.vf_layers = []
        tail = [] if (self.categorical or self.state_std) else [pf.logstd]
        self.D, self.A = int(self.pf_layers[0][0].shape[1]), int(self.pf_layers[-1][0].shape[0])
        if self.state_std:
            self.A //= 2
        self._home(ops.plan_params(self.pf_layers) + tail, [], None)
        views, off = [], 0
        for layer in self.pf_layers:
            view = []
            for p in ops.plan_params([layer]):                         # W, b (, gamma, beta)
                view.append(self.grads[off:off + p.numel()].view(p.shape)); off += p.numel()
            views.append(tuple(view))
        self.gviews = [views]
        if tail:
            self.g_logstd = self.grads[off:off + self.A]
        self.step_state = torch.tensor([0.0, 1.0, 1.0, 0.0], dtype=torch.float64, device=self.dev)
        self.lr_dev = torch.zeros(1, device=self.dev)
        self._graphs, self._joint = GraphCache(4), None
        self.workspace = None

    def sync_target_pf(self, in_prologue=False):
        raise _C.TrlError("Reinforce has no target policy")

    def run(self, t, row_idx, N, pre=None, pre_key=None):
        algo, dev, ops = self.algo, self.dev, self.ops
        if dist.collectives_active():
            raise _C.TrlError(_ONE_RANK)
        K, rows_mb = row_idx.shape
        n_local = rows_mb * N
        n_global = float(n_local)
        idx_dev, stats = self._buffers(K, rows_mb)
        idx_dev.copy_(torch.from_numpy(np.ascontiguousarray(row_idx).reshape(-1)), non_blocking=True)
        rows_total = t["advs"].shape[0]
        raw, info, norms = _stat_views(stats, K)
        ws = self._ws(n_local)
        idx2d = idx_dev.view(K, rows_mb)
        lr = float(algo.pf_optimizer.param_groups[0]['lr'])
        if getattr(self, "_lr_host", None) != lr:                      # the learning rate lives on the device
            self._lr_host = lr
            self.lr_dev.copy_(torch.tensor([lr], dtype=torch.float32), non_blocking=True)
        gather = lambda key, k: _C.gather_rows(t[key].reshape(rows_total, N, -1), idx2d[k]).reshape(n_local, -1)
        c_ent, tanh = float(algo.entropy_coeff), int(bool(algo.pf.tanh_action))
        mode = _C.LOSS_REINFORCE

        def launch_all():
            if pre is not None:
                pre()
            stats.zero_()
            _C.adv_stats(t["advs"].reshape(rows_total, N), idx2d, raw)
            for k in range(K):
                obs, acts, advs = gather("obs", k), gather("acts", k), gather("advs", k)
                mean, tape_pf = ops.mlp_forward(self.pf_layers, obs, self.act)
                if self.categorical:                                   # `mean` holds the logits, acts (n_local, 1) the indices
                    d_mean, _ = _C.cat_losses(mean, acts.view(-1), advs.view(-1), None, None, None, None, raw[k], n_global,
                                              0.0, c_ent, 0, mode, info[k])
                elif self.state_std:                                   # `mean` holds the head [mean | log_std]
                    d_mean, _ = _C.gauss_sd_losses(mean, acts, advs.view(-1), None, None, None, None, raw[k], n_global,
                                                   0.0, c_ent, 0, tanh, mode, info[k])
                else:
                    d_mean, _ = _C.ppo_generic_losses(mean, algo.pf.logstd.detach(), acts, advs.view(-1), None, None, None,
                                                      None, raw[k], n_global, 0.0, c_ent, 0, tanh, mode, self.g_logstd,
                                                      info[k])
                ops.mlp_backward(tape_pf, d_mean, grads=self.gviews[0], workspace=ws)
                _C.clip_adam(self._adam_args(norms_out=norms[k].data_ptr(), step_state=self.step_state.data_ptr(),
                                             device_lr=self.lr_dev.data_ptr()), dev)     # device-side step count / lr

        # eager on the first visit of a configuration, captured into a HIP graph on the second, replayed afterwards
        key = (K, rows_mb, N, rows_total, n_global, idx_dev.data_ptr(), stats.data_ptr(), pre_key, pre is not None, c_ent,
               tanh) + tuple(t[k_].data_ptr() for k_ in ("obs", "acts", "advs"))
        self._graphs.run(key, launch_all)
        self._stepped(K)
        host = stats.cpu()                                             # the only host sync of the update
        return _infos_reinforce(self, *(v.numpy() for v in _stat_views(host, K)[:2]), n_global)
