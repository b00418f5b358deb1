"""DQN and QR-DQN on the HIP path (torchrl/algo/off_policy/dqn.py:9-92, qrdqn.py:11-74).

`update(batch)`: Q(s) and Q'(s') through the conv + dense kernels (uint8 frame stacks are read
as stored and scaled in the first im2col), the TD / quantile-Huber loss kernel returns the loss
sums and dL/dQ, the backward pass fills one flat gradient buffer, trl_clip_adam_f32 steps it,
trl_polyak_f32 (soft) or a full copy every `target_hard_update_period` updates the target net.
Actions are read as (B,) or (B, 1) floats as the replay buffer stores them and cast to an index inside the
loss launch (the reference's two classes disagree on the shape, its Q16).
"""
import copy

import numpy as np
import torch
import torch.optim as optim

from ... import _C, dist, ops
from .. import _optim
from ._deferred import IndexSlab, StatRing
from ._engine import FlatHome, GraphCache, _EngineSurface, _FusedOffPolicy, load_static, net_home
from .off_rl_algo import OffRLAlgo


class DQN(_EngineSurface, OffRLAlgo):
    quantile_num = 1

    def __init__(self, qf, pf, qlr, optimizer_class=optim.Adam, optimizer_info={}, **kwargs):
        super().__init__(**kwargs)
        self.pf = pf
        self.qf = qf
        self.target_qf = copy.deepcopy(qf)
        self.qlr = qlr
        self.optimizer_class = optimizer_class
        self.optimizer_info = dict(optimizer_info)
        self.qf_optimizer = optimizer_class(self.qf.parameters(), lr=self.qlr, **optimizer_info)
        self.to(self.device)
        self._engine = None

    @property
    def networks(self):
        return [self.qf, self.target_qf]

    @property
    def target_networks(self):
        return [(self.qf, self.target_qf)]

    @property
    def snapshot_networks(self):
        return [("pf", self.qf)]

    def engine(self):
        if self._engine is None:
            self._engine = _FusedDQN(self)
        return self._engine


class QRDQN(DQN):
    def __init__(self, quantile_num=100, **kwargs):
        super().__init__(**kwargs)
        self.quantile_num = quantile_num


class _FusedDQN(_FusedOffPolicy):
    def __init__(self, algo):
        self.algo = algo
        self.dev = next(algo.qf.parameters()).device
        if self.dev.type != "cuda":
            raise _C.TrlError("DQN networks live on %s: the HIP path needs a GPU (no CPU path exists)" % self.dev)
        from ...networks.base import MLPBase
        self.is_mlp = isinstance(algo.qf.base, MLPBase)                 # state-vector Q net (examples/dqn_state_vec.py)
        if self.is_mlp:
            # an `add_ln` Q net: its plan with the LayerNorms (ops.net_layers), gamma / beta homed behind their layer's W, b
            (self.layers,), (self.tlayers,), self.act, home = net_home([("qf", algo.qf)], [("target_qf", algo.target_qf)],
                                                                       [algo.qf_optimizer])
            self.gviews = home.layer_views([self.layers])[0]
        else:
            plist, tlist = ops.cnn_param_list(algo.qf), ops.cnn_param_list(algo.target_qf)
            home = FlatHome([plist], [algo.qf_optimizer], tlist)
            self.gviews = home.pairs()[0]
        self.flat, self.tflat, self.grads, self.m, self.v = home.flat, home.tflat, home.grads, home.m, home.v
        self.opt_spec, self.c = home.specs[0], home.c                     # (the whole of `optimizer_info`, as torch read it)
        self.A = int(algo.env.action_space.n)
        self._init_run_state()

    def _init_run_state(self):
        """What `enqueue` / `enqueue_epoch` / `resolve` / `_run` keep between updates, whatever the network is (the
        Bootstrapped DQN engine builds its own parameter buffers and calls this too)."""
        algo = self.algo
        self.step_count = 0
        self.sums = torch.zeros(3, dtype=torch.float64, device=self.dev)
        self.workspace = None
        # update u's three sums are filed into ring row u % slots by its loss launch (one rank), or copied there
        self._ring = StatRing(max(64, int(getattr(algo, "opt_times", 1))), 3, torch.float64, self.dev)
        self._slab = IndexSlab(self.dev)
        self._static, self._graphs = None, GraphCache(4)
        self.step_state = torch.tensor([0.0, 1.0, 1.0, 0.0], dtype=torch.float64, device=self.dev)
        self._head_ws = None                                            # workspace of the one-launch head (conv nets, Q = 1)

    def resolve(self, handles):
        """Info dicts of enqueued updates, in order, after one D2H per ring of loss sums (the only host sync)."""
        rows = self._ring.read([(h[0], h[1]) for h in handles]).tolist()
        return [{'Reward_Mean': s[2] / B, 'Training/qf_loss': s[0] / denom, 'epsilon': eps, 'q_s_a': s[1] / (B * Q)}
                for s, (_, _, B, denom, Q, eps) in zip(rows, handles)]

    def static_batch(self, B=None):
        """Fixed-address input tensors of an update (None until the first batch has shown the shapes, whatever `B`): the
        replay gather writes straight into them (`random_batch(..., out=)`) and the captured launch sequence reads them."""
        return self._static

    def _load(self, batch):
        dev = self.dev
        obs = batch['obs']
        if not self.is_mlp and not (isinstance(obs, torch.Tensor) and obs.dtype == torch.uint8):
            raise _C.TrlError("DQN.update expects uint8 (B, C, H, W) frame stacks from the device replay buffer")
        want = torch.uint8 if not self.is_mlp else torch.float32
        B = int(obs.shape[0])
        st = self._static
        if st is None or int(st["obs"].shape[0]) != B:
            shape = tuple(int(v) for v in (obs.shape if isinstance(obs, torch.Tensor) else np.asarray(obs).shape))
            f = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=dev)
            st = {"obs": torch.zeros(shape, dtype=want, device=dev), "next_obs": torch.zeros(shape, dtype=want, device=dev),
                  "acts": f(B, 1), "rewards": f(B, 1), "terminals": f(B, 1)}
            st.update(self._extra_static(B))
            self._static = st
            self._graphs.clear()                                         # (they read the old tensors)
        load_static(st, batch, self.KEYS)
        return st, B

    def _extra_static(self, B):
        return {}

    def _sequence(self, st, soft):
        """The fixed launch sequence of one update on the static inputs (eager, or under graph capture)."""
        algo, dev = self.algo, self.dev
        obs, nobs = st["obs"], st["next_obs"]
        rew, term = st["rewards"].view(-1), st["terminals"].view(-1)
        acts = st["acts"].view(-1)                                       # floats as stored; the loss launch casts at the read
        ring = (self._ring.t, self.step_state) if dist.world_size() == 1 else None    # (else: copied after the all-reduce)
        B, A, Q = int(obs.shape[0]), self.A, int(algo.quantile_num)
        pair = None
        if self.is_mlp:
            q, tape = ops.mlp_forward(self.layers, obs, self.act)
            qn, _ = ops.mlp_forward(self.tlayers, nobs, self.act)
        else:
            # online net on obs and target net on next_obs: one grouped launch per layer after the first
            (hw, hb), (tw, tb) = ops.fc_layers(algo.qf)[-1], ops.fc_layers(algo.target_qf)[-1]
            if Q == 1 and hb is not None and _C.dqn_head_supported(int(hw.shape[1]), A) and \
                    hw.data_ptr() % 16 == 0 and tw.data_ptr() % 16 == 0:
                pair = ops.cnn_forward_pair(algo.qf, algo.target_qf, obs, nobs, head=False, dx_prep=True)
            if pair is None:
                (q, tape), (qn, _) = ops.cnn_forward_pair(algo.qf, algo.target_qf, obs, nobs, dx_prep=True)
        if pair is not None:
            # the A-wide head: both forward passes, the loss and its whole backward pass in one launch
            (h, tape), (hn, _) = pair
            if self._head_ws is None:
                self._head_ws = _C.dqn_head_workspace(int(hw.shape[1]), A, dev)
            gw, gb = self.gviews[-1]
            dq = _C.dqn_head(h, hn, hw, hb, tw, tb, acts, rew, term, algo.discount, gw, gb, self.sums, self._head_ws,
                             ring=ring)                                  # = d loss / d h
        elif Q == 1:
            dq = _C.dqn_td_loss(q, acts, qn, rew, term, algo.discount, self.sums, ring=ring)
        else:
            dq = _C.quantile_huber(q, acts, qn, rew, term, algo.discount, A, Q, self.sums, ring=ring)
        if self.is_mlp:
            need = max(_C.lib().trl_linear_bwd_weight_workspace(B, int(l[0].shape[1]), int(l[0].shape[0])) for l in self.layers)
        else:
            need = ops.cnn_backward_workspace(tape)                          # every conv layer its own region (one fold launch)
            need = max(need, max(_C.lib().trl_linear_bwd_weight_workspace(B, int(w.shape[1]), int(w.shape[0]))
                                 for w, _ in ops.fc_layers(algo.qf)))
        if self.workspace is None or self.workspace.numel() < need:
            self.workspace = torch.empty(need, device=dev)
        if self.is_mlp:
            ops.mlp_backward(tape, dq, grads=self.gviews, workspace=self.workspace)
        else:
            ops.cnn_backward(algo.qf, tape, dq, self.gviews, workspace=self.workspace)
        dist.all_reduce_sum_(self.grads)                                 # C1: local-mean gradients -> SUM / world
        self._adam_polyak(soft, 1.0 / dist.world_size())
        dist.all_reduce_sum_(self.sums)

    def _adam_polyak(self, soft, grad_scale):
        """The optimiser's step (Adam, RMSprop or SGD: `_optim.step_spec`) over the whole flat buffer, then Polyak when
        `soft` (which also advances the step state)."""
        algo = self.algo
        a = _optim.step_args(self._spec(), self.flat, self.grads, (self.m, self.v, self.c), [self.flat.numel()],
                             [algo.qf_optimizer.param_groups[0]['lr']], grad_scale=grad_scale,
                             step_state=self.step_state.data_ptr())
        if soft:
            _optim.clip_step_polyak(a, self.tflat, self.flat, algo.tau, self.dev)
        else:
            _optim.clip_step(a, self.dev)

    def _spec(self):
        """The step's hyper-parameters as the optimiser holds them now; which state buffers exist was settled at the home."""
        spec = _optim.step_spec(self.algo.qf_optimizer)
        if _optim.state_names(spec) != _optim.state_names(self.opt_spec):
            raise _C.TrlError("the optimiser's momentum / centered options changed after the engine was built")
        return spec

    def _epoch_key(self, soft):
        """What a captured launch sequence has baked in, beside its shapes."""
        algo = self.algo
        return (soft, float(algo.qf_optimizer.param_groups[0]['lr']), float(algo.discount), float(algo.tau),
                int(algo.quantile_num), self._spec())

    def enqueue(self, batch):
        """Launch one update without waiting for it; its loss sums wait in their ring row for `resolve`."""
        algo = self.algo
        st, B = self._load(batch)
        soft = bool(algo.use_soft_update)
        self._ring.make_room(1)
        self._graphs.run((B,) + self._epoch_key(soft), lambda: self._sequence(st, soft))
        self.step_count += 1
        if not soft and algo.training_update_num % algo.target_hard_update_period == 0:
            _C.polyak(self.tflat, self.flat, 1.0)
        handle = self._handles(1, B)[0]
        if dist.world_size() > 1:
            self._ring.t[handle[1]].copy_(self.sums, non_blocking=True)
        return handle

    def _handles(self, count, B):
        algo, world = self.algo, dist.world_size()
        Q = int(algo.quantile_num)
        denom = (float(B) if Q == 1 else float(B) * Q * Q) * world
        return [(ref, row, B * world, denom, Q, algo.pf.epsilon)
                for ref, row in self._ring.handles(self.step_count - count, count)]

    def _epoch_declined(self, count):
        """Whole epochs need one rank, an update seen at this batch size and no hard target copy due inside the epoch."""
        algo, st = self.algo, self._static
        period, done = int(algo.target_hard_update_period), int(algo.training_update_num)
        return st is None or dist.world_size() != 1 or int(st["obs"].shape[0]) != int(algo.batch_size) or \
            (not algo.use_soft_update and any((done + j) % period == 0 for j in range(1, count + 1)))
