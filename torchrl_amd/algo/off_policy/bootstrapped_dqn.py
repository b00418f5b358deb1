"""Bootstrapped DQN on the HIP path (torchrl/algo/off_policy/bootstrapped_dqn.py:7-104).

K Q heads on one MLP trunk (`networks.BootstrappedNet`); every stored transition carries a Bernoulli(p) mask per head
(drawn by the collector, trl_boot_masks_f32) and head k learns from the transitions whose mask k is set:

    loss = mean_b sum_k masks[b, k] (Q_k(s_b)[a_b] - (r_b + gamma (1 - d_b) max_a' Q'_k(s'_b)[a']))^2 / K

`update(batch)`: the trunk once per network, all K heads as ONE grouped launch per head level (online on obs, target on
next_obs) writing head-major (K, B, A) stacks, trl_boot_td_loss_f32 for the loss sums and dL/dQ, the heads' backward
pass as one grouped weight- and one grouped input-gradient launch per level, trl_boot_fold_f32 to sum the K gradients at
the trunk feature, the trunk's backward pass, then Adam (+ Polyak) over ONE flat buffer of trunk and heads, as DQN does.
The launch count does not grow with K up to 12 heads, the most problems one grouped dense-layer launch carries
(_C.GROUP_MAX); beyond, each grouped launch of the heads becomes ceil(K / 12) launches.  The reference does not detach the target; that only reaches the target net's
unused gradients.

Scope: MLP trunks, one rank, Adam; 1 <= K <= 64 heads and 1 <= A <= 64 actions.  Everything else raises _C.TrlError.

TRL_BOOT_CONV=1 (opt-in, `ops.boot_conv`; read in `engine()`): conv trunks (a `BootstrappedNet` over a CNNBase, uint8 frame
batches) and `torch.optim.RMSprop` / `torch.optim.SGD` beside Adam, for MLP and conv trunks alike (`_optim.step_spec`, the
step of `_FusedDQN._adam_polyak`).  Over a conv trunk the update is DQN's paired conv forward up to the flattened feature
(online on obs, target on next_obs), heads / loss / head weight gradients as above, then the heads' input gradient at the
feature -- summed over the K heads, gated by act' of the top conv output, stored as the conv backward reads it -- and the
conv half of DQN's backward pass (`ops.cnn_backward_from_dz`).  BY DEFAULT that gradient is three launches: the grouped
input gradient into a (K, B, F) stack, trl_boot_fold_f32, the gated transpose.  `HEAD_DX_FUSED = True` (opt-in, a module
global read when the engine is built) takes ONE launch instead, trl_boot_head_dx_f32 (`_C.boot_head_dx`: one reduction over
K and the heads' first width, no stack); it is not the default because it measured slower than the three launches at the
reference's shape (profiles/NOTES_bootstrapped_dqn_conv.md).  `head_dx_route` records which of the two an update took.
"""
import torch
import torch.optim as optim

from ... import _C, dist, ops
from ._engine import FlatHome
from .dqn import DQN, _FusedDQN


# conv trunks: True takes trl_boot_head_dx_f32 for the heads' input gradient at the feature, False the three launches it
# replaces.  False by default: at the reference's shape the one launch measured slower than the three
# (profiles/NOTES_bootstrapped_dqn_conv.md); the tests run both.
HEAD_DX_FUSED = False


class BootstrappedDQN(DQN):
    sample_key = ("obs", "next_obs", "acts", "rewards", "terminals", "masks")

    def __init__(self, head_num=10, bernoulli_p=0.5, **kwargs):
        super().__init__(**kwargs)
        self.head_num = int(head_num)
        self.bernoulli_p = float(bernoulli_p)
        if not 0.0 <= self.bernoulli_p <= 1.0:
            raise _C.TrlError("BootstrappedDQN: bernoulli_p is a probability, got %s" % (bernoulli_p,))
        qf_heads = getattr(self.qf, "head_num", None)
        if qf_heads != self.head_num or getattr(self.pf, "head_num", None) != self.head_num:
            raise _C.TrlError("BootstrappedDQN(head_num=%d) needs a BootstrappedNet and a BootstrappedDQNDiscretePolicy with "
                              "the same number of heads (network: %s, policy: %s)"
                              % (self.head_num, qf_heads, getattr(self.pf, "head_num", None)))
        self.pf.bernoulli_p = self.bernoulli_p                          # the collector draws the masks with it

    def engine(self):
        if self._engine is None:
            # (TRL_BOOT_CONV=1: RMSprop and SGD step on trl_clip_step_f32 as in DQN; `_optim.step_spec` refuses the rest)
            if self.optimizer_class is not optim.Adam and not ops.boot_conv():
                raise _C.TrlError("the fused Bootstrapped DQN step implements torch.optim.Adam only (got %s)"
                                  % getattr(self.optimizer_class, "__name__", self.optimizer_class))
            if dist.world_size() != 1:
                raise _C.TrlError("Bootstrapped DQN runs on one rank (got a world of %d): several ranks are not built"
                                  % dist.world_size())
            self._engine = _FusedBootDQN(self)
        return self._engine


class _FusedBootDQN(_FusedDQN):
    """`_FusedDQN`'s protocol (static inputs, eager -> captured -> replayed launch sequence, loss sums through a StatRing,
    whole epochs as one graph) for a BootstrappedNet."""
    KEYS = ("obs", "next_obs", "acts", "rewards", "terminals", "masks")

    def __init__(self, algo):
        from ...networks.base import MLPBase
        self.algo = algo
        qf = algo.qf
        self.dev = next(qf.parameters()).device
        if self.dev.type != "cuda":
            raise _C.TrlError("Bootstrapped DQN networks live on %s: the HIP path needs a GPU (no CPU path exists)" % self.dev)
        self.is_conv = bool(getattr(qf, "is_conv", False)) and ops.boot_conv()
        if not (isinstance(qf.base, MLPBase) or self.is_conv) or qf.add_ln:
            raise _C.TrlError("Bootstrapped DQN runs MLP trunks without LayerNorm only")
        self.is_mlp = not self.is_conv                                   # (`_load`: uint8 frame stacks for a conv trunk)
        self.head_dx_fused = HEAD_DX_FUSED
        self.head_dx_route = None                                        # which route the last built launch sequence took
        self.K, self.A = int(algo.head_num), int(algo.env.action_space.n)
        if not 1 <= self.K <= 64 or not 1 <= self.A <= 64 or int(qf.out_dim) != self.A:
            raise _C.TrlError("Bootstrapped DQN: 1..64 heads and 1..64 actions, the heads as wide as the env's action set "
                              "(K=%d, A=%d, heads emit %d)" % (self.K, self.A, int(qf.out_dim)))
        self.act = ops.cnn_act_code(qf) if self.is_conv else ops.act_code(qf)
        self._init_run_state()                                          # (ring, slab, static inputs, graphs, step state)
        self._loss_ws = _C.boot_td_loss_workspace(self.dev)              # (the loss launch's arrival counter lives there)
        self._home()

    def _home(self):
        """One flat parameter / gradient / Adam buffer over trunk and all heads (module order), the networks' parameters
        views of it and `qf_optimizer.state` bound to the moments."""
        algo, qf, tqf = self.algo, self.algo.qf, self.algo.target_qf
        K = self.K
        self.trunk, self.ttrunk = qf.trunk_layers(), tqf.trunk_layers()
        self.heads = [qf.head_layers(k) for k in range(K)]
        self.theads = [tqf.head_layers(k) for k in range(K)]
        plist, tlist = qf.param_list(), tqf.param_list()
        home = FlatHome([plist], [algo.qf_optimizer], tlist, keep=(self.m, self.v) if hasattr(self, "m") else None)
        self.flat, self.tflat, self.grads, self.m, self.v = home.flat, home.tflat, home.grads, home.m, home.v
        self.opt_spec, self.c = home.specs[0], home.c                    # (Adam, unless TRL_BOOT_CONV=1: see `engine()`)
        pairs = home.pairs()[0]
        nt, nh = len(self.trunk), len(self.heads[0])
        self.trunk_gviews = pairs[:nt]
        self.head_gviews = [pairs[nt + k * nh:nt + (k + 1) * nh] for k in range(K)]
        self._homed = (plist[0].data_ptr(), plist[-1].data_ptr(), tlist[0].data_ptr(), tlist[-1].data_ptr())
        self._graphs.clear()                                             # (they carry the old addresses)

    def _check_home(self):
        """A `.to()` or an assignment that replaced parameter storage (a checkpoint load copies in place and needs nothing):
        re-home the flat buffers and drop the captured graphs, which carry the old addresses."""
        p, t = self.algo.qf.param_list(), self.algo.target_qf.param_list()
        if (p[0].data_ptr(), p[-1].data_ptr(), t[0].data_ptr(), t[-1].data_ptr()) != self._homed:
            self._home()

    def _extra_static(self, B):
        return {"masks": torch.zeros((B, self.K), dtype=torch.float32, device=self.dev)}

    def resolve(self, handles):
        rows = self._ring.read([(h[0], h[1]) for h in handles]).tolist()
        return [{'Reward_Mean': s[2] / B, 'Training/qf_loss': s[0] / B} for s, (_, _, B) in zip(rows, handles)]

    def _handles(self, count, B):
        return [(ref, row, B) for ref, row in self._ring.handles(self.step_count - count, count)]

    def enqueue(self, batch):
        self._check_home()
        return super().enqueue(batch)

    def enqueue_epoch(self, count):
        self._check_home()
        return super().enqueue_epoch(count)

    def _sequence(self, st, soft):
        """The fixed launch sequence of one update on the static inputs (eager, or under graph capture)."""
        algo, dev, K, A, act = self.algo, self.dev, self.K, self.A, self.act
        obs, nobs = st["obs"], st["next_obs"]
        B = int(obs.shape[0])
        f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        # trunks: online on obs (kept for the backward pass), target on next_obs
        if self.is_conv:
            # the paired conv forward of DQN (one grouped launch per layer after the first), stopping at the feature
            (feat, trunk_tape), (tfeat, _) = ops.cnn_forward_pair(algo.qf, algo.target_qf, obs, nobs, dx_prep=True,
                                                                  feature=True)
        else:
            feat, trunk_tape = ops.mlp_forward(self.trunk, obs, act, last_act=act)
            tfeat, _ = ops.mlp_forward(self.ttrunk, nobs, act, last_act=act, keep=False)
        F = int(feat.shape[1])
        # all K heads: one grouped launch per head level, the last one writing the head-major (K, B, A) stack
        q, qn = f(K, B, A), f(K, B, A)
        _, tapes = ops.mlp_forward_group(self.heads, [feat] * K, act, out=list(q.unbind(0)))
        ops.mlp_forward_group(self.theads, [tfeat] * K, act, keep=[False] * K, out=list(qn.unbind(0)))
        dq = _C.boot_td_loss(q, qn, st["acts"].view(-1), st["rewards"].view(-1), st["terminals"].view(-1), st["masks"],
                             algo.discount, self.sums, ring=(self._ring.t, self.step_state), workspace=self._loss_ws)
        wsz = _C.lib().trl_linear_bwd_weight_workspace
        need = max(([ops.cnn_backward_workspace(trunk_tape)] if self.is_conv else
                    [wsz(B, int(w.shape[1]), int(w.shape[0])) for w, _ in self.trunk]) +
                   [K * wsz(B, int(w.shape[1]), int(w.shape[0])) for w, _ in self.heads[0]])
        if self.workspace is None or self.workspace.numel() < need:
            self.workspace = torch.empty(max(need, 4), device=dev)
        if self.is_conv:
            return self._conv_backward(st, soft, tapes, dq, trunk_tape, f)
        # heads backwards: per level one grouped weight-gradient and one grouped input-gradient launch; the K gradients at
        # the trunk feature land in one (K, B, F) stack and are folded in ascending k by one launch
        dfeat_k = f(K, B, F)

        def sink(dys, gates, gate_act, ws):
            _C.linear_bwd_input_group(dys, gates, gate_act, ws, dxs=list(dfeat_k.unbind(0)))
        ops.mlp_backward_group(tapes, list(dq.unbind(0)), self.head_gviews, need_input=True, workspace=self.workspace,
                               input_sink=sink)
        dfeat = _C.boot_fold(dfeat_k)
        ops.mlp_backward(trunk_tape, dfeat, grads=self.trunk_gviews, workspace=self.workspace)
        self._adam_polyak(soft, 1.0)

    def _conv_backward(self, st, soft, tapes, dq, trunk_tape, f):
        """The backward half of `_sequence` over a conv trunk.  The heads' weight gradients as over an MLP trunk; their
        input gradient at the feature -- summed over the K heads, gated by act' of the top conv output and un-flattened to
        the (b, p, c) order the conv backward reads -- is three launches by default (grouped input gradient into a
        (K, B, F) stack, trl_boot_fold_f32, the gated transpose), or with `head_dx_fused` (`HEAD_DX_FUSED = True`, opt-in:
        it measured slower) ONE launch, trl_boot_head_dx_f32, where that launch carries the shape.  `head_dx_route`
        ("fused" / "three_launches") says which one ran.  Then the conv half of DQN's backward pass and the step."""
        K, act = self.K, self.act
        B = trunk_tape.B
        P, Cc = trunk_tape.feat_shape
        top_y, like_in = trunk_tape.convs[-1][2], bool(trunk_tape.feat_chw)
        got = {}

        def sink(dys, gates, gate_act, ws):
            if self.head_dx_fused and _C.boot_head_dx_supported(K, B, int(dys[0].shape[1]), Cc, P):
                got["dz"] = _C.boot_head_dx(dys, gates if any(g is not None for g in gates) else None, gate_act, ws, top_y,
                                            act, Cc, P, like_in)
                self.head_dx_route = "fused"
                return
            self.head_dx_route = "three_launches"
            dfeat_k = f(K, B, Cc * P)
            _C.linear_bwd_input_group(dys, gates, gate_act, ws, dxs=list(dfeat_k.unbind(0)))
            got["dz"] = _C.transpose_bpc(_C.boot_fold(dfeat_k).view(B, Cc, P), B, Cc, P, y_gate=top_y, gate_act=act,
                                         gate_like_in=like_in)
        ops.mlp_backward_group(tapes, list(dq.unbind(0)), self.head_gviews, need_input=True, workspace=self.workspace,
                               input_sink=sink)
        ops.cnn_backward_from_dz(trunk_tape, got["dz"].view(B * P, Cc), self.trunk_gviews, workspace=self.workspace)
        self._adam_polyak(soft, 1.0)
