"""Discrete-action policies: epsilon-greedy wrappers over a Q network (torchrl/policies/discrete_policies.py:23-89)
and the categorical policy of the on-policy algorithms (:124-168, `CategoricalDisPolicy` below).

`explore` keeps the reference's host-side protocol -- linear epsilon decay per call, then
`np.random.rand(*shape)` and `np.random.randint(0, A, shape)` from the global numpy stream (so
seeded runs replay the reference's exploration decisions) -- but the Q network runs on the conv /
dense HIP kernels and the argmax + mask is one kernel (trl_eps_greedy_i64).  Unlike the
reference's QR-DQN policy (single env, `.item()`, its Q16) both policies are vectorised over N
envs; actions are returned as (N, 1) int64.

`BootstrappedDQNDiscretePolicy` (:92-121): every env plays one of K heads (trl_boot_act_i64 behind one shared trunk pass),
evaluation takes the ensemble vote; heads are device Philox draws (trl_boot_heads_i64), not host numpy draws.
"""
import numpy as np
import torch

from .. import _C, networks, ops


class EpsilonGreedyDQNDiscretePolicy:
    quantile_num = 1

    def __init__(self, qf, start_epsilon, end_epsilon, decay_frames, action_shape):
        self.qf = qf
        self.start_epsilon = start_epsilon
        self.end_epsilon = end_epsilon
        self.decay_frames = decay_frames
        self.count = 0
        self.action_shape = action_shape
        self.epsilon = self.start_epsilon
        self.continuous = False

    def _q(self, x):
        with torch.no_grad():
            if x.dtype == torch.uint8:
                return ops.cnn_forward(self.qf, x)[0]
            return self.qf(x)

    def q_to_a(self, q):
        return _C.eps_greedy(q.contiguous(), self.action_shape, self.quantile_num, None, None, 0.0).unsqueeze(-1)

    def one_launch_act(self):
        """Conv nets with a hidden FC layer in front of an A <= 8 wide head (Q = 1): head and action are ONE launch."""
        A = int(self.action_shape)
        if self.quantile_num != 1 or A > 8 or not hasattr(self.qf, "base") or not hasattr(self.qf.base, "seq_convs"):
            return False
        fcs = ops.fc_layers(self.qf)
        return len(fcs) >= 2 and int(fcs[-1][0].shape[0]) == A and \
            bool(_C.lib().trl_dqn_act_supported(int(fcs[-1][0].shape[1]), A)) and fcs[-1][0].data_ptr() % 16 == 0

    def act_on(self, x, u=None, rand_act=None, epsilon=0.0, want_q=True, ring_row=None, n_rows=0):
        """(q or None, action (N,) int64) for a batch of observations: greedy (u None) or mixed with the given draws.  Conv
        nets with a hidden FC layer and an A <= 8 wide head (Q = 1) run the head and the action as ONE launch on the last
        hidden activations (trl_dqn_act_f32); everything else is Q network -> trl_eps_greedy_i64.  `ring_row`: the collector's
        device-resident replay row advances in the action launch."""
        A = int(self.action_shape)
        if x.dtype == torch.uint8 and self.one_launch_act():
            with torch.no_grad():
                h, _ = ops.cnn_forward(self.qf, x, head=False)
            w, b = ops.fc_layers(self.qf)[-1]
            if _C.dqn_act_ok(h, w):
                return _C.dqn_act(h, w, b, u, rand_act, epsilon, want_q=want_q, ring_row=ring_row, n_rows=n_rows)
        q = self._q(x)
        return q, _C.eps_greedy(q.contiguous(), A, self.quantile_num, u, rand_act, epsilon, ring_row=ring_row, n_rows=n_rows)

    def explore(self, x):
        self.count += 1
        if x.dim() in (3, 5) and x.shape[0] == 1:                    # the collector's unsqueeze(0) (base.py:185-186)
            x = x.squeeze(0)
        if self.count < self.decay_frames:
            self.epsilon = self.start_epsilon - (self.start_epsilon - self.end_epsilon) * (self.count / self.decay_frames)
        else:
            self.epsilon = self.end_epsilon
        n = int(x.shape[0])
        from .. import dist
        w, r = dist.world_size(), dist.rank()                       # env shards on several ranks: this rank's rows of the
        u = np.random.rand(n * w, 1)[r * n:(r + 1) * n]             # host draws for ALL envs (identical numpy streams)
        ra = np.random.randint(low=0, high=self.action_shape, size=(n * w, 1))[r * n:(r + 1) * n]
        u = torch.from_numpy(u.astype(np.float32)).to(x.device)
        ra = torch.from_numpy(ra.astype(np.int64)).to(x.device)
        output, action = self.act_on(x, u.reshape(-1).contiguous(), ra.reshape(-1).contiguous(), self.epsilon)
        return {"q_value": output, "action": action.unsqueeze(-1)}

    def eval_act(self, x):
        return self.act_on(x, want_q=False)[1].unsqueeze(-1).cpu().numpy()

    def to(self, device):
        self.qf.to(device)

    def parameters(self):
        return self.qf.parameters()


class EpsilonGreedyQRDQNDiscretePolicy(EpsilonGreedyDQNDiscretePolicy):
    """argmax over the mean of the quantiles (discrete_policies.py:86-89), for all N envs."""

    def __init__(self, quantile_num, **kwargs):
        super().__init__(**kwargs)
        self.quantile_num = quantile_num


class BootstrappedDQNDiscretePolicy:
    """Wrapper over a `networks.BootstrappedNet` (torchrl/policies/discrete_policies.py:92-121), vectorised over N envs:
    the reference plays ONE env with `.item()` and a host `np.random.randint` head; here every env plays a head of its own.

    `idx` is an (N,) int64 device tensor -- allocated at the first `explore` for N envs and drawn for all of them --
    `explore` returns each env's arg-max under its head ((N, 1) int64) with that head's Q row, `eval_act` the arg-max of
    the ensemble vote (the reference's `eval_act` on a (1, D) input).  All K heads share one trunk pass; the selection is
    one launch (trl_boot_act_i64).  Heads are Philox draws of (`seed`, counter, global env index) (trl_boot_heads_i64), not
    host numpy draws: those would interleave with the replay index stream, and the reference has no vector-env
    behaviour to match.  `bernoulli_p` is set by the algorithm (the collector draws the masks with it)."""
    seed = 0xB007D
    bernoulli_p = 0.5

    def __init__(self, qf, head_num, action_shape):
        if not 1 <= int(head_num) <= 64 or not 1 <= int(action_shape) <= 64:
            raise _C.TrlError("BootstrappedDQNDiscretePolicy: the kernels carry 1..64 heads and 1..64 actions, got "
                              "head_num=%s, action_shape=%s" % (head_num, action_shape))
        self.qf = qf
        self.head_num = int(head_num)
        self.action_shape = action_shape
        self.idx = None
        self._pending_head = None
        self.continuous = False

    def _ensure_idx(self, n, device):
        if self.idx is None or int(self.idx.numel()) != n or self.idx.device != device:
            self.idx = torch.zeros(n, dtype=torch.int64, device=device)
            self.sample_head(counter=-1)                             # (the draw "before step 0": steps count from 0)

    def sample_head(self, mask=None, counter=0, env_offset=0):
        """Fresh heads where `mask` (N bytes) is set, everywhere when it is None: the Philox word of
        (seed, counter, env_offset + n) scaled to [0, K)."""
        if self.idx is None:
            return                                                   # (no envs seen yet: the first explore draws)
        if mask is not None:
            mask = torch.as_tensor(mask).to(device=self.idx.device, dtype=torch.uint8).reshape(-1).contiguous()
        _C.boot_heads(self.idx, self.head_num, self.seed, counter, env_offset, mask)

    def set_head(self, idx):
        """One head for every env (an int; before the envs are known it is applied at the first explore), or an (N,) tensor."""
        if isinstance(idx, torch.Tensor):
            dev = next(self.qf.parameters()).device
            self.idx = idx.to(device=dev, dtype=torch.int64).reshape(-1).contiguous().clone()
        elif self.idx is None:
            self._pending_head = int(idx)
        else:
            self.idx.fill_(int(idx))

    def _rows(self, x):
        if getattr(self.qf, "is_conv", False):                       # frame batches (..., C, H, W): one row per stack
            if x.dim() < 3:
                raise _C.TrlError("BootstrappedDQNDiscretePolicy over a conv trunk takes (N, C, H, W) frame stacks, got a "
                                  "tensor of shape %s" % (tuple(x.shape),))
            return x.reshape((-1,) + tuple(x.shape[-3:]))
        if x.dim() == 3 and x.shape[0] == 1:                         # the collector's unsqueeze(0)
            x = x.squeeze(0)
        return x.reshape(-1, x.shape[-1])

    def act_on(self, x, greedy_vote=False, want_q=True, onehot=None):
        """(q_sel or None, action (N,) int64) for a batch of observations: under each env's head, or the ensemble vote."""
        x = self._rows(x)
        if not x.is_cuda:
            raise _C.TrlError("BootstrappedDQNDiscretePolicy: observations live on %s, the HIP path needs a GPU" % x.device)
        n = int(x.shape[0])
        if not greedy_vote:
            had = self.idx is not None and int(self.idx.numel()) == n and self.idx.device == x.device
            self._ensure_idx(n, x.device)
            if not had and getattr(self, "_pending_head", None) is not None:
                self.idx.fill_(self._pending_head)
            self._pending_head = None
        with torch.no_grad():
            stack = self.qf.forward_stack(x)
        act, q = _C.boot_act(stack, None if greedy_vote else self.idx, want_q=want_q, onehot=onehot)
        return q, act

    def explore(self, x):
        q, act = self.act_on(x)
        return {"q_value": q, "action": act.unsqueeze(-1)}

    def eval_act(self, x):
        return self.act_on(x, greedy_vote=True, want_q=False)[1].unsqueeze(-1).cpu().numpy()

    def to(self, device):
        self.qf.to(device)

    def parameters(self):
        return self.qf.parameters()


class CategoricalDisPolicy(networks.Net):
    """Categorical policy over a discrete action set (torchrl/policies/discrete_policies.py:124-168): an MLP whose head
    emits A logits.  Same constructor signature and protocol as the reference -- `forward` returns the softmax
    probabilities, `explore` / `eval_act` / `update` their dicts -- with the reference's initialisation (it is `Net`'s).
    On the GPU the trunk runs on the dense-layer kernels and everything behind the logits on k_categorical.hip:
    `trl_cat_act_f32` samples (Philox uniforms, not torch.multinomial's stream), `trl_cat_logp_f32` gives
    log pi / entropy / probabilities; PPO / A2C read `logits()` and use `trl_cat_losses_f32` (algo/on_policy/ppo.py).

    MLP trunks of any shape; a conv trunk (the reference's Atari-shaped examples) is not built.  The reference's
    `explore` returns `action` of shape (N,); here it is (N, 1) float holding the integer value, the layout the
    on-policy ring stores.  `update` takes actions of shape (B,) or (B, 1)."""

    def __init__(self, **kwargs):
        missing = [k for k in ("output_shape", "base_type") if k not in kwargs]
        if missing:
            raise _C.TrlError("a CategoricalDisPolicy without a network (`output_shape`, `base_type`) is not built: "
                              "missing %s" % ", ".join(missing))
        base_type = kwargs["base_type"]
        if not (isinstance(base_type, type) and issubclass(base_type, networks.MLPBase)):
            raise _C.TrlError("CategoricalDisPolicy over a %s trunk is not built: on-policy algorithms here run MLP trunks "
                              "(networks.MLPBase) only, CNN trunks are outside the categorical HIP path"
                              % getattr(base_type, "__name__", base_type))
        if not 2 <= int(kwargs["output_shape"]) <= 64:
            raise _C.TrlError("CategoricalDisPolicy: the categorical kernels carry 2..64 actions, got %s"
                              % (kwargs["output_shape"],))
        super().__init__(**kwargs)
        self.continuous = False
        self._explore_calls = 0

    tanh_action = False                                                # (the engines' launch descriptors ask every policy)
    explore_seed = 0xCA7

    def logits(self, x):
        return networks.Net.forward(self, x)

    @staticmethod
    def _rows(t):
        return t.reshape(-1, t.shape[-1]).float().contiguous()

    def forward(self, x):
        l = self.logits(x)
        if l.is_cuda and not l.requires_grad:
            return _C.cat_probs(self._rows(l)).reshape(l.shape)
        if l.is_cuda:
            _C.note_eager(type(self).__name__ + ".forward", "autograd is on")
        return torch.softmax(l, dim=-1)

    def explore(self, x, return_log_probs=False):
        """One draw per row.  On the GPU: trl_cat_act_f32 with the Philox uniform of (explore_seed, number of calls so
        far, row) -- the collectors do not come through here (they key the draw by their own global step)."""
        with torch.no_grad():
            l = self.logits(x)
        if l.is_cuda:
            rows = self._rows(l)
            act, lp = _C.cat_act(rows, seed=self.explore_seed, counter=self._explore_calls)
            self._explore_calls += 1
            out = {"dis": _C.cat_probs(rows).reshape(l.shape), "action": act.reshape(l.shape[:-1] + (1,))}
            if return_log_probs:
                out["log_prob"] = lp.reshape(l.shape[:-1])
            return out
        probs = torch.softmax(l, dim=-1)
        dis = torch.distributions.Categorical(probs)
        action = dis.sample()
        out = {"dis": probs, "action": action.unsqueeze(-1).float()}
        if return_log_probs:
            out["log_prob"] = dis.log_prob(action)
        return out

    def eval_act(self, x):
        with torch.no_grad():
            l = self.logits(x)
        if l.is_cuda:
            act, _ = _C.cat_act(self._rows(l), deterministic=True)
            return act.reshape(l.shape[:-1]).to(torch.int64).cpu().numpy()
        return l.max(dim=-1)[1].cpu().numpy()

    def update(self, obs, actions):
        l = self.logits(obs)
        if l.is_cuda and not l.requires_grad:
            rows = self._rows(l)
            lp, ent = _C.cat_logp(rows, actions.reshape(-1).float().contiguous(), want_ent=True)
            return {"dis": _C.cat_probs(rows).reshape(l.shape), "log_prob": lp.reshape(l.shape[:-1] + (1,)),
                    "ent": ent.reshape(l.shape[:-1])}
        if l.is_cuda:
            _C.note_eager(type(self).__name__ + ".update", "autograd is on")
        dis = torch.distributions.Categorical(torch.softmax(l, dim=-1))
        return {"dis": dis, "log_prob": dis.log_prob(actions.reshape(l.shape[:-1]).long()).unsqueeze(-1), "ent": dis.entropy()}
