"""Plain torch restatement (CPU, float64 by default) of REINFORCE as this package runs it -- test infrastructure, imported
by tests/test_reinforce_*.py only.

`ReinforceUpdate.update` restates Reinforce.update (torchrl/algo/on_policy/reinforce.py:33-75) for the three policy heads:
L = mean(-log pi * adv_n) - c_ent * mean(ent) with adv_n = (adv - mean) / (unbiased std + 1e-5), clip_grad_norm_(0.5),
one Adam step with torch's default eps 1e-8; the info dict in the reference's key order, whose `advs/*` are numpy
statistics of the batch (so `advs/std` is the POPULATION std) and whose `logprob/std` is torch's unbiased one.  The
log-probabilities are those of the existing restatements (_gauss_ref, _gauss_sd_ref, _categorical_ref)."""
import math

import numpy as np
import torch

import _categorical_ref as cat_ref
import _gauss_ref as gauss_ref
import _gauss_sd_ref as sd_ref

LOSS_PPO_CLIP, LOSS_A2C, LOSS_REINFORCE = 0, 1, 2
INFO_KEYS = ['advs/mean', 'advs/std', 'advs/max', 'advs/min', 'Training/policy_loss', 'ent', 'logprob/mean', 'logprob/std',
             'logprob/max', 'logprob/min']
VALUE_SLOTS = (7, 12, 13, 14, 15)                                            # value loss and value statistics of the info row
POLICY_SLOTS = tuple(range(0, 7)) + tuple(range(8, 12)) + tuple(range(16, 21))
HEADS = {"g": "gauss", "sd": "sd", "cat": "cat"}                              # fixture tag -> head


class MLP:
    """Tanh / ReLU MLP on explicit parameter lists [W1, b1, W2, b2, ...] (nn.Linear layout) in a given dtype."""

    def __init__(self, params, act=torch.tanh, dtype=torch.float64):
        self.params = [torch.as_tensor(np.asarray(p)).clone().to(dtype).requires_grad_(True) for p in params]
        self.act = act

    def __call__(self, x):
        h = x
        n = len(self.params) // 2
        for k in range(n):
            h = h @ self.params[2 * k].t() + self.params[2 * k + 1]
            if k < n - 1:
                h = self.act(h)
        return h


def logp_ent(head, out, logstd, acts, tanh):
    """-> (log pi (B,), entropy (B,)) of the network output `out` under `head`."""
    if head == "cat":
        lp, H, _ = cat_ref.cat_logp(out, acts)
        return lp, H
    if head == "sd":
        return sd_ref.logp(out, acts, tanh)
    ls = logstd.clamp(-20.0, 2.0)
    ent = (0.5 + gauss_ref.HALF_LOG_2PI + ls).sum()
    return gauss_ref.logp(out, logstd, acts, tanh), ent.expand(out.shape[0])


class ReinforceUpdate:
    def __init__(self, head, params, logstd=None, plr=3e-3, entropy_coeff=0.001, tanh=True, act=torch.tanh,
                 dtype=torch.float64):
        self.head, self.tanh, self.dtype, self.entropy_coeff = head, tanh, dtype, entropy_coeff
        self.pf = MLP(params, act, dtype)
        self.logstd = None if logstd is None else torch.as_tensor(np.asarray(logstd)).clone().to(dtype).requires_grad_(True)
        self.params = self.pf.params + ([] if self.logstd is None else [self.logstd])
        self.opt = torch.optim.Adam(self.params, lr=plr)                     # eps 1e-8: reinforce.py:25-28 passes none

    def update(self, batch):
        t = lambda x: torch.as_tensor(np.asarray(x)).to(self.dtype)
        obs, acts, advs = t(batch["obs"]), t(batch["acts"]), t(batch["advs"]).reshape(-1)
        a_np = np.asarray(batch["advs"], dtype=np.float64)
        info = {'advs/mean': a_np.mean(), 'advs/std': a_np.std(), 'advs/max': a_np.max(), 'advs/min': a_np.min()}
        lp, ent = logp_ent(self.head, self.pf(obs), self.logstd, acts, self.tanh)
        advn = ((advs - advs.mean()) / (advs.std() + 1e-5)).detach()
        loss = (-lp * advn).mean() - self.entropy_coeff * ent.mean()
        self.opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(self.params, 0.5)
        self.opt.step()
        lp = lp.detach()
        info.update({'Training/policy_loss': loss.item(), 'ent': ent.mean().item(), 'logprob/mean': lp.mean().item(),
                     'logprob/std': lp.std().item(), 'logprob/max': lp.max().item(), 'logprob/min': lp.min().item()})
        return {k: float(v) for k, v in info.items()}

    def moments(self):
        """(exp_avg list, exp_avg_sq list) in the order of `self.params`."""
        return [self.opt.state[p]["exp_avg"] for p in self.params], [self.opt.state[p]["exp_avg_sq"] for p in self.params]


# ------------------------------------------------------------------ the fixture (tests/golden/reinforce_update.npz)
def batch_of(g, tag):
    return {k: g[f"{tag}_batch_{k}"] for k in ("obs", "acts", "advs")}


def info_of(g, tag, s):
    return dict(zip((str(k) for k in g[f"{tag}_info{s}_keys"]), (float(x) for x in g[f"{tag}_info{s}_vals"])))


def _names(g, prefix):
    """The fixture's parameter names behind `prefix`, as [W1, b1, ..., W_head, b_head] (+ ['logstd'])."""
    index = lambda k: int([x for x in k.split("__") if x.isdigit()][0])
    names = [k[len(prefix):] for k in g.files if k.startswith(prefix)]
    layers = sorted((k for k in names if k != "logstd"), key=lambda k: (not k.startswith("base"), index(k), k.endswith("bias")))
    return layers + (["logstd"] if "logstd" in names else [])


def params_of(g, prefix):
    """(layer parameter list, logstd or None) stored behind `prefix`."""
    names = _names(g, prefix)
    arrays = [g[prefix + k].copy() for k in names]
    return (arrays[:-1], arrays[-1]) if names[-1] == "logstd" else (arrays, None)


def restatement_of(g, tag, dtype=torch.float64):
    layers, logstd = params_of(g, f"{tag}_pf0_")
    plr, ent = (float(x) for x in g[f"{tag}_hyper"])
    return ReinforceUpdate(HEADS[tag], layers, logstd, plr=plr, entropy_coeff=ent, tanh=True, dtype=dtype)


def info_close(got, want, rel=1e-4, ab=1e-5):
    """Worst |got - want| / (ab + rel |want|) over the keys of `want` (rel 1e-4 / abs 1e-5)."""
    return max(abs(got[k] - want[k]) / (ab + rel * abs(want[k])) for k in want)


def state_error(g, prefix, tensors):
    """max |tensor - fixture array| over the parameter list `tensors` ([W1, b1, ..., (logstd)]) stored behind `prefix`."""
    names = _names(g, prefix)
    assert len(names) == len(tensors), (names, len(tensors))
    return max(float(np.abs(np.asarray(t.detach().cpu().double()) - g[prefix + k].astype(np.float64)).max())
               for k, t in zip(names, tensors))


def discounted_returns(rewards, terminals, gamma):
    """The reference's discount_reward with zero values and a zero bootstrap (replay_buffers/on_policy.py:46-70), float64:
    R_t = r_t + gamma (1 - done_t) R_{t+1}; the time-limit filter multiplies a zero value, whichever way it is set."""
    r, d = np.asarray(rewards, dtype=np.float64), np.asarray(terminals, dtype=np.float64)
    out, run = np.zeros_like(r), np.zeros_like(r[0])
    for t in reversed(range(r.shape[0])):
        run = r[t] + gamma * (1.0 - d[t]) * run
        out[t] = run
    return out


# ------------------------------------------------------------------ loss-kernel inputs of the other two heads
def sd_loss_case(B, A, tanh, seed):
    """tests/test_gauss_sd_gpu.py::loss_case without the value half: head (B, 2A), actions drawn from it (tanh actions
    clamped to +-0.995), advantages 2 N(0, 1) + 0.5."""
    rs = np.random.RandomState(seed)
    t = lambda *s: torch.from_numpy(rs.randn(*s).astype(np.float32))
    head = torch.cat([t(B, A) * 0.5, torch.from_numpy(rs.uniform(-1.5, 0.5, (B, A)).astype(np.float32))], dim=1)
    acts = sd_ref.explore(head, t(B, A), tanh)[0]
    if tanh:
        acts = acts.clamp(-0.995, 0.995)
    return dict(head=head, acts=acts.contiguous(), advs=t(B) * 2 + 0.5, v=t(B), rets=t(B))


def cat_loss_case(B, A, seed):
    rs = np.random.RandomState(seed)
    t = lambda *s: torch.from_numpy(rs.randn(*s).astype(np.float32))
    return dict(logits=t(B, A) * 1.5, acts=torch.from_numpy(rs.randint(0, A, size=(B,)).astype(np.float32)),
                advs=t(B) * 2 + 0.5, v=t(B), rets=t(B))


def raw_of(advs):
    return gauss_ref.adv_raw_of(advs)


def zero_value_slots(info):
    out = np.array(info, dtype=np.float64, copy=True)
    out[list(VALUE_SLOTS)] = 0.0
    return out


def population_std(raw, n):
    """`advs/std` from the raw statistics {sum, sumsq, max, -min}: the population (ddof = 0) std, in double."""
    return math.sqrt(max((float(raw[1]) - float(raw[0]) ** 2 / n) / n, 0.0))
