"""The device side of the rollout kernel tests -- test infrastructure, imported by tests/test_rollout_kernels_gpu.py and
tests/test_rollout_heads_gpu.py only.  `Launcher` plants one case of tests/_rollout_ref.py on the device, launches
trl_rollout_synth_f32 / _cat_f32 / _sd_f32 through torchrl_amd._C and reads the run back; every tensor a launch may write lies
between guard words that `read` checks."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _gauss_ref as G                                                        # noqa: E402
import _rollout_ref as R                                                      # noqa: E402

DEV = torch.device("cuda:0")
GUARD = 64
GUARD_VALUE = 4242.5                                                          # (not the ring's pre-fill: a guard is never a row)
RING = (("obs", "D"), ("next_obs", "D"), ("acts", "A"), ("values", 1), ("rewards", 1), ("terminals", 1), ("time_limits", 1),
        ("old_logp", 1))


def dev(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


class Launcher:
    """The device side of one case: parameters, env / collector state, a ring pre-filled with the sentinel, the episode log,
    and (norm) the normaliser state, policy observations and a freshly zeroed workspace.  `launch` may be called again: the
    state continues on the device.  Every ring tensor is the middle of a buffer with GUARD words in front of it and behind it:
    a store of the wrong width (A floats per cell into the (N, 1) acts of a categorical head) lands inside the launch's own
    rows until the last one, where it runs into the guard."""

    def __init__(self, c, norm=False):
        from torchrl_amd import _C
        self._C, self.c, self.norm = _C, c, norm
        N, D, A = c["N"], c["D"], c["A"]
        self.pf, self.vf = R.flat(c["pf"], c["logstd"]).to(DEV), R.flat(c["vf"]).to(DEV)
        self.env_A, self.env_B = dev(c["env_A"]), dev(c["env_B"])
        self.cur_obs, self.t_env, self.cur_step = dev(c["cur_obs"]), dev(c["t_env"]), dev(c["cur_step"])
        self.episode_idx, self.ep_return = dev(c["episode_idx"]), dev(c["ep_return"])
        self.ring_buf, self.ring = {}, {}
        for k, f in RING:
            f = R.acts_width(c) if k == "acts" else c[f] if isinstance(f, str) else f
            # (behind a categorical head's acts the guard is as long as an (N, A)-shaped store would reach: such a store
            # is caught, and caught inside the allocation)
            tail = GUARD + (c["rows"] * N * (A - 1) if k == "acts" and f != A else 0)
            buf = torch.full((GUARD + c["rows"] * N * f + tail,), GUARD_VALUE, device=DEV)
            self.ring_buf[k], self.ring[k] = buf, buf[GUARD:GUARD + c["rows"] * N * f].view(c["rows"], N, f)
            self.ring[k].fill_(R.SENT)
        self.epoch_reward = torch.full((1,), c["epoch_reward0"], dtype=torch.float64, device=DEV)
        self.ep_count = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.ep_log = torch.full((c["ep_cap"] + 4, 3), R.SENT, device=DEV)
        self.boot = torch.full((N + GUARD,), R.SENT, device=DEV)
        self.pub_src = dev(c["pub_src"].view(np.int32))
        self.pub_dst = torch.full((c["publish"] + GUARD,), -7, dtype=torch.int32, device=DEV)
        if norm:
            self.state = dev(G.norm_state_vec(c["state"]))
            self.policy_obs = dev(c["policy_obs"])
            self.ws = torch.zeros(_C.lib().trl_rollout_norm_workspace(N), dtype=torch.float64, device=DEV)

    def args(self, T=None, top=None, noise_step0=None, eps=None):
        """The launch descriptor of the case (tests of the refusals edit it before `call`)."""
        _C, c = self._C, self.c
        T = c["T"] if T is None else T
        a = _C.RolloutArgs()
        a.pf_params, a.vf_params = self.pf.data_ptr(), self.vf.data_ptr()
        a.D, a.H, a.A, a.act = c["D"], 64, c["A"], _C.ACT_TANH if c["act"] == "tanh" else _C.ACT_RELU
        a.tanh_action = int(c["tanh"])
        a.env_A, a.env_B = self.env_A.data_ptr(), self.env_B.data_ptr()
        a.reward_scale, a.horizon, a.env_seed_base = c["reward_scale"], c["horizon"], c["seed_base"]
        a.cur_obs, a.t_env, a.cur_step = self.cur_obs.data_ptr(), self.t_env.data_ptr(), self.cur_step.data_ptr()
        a.episode_idx, a.ep_return = self.episode_idx.data_ptr(), self.ep_return.data_ptr()
        self.noise = None
        if c["noise"] == "host":
            self.noise = dev(c["eps"] if eps is None else eps)
            assert self.noise.shape == (T, c["N"], c["A"])
        a.noise = None if self.noise is None else self.noise.data_ptr()
        a.noise_step0 = c["noise_step0"] if noise_step0 is None else noise_step0
        a.deterministic = int(c["noise"] == "det")
        for k, _ in RING:
            setattr(a, k, self.ring[k].data_ptr())
        a.rows, a.top, a.N, a.n_steps = c["rows"], c["top"] if top is None else top, c["N"], T
        a.max_episode_frames, a.discount = c["max_frames"], c["discount"]
        a.epoch_reward, a.ep_count, a.ep_log = self.epoch_reward.data_ptr(), self.ep_count.data_ptr(), self.ep_log.data_ptr()
        a.ep_cap, a.step0 = c["ep_cap"], c["step0"]
        if c["boot"]:
            a.boot_values = self.boot.data_ptr()
        if c["publish"]:
            a.publish_dst, a.publish_src, a.publish_words = self.pub_dst.data_ptr(), self.pub_src.data_ptr(), c["publish"]
        if self.norm:
            a.norm_state, a.policy_obs, a.norm_workspace = self.state.data_ptr(), self.policy_obs.data_ptr(), self.ws.data_ptr()
            a.norm_clip, a.norm_update, a.normalize_partial_reset = c["norm_clip"], c["norm_update"], c["partial_reset"]
        return a

    def call(self, a):
        """The entry point of the case's head."""
        _C, c = self._C, self.c
        head = R.head_of(c)
        if head == "cat":
            _C.rollout_cat(a, c["cat_seed"], c["env_offset"], DEV)
        elif head == "sd":
            _C.rollout_sd(a, DEV)
        else:
            _C.rollout(a, DEV)

    def launch(self, T=None, top=None, noise_step0=None, eps=None):
        self.call(self.args(T, top, noise_step0, eps))
        torch.cuda.synchronize()
        return self

    def untouched(self):
        """Nothing was launched: every ring tensor, the log and the boot row still hold their pre-fill, the guards theirs."""
        self.check_guards()
        return all(bool((v == R.SENT).all()) for v in self.ring.values()) and bool((self.ep_log == R.SENT).all()) and \
            bool((self.boot == R.SENT).all()) and int(self.ep_count.item()) == 0

    def check_guards(self):
        for k, buf in self.ring_buf.items():
            b = buf.cpu().numpy()
            assert (b[:GUARD] == np.float32(GUARD_VALUE)).all(), "the guard in front of the ring's %s was overwritten" % k
            assert (b[GUARD + self.ring[k].numel():] == np.float32(GUARD_VALUE)).all(), "the guard behind the ring's %s was overwritten" % k

    def read(self):
        c, N = self.c, self.c["N"]
        self.check_guards()
        o = {k: v.cpu().numpy() for k, v in self.ring.items()}
        o.update(cur_obs=self.cur_obs.cpu().numpy(), t_env=self.t_env.cpu().numpy(), cur_step=self.cur_step.cpu().numpy(),
                 episode_idx=self.episode_idx.cpu().numpy(), ep_return=self.ep_return.cpu().numpy(),
                 epoch_reward=float(self.epoch_reward.item()), ep_count=int(self.ep_count.item()), ep_log=self.ep_log.cpu().numpy(),
                 pub_dst=self.pub_dst.cpu().numpy()[:c["publish"]].view(np.uint32))
        boot = self.boot.cpu().numpy()
        assert (boot[N:] == np.float32(R.SENT)).all() and (self.pub_dst.cpu().numpy()[c["publish"]:] == -7).all(), "guard overwritten"
        o["boot"] = boot[:N] if c["boot"] else None
        if not c["boot"]:
            assert (boot == np.float32(R.SENT)).all(), "boot_values = NULL, yet the buffer was written"
        if self.norm:
            o.update(state=self.state.cpu().numpy(), policy_obs=self.policy_obs.cpu().numpy())
            assert int(self.ws.view(torch.int32)[2].item()) == 0, "the rendezvous raised its error word"
        return o


def check(res, what, errlog):
    print("%s: worst err / bound %s" % (what, {k: round(float(v), 4) for k, v in res.items()}))
    for k, v in res.items():
        if not k.startswith("_"):
            errlog("%s/%s" % (what, k), v, 1.0)
    bad = {k: v for k, v in res.items() if not k.startswith("_") and not v <= 1.0}
    assert not bad, (what, bad)
