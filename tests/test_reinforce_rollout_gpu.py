"""The persistent rollout WITHOUT a critic (trl_rollout_t.vf_params = NULL; REINFORCE's ZeroNet, V == 0) through
torchrl_amd._C, on the planted cases of tests/_rollout_ref.py: the rollout kernel is the one every other algorithm launches,
the value pass behind it is replaced by a streaming launch that stores 0.0f in `values` and the bootstrap row, publishes
the header and leaves the rewards alone.

Every launch is made twice from the same planted state, with and without the critic, into rings pre-filled with NaN:
  * no env runs over its episode length (max_episode_frames > T): every stored array but `values` is bit-equal;
  * every env does, every second step (max_episode_frames = 2): the with-critic twin gets an all-zero value network, whose
    value pass adds discount * 0 to the marked rewards -- the rollout kernel's own bits -- and the critic-free rewards equal
    them bit for bit and the restated raw env reward at its bound;
  * in both: `values` of the stored cells and the bootstrap row are exactly 0, rows outside the launch keep their NaN, the
    published header equals the device header.
Shapes (T, N, rows, top): a partial 16-env tile (3, 20, ...), a ring that wraps inside the launch (rows 4, top 3), three
workgroups (33 envs); the compile-time 17 / 6 instantiation and a runtime-dims one; host and device noise; the categorical and
the state-dependent-std entry points; the cooperative normalised (NORM) instantiation."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _gauss_ref as G                                                        # noqa: E402
import _rollout_ref as R                                                      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAN = float("nan")
GUARD = 8
SHAPES = [(3, 16, 3, 0), (3, 20, 4, 3), (5, 33, 5, 2)]                        # (T, N, rows, top)
KEYS = ("obs", "next_obs", "acts", "values", "rewards", "terminals", "time_limits", "old_logp")


def dev(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


def no_events(N, T, horizon, max_frames):
    return np.zeros(N, np.int32), np.zeros(N, np.int32)


def case(D, A, noise, T, N, rows, top, max_frames, seed, entry="gauss"):
    c = R.rollout_case(D, A, "tanh", True, N, T, seed, noise=noise, rows=rows, top=top, counters=no_events, noise_step0=40)
    c["max_frames"], c["entry"] = max_frames, entry
    if entry == "sd":                                                          # a [mean | log_std] head of 2A rows, no logstd tail
        c["pf"] = R.make_nets(D, 2 * A, seed + 1)[0]
        c["pf"][5][A:] = -1.5
    return c


class Launch:
    """One launch of case `c` into NaN-filled rings; critic: "net" (the case's value network), "zero" (an all-zero value
    network) or None (vf_params = NULL)."""

    def __init__(self, c, critic, norm=False):
        from torchrl_amd import _C
        N, D, A, T, entry = c["N"], c["D"], c["A"], c["T"], c.get("entry", "gauss")
        self.c = c
        pf = R.flat(c["pf"], c["logstd"] if entry == "gauss" else None).to(DEV)
        vf = R.flat(c["vf"]).to(DEV)
        if critic == "zero":
            vf.zero_()
        keep = [pf, vf]
        a = _C.RolloutArgs()
        a.pf_params, a.vf_params = pf.data_ptr(), (None if critic is None else vf.data_ptr())
        a.D, a.H, a.A, a.act, a.tanh_action = D, 64, A, _C.ACT_TANH, int(c["tanh"])
        self.state = {k: dev(c[k]) for k in ("env_A", "env_B", "cur_obs", "t_env", "cur_step", "episode_idx", "ep_return")}
        for k, v in self.state.items():
            setattr(a, k, v.data_ptr())
        a.reward_scale, a.horizon, a.env_seed_base = c["reward_scale"], c["horizon"], c["seed_base"]
        if c["noise"] == "host" and entry != "cat":
            keep.append(dev(c["eps"]))
            a.noise = keep[-1].data_ptr()
        a.noise_step0 = c["noise_step0"]
        width = dict(obs=D, next_obs=D, acts=1 if entry == "cat" else A)
        self.ring = {k: torch.full((c["rows"], N, width.get(k, 1)), NAN, device=DEV) for k in KEYS}
        for k in KEYS:
            setattr(a, k, self.ring[k].data_ptr())
        a.rows, a.top, a.N, a.n_steps = c["rows"], c["top"], N, T
        a.max_episode_frames, a.discount = c["max_frames"], c["discount"]
        self.epoch_reward = torch.full((1,), c["epoch_reward0"], dtype=torch.float64, device=DEV)
        self.ep_count = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.ep_log = torch.full((c["ep_cap"] + 4, 3), NAN, device=DEV)
        a.epoch_reward, a.ep_count, a.ep_log = self.epoch_reward.data_ptr(), self.ep_count.data_ptr(), self.ep_log.data_ptr()
        a.ep_cap, a.step0 = c["ep_cap"], c["step0"]
        self.boot = torch.full((N + GUARD,), NAN, device=DEV)
        if c["boot"]:
            a.boot_values = self.boot.data_ptr()
        # the header's page-locked twin, as the collector publishes it: written in place from the device
        self.pub_src = dev(c["pub_src"].view(np.int32))
        self.pub_dst = torch.full((max(c["publish"], 1) + GUARD,), -7, dtype=torch.int32).pin_memory()
        if c["publish"]:
            a.publish_dst, a.publish_src, a.publish_words = self.pub_dst.data_ptr(), self.pub_src.data_ptr(), c["publish"]
        if norm:
            self.norm_state = dev(G.norm_state_vec(c["state"]))
            self.policy_obs = dev(c["policy_obs"])
            ws = torch.zeros(_C.lib().trl_rollout_norm_workspace(N), dtype=torch.float64, device=DEV)
            keep.append(ws)
            a.norm_state, a.policy_obs, a.norm_workspace = self.norm_state.data_ptr(), self.policy_obs.data_ptr(), ws.data_ptr()
            a.norm_clip, a.norm_update, a.normalize_partial_reset = c["norm_clip"], c["norm_update"], c["partial_reset"]
        if entry == "cat":
            _C.rollout_cat(a, 0xC0FFEE, 0, DEV)
        elif entry == "sd":
            _C.rollout_sd(a, DEV)
        else:
            _C.rollout(a, DEV)
        torch.cuda.synchronize()
        self.keep = keep
        if norm:
            assert int(ws.view(torch.int32)[2].item()) == 0, "the rendezvous raised its error word"


def check_pair(c, free, twin, reward_twin):
    """The critic-free launch `free` against its with-critic twin(s) and the invariants of the module docstring."""
    T, N, rr = c["T"], c["N"], R.ring_rows(c)
    rest = [r for r in range(c["rows"]) if r not in rr]
    for k in KEYS:
        got = free.ring[k]
        if k == "values":
            assert bool((got[rr] == 0.0).all()) and not bool(torch.signbit(got[rr]).any()), "values of the stored cells"
        elif k == "rewards":
            assert torch.equal(got[rr], reward_twin.ring[k][rr]), k
        else:
            assert torch.equal(got[rr], twin.ring[k][rr]), k
        assert bool(torch.isfinite(got[rr]).all()), k
        assert bool(torch.isnan(got[rest]).all()), k + ": a ring row outside the launch was written"
    assert bool(torch.isfinite(twin.ring["values"][rr]).all())               # (the twin's value pass did run)
    for k in ("cur_obs", "t_env", "cur_step", "episode_idx", "ep_return"):
        assert torch.equal(free.state[k], twin.state[k]), k
    assert torch.equal(free.epoch_reward, twin.epoch_reward) and torch.equal(free.ep_count, twin.ep_count)
    assert torch.equal(free.ep_log.nan_to_num(-1.0), twin.ep_log.nan_to_num(-1.0))
    if c["boot"]:
        assert bool((free.boot[:N] == 0.0).all()) and bool(torch.isnan(free.boot[N:]).all()), "bootstrap row"
    else:
        assert bool(torch.isnan(free.boot).all())
    if c["publish"]:
        assert np.array_equal(free.pub_dst[:c["publish"]].numpy().view(np.uint32), c["pub_src"][:c["publish"]]), "header"
        assert bool((free.pub_dst[c["publish"]:] == -7).all()), "publish guard"


def run_both_settings(D, A, noise, T, N, rows, top, seed, entry="gauss"):
    # (1) nobody runs over the episode length: the rewards are the rollout's in both launches
    c = case(D, A, noise, T, N, rows, top, T + 4, seed, entry)
    free, twin = Launch(c, None), Launch(c, "net")
    check_pair(c, free, twin, twin)
    assert not bool(free.ring["terminals"][R.ring_rows(c)].any())
    # (2) everybody does, every second step: the value pass of the zero-network twin adds discount * 0 to the marked cells
    c = case(D, A, noise, T, N, rows, top, 2, seed + 1, entry)
    free, twin, zero = Launch(c, None), Launch(c, "net"), Launch(c, "zero")
    check_pair(c, free, twin, zero)
    rr = R.ring_rows(c)
    over = free.ring["terminals"][rr][..., 0].cpu().numpy() != 0
    assert over.sum() == (T // 2) * N and bool((zero.ring["values"][rr] == 0.0).all())
    assert not torch.equal(twin.ring["rewards"][rr], free.ring["rewards"][rr])        # (a critic does move the marked rewards)
    return c, free


@pytest.mark.parametrize("D,A,noise", [(17, 6, "host"), (5, 3, "device")], ids=["D17A6-host", "D5A3-device"])
@pytest.mark.parametrize("T,N,rows,top", SHAPES)
def test_gaussian_rollout_without_a_critic(T, N, rows, top, D, A, noise):
    c, free = run_both_settings(D, A, noise, T, N, rows, top, 500 + 7 * N + D)
    # the stored rewards are the raw env rewards: the restatement, teacher-forced on the stored observations and actions
    rr, M = R.ring_rows(c), T * N
    g = {k: free.ring[k][rr].cpu().numpy() for k in ("obs", "acts", "rewards")}
    st = R.step_terms(c, g["obs"].reshape(M, D), g["obs"].reshape(M, D), c["eps"].reshape(M, A), g["acts"].reshape(M, A))
    ratio = float((np.abs(g["rewards"].reshape(M).astype(np.float64) - st["reward"]) / st["b_rew"]).max())
    print("T %d N %d D %d: raw reward worst err / bound %.3f" % (T, N, D, ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize("D,A,noise", [(17, 6, "device"), (5, 3, "host")], ids=["D17A6-device", "D5A3-host"])
def test_the_other_noise_mode_of_each_instantiation(D, A, noise):
    run_both_settings(D, A, noise, 3, 20, 4, 3, 700 + D)


@pytest.mark.parametrize("entry,D,A,noise", [("cat", 17, 6, "device"), ("sd", 17, 3, "host")], ids=["categorical", "state-std"])
def test_categorical_and_state_std_entry_points(entry, D, A, noise):
    c, free = run_both_settings(D, A, noise, 3, 20, 4, 3, 800 + D + A, entry)
    acts = free.ring["acts"][R.ring_rows(c)]
    if entry == "cat":
        assert acts.shape[-1] == 1 and bool(((acts >= 0) & (acts < A) & (acts == acts.round())).all())
    else:
        assert acts.shape[-1] == A and bool((acts.abs() <= 1.0).all())


@pytest.mark.parametrize("update", [1, 0])
def test_normalised_rollout_without_a_critic(update):
    """The cooperative NORM instantiation reads no value parameters either: one step of 40 envs with a running normaliser,
    bit-equal to the with-critic launch in everything but `values`, the statistics included."""
    c = R.norm_case("tanh", 40, 240, update=update, reset_env=7, partial_reset=1 - update)
    c.update(boot=True, publish=7, pub_src=np.arange(11, 18, dtype=np.uint32))
    free, twin = Launch(c, None, norm=True), Launch(c, "net", norm=True)
    check_pair(c, free, twin, twin)
    assert torch.equal(free.norm_state, twin.norm_state) and torch.equal(free.policy_obs, twin.policy_obs)
    assert update == int(not np.array_equal(free.norm_state.cpu().numpy(), G.norm_state_vec(c["state"])))
