"""REINFORCE without a GPU: the float64 restatement (tests/_reinforce_ref.py) against the reference's fixture
(tests/golden/reinforce_update.npz), the population `advs/std`, returns == advantages under a zero critic, the new
loss-mode constant and the host-side argument checks of the entry points that take it (every case returns before anything
is launched), and the constructor's refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _reinforce_ref as R                                                    # noqa: E402

EINVAL = -1
FAKE = 0x1000


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(HERE, "golden", "reinforce_update.npz"))


@pytest.fixture(scope="module")
def built_lib():
    from torchrl_amd import build
    return build.build(verbose=False)


@pytest.mark.parametrize("tag", list(R.HEADS))
def test_restatement_reproduces_the_fixture(g, tag):
    """Two chained updates in float64 against the reference's float32 run: info scalars rel 1e-4 / abs 1e-5, parameters abs
    1e-6 per update; Adam's moments, which are sums of gradients of size <= 0.5 (the clip), within the same
    absolute bound."""
    assert "torch" in str(g["meta"]) and "numpy" in str(g["meta"])
    upd = R.restatement_of(g, tag)
    assert upd.opt.param_groups[0]["eps"] == 1e-8
    for s in range(2):
        info = upd.update(R.batch_of(g, tag))
        want = R.info_of(g, tag, s)
        assert list(info) == R.INFO_KEYS == list(want)
        worst = R.info_close(info, want)
        err = R.state_error(g, f"{tag}_pf{s + 1}_", upd.params)
        m, v = upd.moments()
        err_m, err_v = R.state_error(g, f"{tag}_adam{s + 1}_m_", m), R.state_error(g, f"{tag}_adam{s + 1}_v_", v)
        print("%s update %d: info err / bound %.3f, params %.3e, exp_avg %.3e, exp_avg_sq %.3e" % (tag, s, worst, err, err_m, err_v))
        assert worst <= 1.0, (info, want)
        assert err <= 1e-6 * (s + 1) and err_m <= 1e-6 and err_v <= 1e-6


@pytest.mark.parametrize("tag", list(R.HEADS))
def test_advs_std_is_the_population_std(g, tag):
    advs = g[f"{tag}_batch_advs"].astype(np.float64)
    B = advs.size
    assert B == 64
    logged = R.info_of(g, tag, 0)["advs/std"]
    pop, unbiased = advs.std(), advs.std(ddof=1)
    assert logged == pytest.approx(pop, rel=1e-6)
    assert abs(unbiased - pop) > 1e-3 * pop and abs(logged - unbiased) > 100 * abs(logged - pop)
    # ... and what the engines compute from the raw statistics {sum, sumsq, max, -min}
    raw = R.raw_of(torch.from_numpy(g[f"{tag}_batch_advs"]))
    assert R.population_std(raw, B) == pytest.approx(pop, rel=1e-12)


def test_zero_critic_returns_are_the_advantages(g):
    T, N, gamma = int(g["disc_args"][0]), int(g["disc_args"][1]), float(g["disc_args"][2])
    assert (T, N) == (16, 8)
    d, tl = g["disc_terminals"], g["disc_time_limits"]
    assert tl.any() and (d & ~tl).any() and bool(d[T - 1, 0]) and bool(tl[T - 1, 0])
    for filt in (0, 1):
        assert np.array_equal(g[f"disc{filt}_advs"], g[f"disc{filt}_rets"])
        want = R.discounted_returns(g["disc_rewards"], d, gamma)
        np.testing.assert_allclose(g[f"disc{filt}_rets"], want, rtol=1e-12, atol=1e-12)
    assert np.array_equal(g["disc0_rets"], g["disc1_rets"])


def test_loss_mode_is_exported(built_lib):
    from torchrl_amd import _C
    assert (_C.LOSS_PPO_CLIP, _C.LOSS_A2C, _C.LOSS_REINFORCE) == (0, 1, 2) == (R.LOSS_PPO_CLIP, R.LOSS_A2C, R.LOSS_REINFORCE)
    header = open(os.path.join(os.path.dirname(HERE), "include", "trl_hip.h")).read()
    assert "#define TRL_LOSS_REINFORCE 2" in header


def _batch(loss_mode):
    """A descriptor whose pointers are never dereferenced: every call below returns from the host-side checks."""
    from torchrl_amd import _C
    b = _C.PpoBatchArgs()
    for k in ("obs", "acts", "advs", "adv_raw", "pf_params", "partial", "scal_partial"):
        setattr(b, k, FAKE)
    b.rows_mb, b.N, b.n_global = 4, 16, 64.0
    b.D, b.H, b.A, b.act = 17, 64, 6, _C.ACT_TANH
    b.clip_para, b.entropy_coeff, b.loss_mode = 0.2, 0.01, loss_mode
    b.n_wg, b.n_wg_pf = 2, 2
    return b


@pytest.mark.parametrize("entry", ["trl_ppo_minibatch_grad_f32", "trl_ppo_cat_minibatch_grad_f32", "trl_ppo_sd_minibatch_grad_f32"])
def test_grad_launch_takes_the_mode_only_all_policy(built_lib, entry):
    from torchrl_amd import _C
    lib = _C.lib()
    fn = getattr(lib, entry)

    def bad(needle, mode=_C.LOSS_REINFORCE, **kw):
        b = _batch(mode)
        for k, v in kw.items():
            setattr(b, k, v)
        assert fn(C.byref(b), None) == EINVAL, kw
        assert needle in lib.trl_last_error(), lib.trl_last_error()

    bad(b"all-policy", n_wg_pf=1)                                             # a split launch
    bad(b"all-policy", n_wg_pf=0)                                             # the even split
    bad(b"all-policy", n_wg_pf=-1, vf_params=FAKE)                            # the value net alone
    bad(b"clipped_value_loss", clipped_value_loss=1)
    bad(b"clipped_value_loss", clipped_value_loss=1, old_values=FAKE)
    bad(b"null", obs=None)                                                    # what the policy pass does load stays required
    bad(b"null", advs=None)
    bad(b"null", pf_params=None)
    # the other two modes keep their requirements: no returns / no log pi_old is still refused there
    bad(b"null", mode=_C.LOSS_A2C)
    bad(b"null", mode=_C.LOSS_PPO_CLIP, old_logp=FAKE)
    bad(b"old_logp", mode=_C.LOSS_PPO_CLIP, rets=FAKE)


def test_loss_kernels_refuse_a_value_clip_in_the_mode(built_lib):
    """trl_ppo_generic_losses_f32 / trl_cat_losses_f32 / trl_gauss_sd_losses_f32 with pointers that are never dereferenced."""
    from torchrl_amd import _C
    lib = _C.lib()
    P, N_ = FAKE, None

    def gauss(mode, clipv, v=N_, rets=N_, v_old=N_, d_v=N_, old=N_):
        return lib.trl_ppo_generic_losses_f32(P, P, P, P, old, v, rets, v_old, P, 64.0, 64, 6, 0.2, 0.01, clipv, 1, mode, P, d_v, P,
                                              P, P, None)

    def cat(mode, clipv, v=N_, rets=N_, v_old=N_, d_v=N_, old=N_):
        return lib.trl_cat_losses_f32(P, P, P, old, v, rets, v_old, P, 64.0, 64, 6, 0.2, 0.01, clipv, mode, P, d_v, P, P, None)

    def sd(mode, clipv, v=N_, rets=N_, v_old=N_, d_v=N_, old=N_):
        return lib.trl_gauss_sd_losses_f32(P, P, P, old, v, rets, v_old, P, 64.0, 64, 6, 0.2, 0.01, clipv, 1, mode, P, d_v, P, P,
                                           None)

    for call in (gauss, cat, sd):
        assert call(_C.LOSS_REINFORCE, 1) == EINVAL and b"clipped_value_loss" in lib.trl_last_error()
        assert call(_C.LOSS_REINFORCE, 1, v=P, rets=P, v_old=P, d_v=P) == EINVAL and b"clipped_value_loss" in lib.trl_last_error()
        assert call(5, 0, v=P, rets=P, d_v=P, old=P) == EINVAL and b"loss_mode" in lib.trl_last_error()
        # A2C / PPO keep refusing a NULL v, rets or d_v, and PPO a NULL log pi_old
        for mode in (_C.LOSS_A2C, _C.LOSS_PPO_CLIP):
            assert call(mode, 0, old=P) == EINVAL and b"null" in lib.trl_last_error()
            assert call(mode, 0, v=P, rets=P, old=P) == EINVAL and b"null" in lib.trl_last_error()
            assert call(mode, 0, rets=P, d_v=P, old=P) == EINVAL and b"null" in lib.trl_last_error()
        assert call(_C.LOSS_PPO_CLIP, 0, v=P, rets=P, d_v=P) == EINVAL and b"old_logp" in lib.trl_last_error()
        assert call(_C.LOSS_A2C, 1, v=P, rets=P, d_v=P) == EINVAL and b"old values" in lib.trl_last_error()


def test_policy_fold_takes_a_one_group_optimiser(built_lib):
    """trl_ppo_reduce_adam_net_f32 (net 0) accepts [policy]; the joint fold and the value function's do not."""
    from torchrl_amd import _C
    lib = _C.lib()
    D, A = 17, 6
    p_pf = 64 * D + 64 + 4096 + 64 + 64 * A + A + A

    def adam(*sizes):
        a = _C.AdamArgs()
        a.params, a.grads, a.exp_avg, a.exp_avg_sq = FAKE, FAKE, FAKE, FAKE
        a.n_groups = len(sizes)
        for k, s in enumerate(sizes):
            a.group_sizes[k] = s
        a.max_norm, a.beta1, a.beta2, a.eps, a.grad_scale, a.step_count = 0.5, 0.9, 0.999, 1e-8, 1.0, 1
        return a
    net = lambda which, a: lib.trl_ppo_reduce_adam_net_f32(FAKE, FAKE, 2, which, D, 64, A, FAKE, FAKE, C.byref(a), FAKE, None)
    assert net(1, adam(p_pf)) == EINVAL and b"groups" in lib.trl_last_error()
    assert net(0, adam(p_pf + 1)) == EINVAL and b"groups" in lib.trl_last_error()
    assert lib.trl_ppo_reduce_adam_f32(FAKE, FAKE, 2, 1, D, 64, A, FAKE, FAKE, C.byref(adam(p_pf)), FAKE, None) == EINVAL
    assert b"groups" in lib.trl_last_error()


class _Stub:
    epoch_frames = 0


def _agent(pf, **kw):
    from oracle.synth_env import SynthVecEnvCPU
    from torchrl_amd.algo import Reinforce
    return Reinforce(pf=pf, plr=3e-3, shuffle=True, discount=0.99, num_epochs=10, batch_size=8, env=SynthVecEnvCPU(4),
                     replay_buffer=None, collector=_Stub(), logger=None, device=torch.device("cpu"), save_dir=None, **kw)


def _policies(D=4, A=2):
    from torchrl_amd import networks, policies
    net = dict(base_type=networks.MLPBase, hidden_shapes=[8, 8])
    return (policies.GuassianContPolicyBasicBias(input_shape=D, output_shape=A, tanh_action=True, **net),
            policies.GuassianContPolicy(input_shape=D, output_shape=2 * A, tanh_action=True, **net),
            policies.CategoricalDisPolicy(input_shape=D, output_shape=A, **net))


def test_constructor_and_refusals(monkeypatch):
    from torchrl_amd import _C, dist, networks
    from torchrl_amd.algo import Reinforce
    with pytest.raises(_C.TrlError, match="not built"):
        Reinforce()
    with pytest.raises(_C.TrlError, match="not built"):
        Reinforce(plr=3e-3)
    for pf in _policies():
        agent = _agent(pf, gae=True, entropy_coeff=0.002)
        assert isinstance(agent.vf, networks.ZeroNet) and agent.networks == [agent.pf, agent.vf]
        assert agent.gae is False and agent.entropy_coeff == 0.002 and agent.plr == 3e-3
        assert agent.snapshot_networks == [("pf", pf)]
        assert agent.pf_optimizer.param_groups[0]["eps"] == 1e-8 and agent.loss_mode == _C.LOSS_REINFORCE
        assert agent.sample_key == ["obs", "acts", "advs"]
        with pytest.raises(_C.TrlError, match="needs a GPU"):
            agent.engine()
        with pytest.raises(_C.TrlError, match="needs a GPU"):
            agent.update({"obs": np.zeros((8, 4), np.float32), "acts": np.zeros((8, 2), np.float32),
                          "advs": np.zeros((8, 1), np.float32)})
    with pytest.raises(_C.TrlError, match="Adam only"):
        _agent(_policies()[0], optimizer_class=torch.optim.RMSprop).engine()
    monkeypatch.setattr(dist, "collectives_active", lambda: True)
    with pytest.raises(_C.TrlError, match="Reinforce runs on one rank"):
        _agent(_policies()[0]).engine()
