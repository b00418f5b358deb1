"""One-launch rollouts for 128- and 256-wide networks (trl_rollout_synth_wide_f32; rollout_wide_kernel / value_pass_wide_kernel,
torchrl_amd/csrc/k_rollout_wide.hip): every stored cell against the float64 restatement of tests/_rollout_ref.py (teacher-forced,
the bounds of the 64-wide tests unchanged), the value pass alone, two launches over one state, the collector's opt-in route
against the per-step collection, whole PPO / A2C iterations, and the refusals.

Measured worst err / bound per quantity: profiles/NOTES_wide_rollout.md."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _gauss_sd_rollout_ref as rr                                            # noqa: E402
import _rollout_ref as R                                                      # noqa: E402
from _rollout_launch import DEV, Launcher, check                              # noqa: E402
from test_layernorm_rollout_gpu import RING_KEYS, _Log, collect               # noqa: E402

pytestmark = pytest.mark.gpu
SWITCH = "TRL_WIDE_FUSED_ROLLOUT"                                             # the fused route is opt-in
HEAD_ID = {"gauss": 0, "cat": 1, "sd": 2}


def wide_case(H, head, D, A, act, N, T, noise, seed, **kw):
    """`R.rollout_case` with H-wide nets: oracle.nets.init_mlp at [H, H] under the head scaling of `R.make_nets`."""
    c = R.rollout_case(D, A, act, head != "cat", N, T, seed, noise=noise, head=head, **kw)
    gen = torch.Generator().manual_seed(seed)
    pf, vf = R.nets.init_mlp(D, [H, H], 2 * A if head == "sd" else A, generator=gen), R.nets.init_mlp(D, [H, H], 1, generator=gen)
    pf[4], pf[5], vf[4] = pf[4] * 30.0, pf[5] * 100.0, vf[4] * 100.0
    if head == "sd":
        pf[5][A:] = -1.5
    return dict(c, pf=pf, vf=vf, H=H)


def launch(run, zero_net=False, edit=None):
    """The case's descriptor at its own width through `_C.rollout_wide` -> the run read back (guards checked)."""
    from torchrl_amd import _C
    a, c = run.args(), run.c
    a.H = c["H"]
    if zero_net:
        a.vf_params = None
    if edit:
        edit(a)
    _C.rollout_wide(a, HEAD_ID[R.head_of(c)], c.get("cat_seed", 0), c.get("env_offset", 0), DEV)
    torch.cuda.synchronize()
    return run.read()


# ---------------------------------------------------------------- 1. stored cells against float64
# pairwise over D in {3, 17, 18, 32} x A in {head minimum, 6, 8} x act x N in {16, 17, 40} x T in {1, 5} x every noise mode of the
# head, both widths under every head: partial env tiles, both input tiles, both halves of the head tile, one and two (four) row
# tiles per wave, a ring that wraps inside the launch, envs out of step (R.plant_counters)
CELL_CASES = [(128, "gauss", 3, 1, "tanh", 16, 1, "host"), (256, "gauss", 17, 6, "relu", 17, 5, "device"),
              (128, "gauss", 18, 8, "relu", 40, 5, "det"), (256, "gauss", 32, 8, "tanh", 40, 5, "host"),
              (128, "gauss", 17, 6, "tanh", 17, 5, "device"), (256, "cat", 3, 2, "relu", 17, 5, "device"),
              (128, "cat", 17, 8, "tanh", 40, 5, "det"), (256, "cat", 18, 6, "tanh", 16, 1, "device"),
              (128, "cat", 32, 6, "relu", 17, 5, "device"), (128, "sd", 3, 6, "relu", 40, 5, "host"),
              (256, "sd", 17, 1, "tanh", 16, 5, "device"), (128, "sd", 18, 8, "tanh", 17, 1, "det"),
              (256, "sd", 32, 8, "relu", 40, 5, "host")]


@pytest.mark.parametrize("spec", CELL_CASES, ids=["H%d-%s-D%d-A%d-%s-N%d-T%d-%s" % s for s in CELL_CASES])
def test_stored_cells_vs_float64(spec, errlog):
    c = wide_case(*spec, seed=700 + CELL_CASES.index(spec))
    res = R.verify(c, launch(Launcher(c)))
    check(res, "wide cells %s" % (spec,), errlog)
    if spec[1] == "cat":
        assert res["_share_borderline"] <= R.BORDERLINE_CAP


# ---------------------------------------------------------------- 2. the value pass alone
# M = T N below one tile (one workgroup copies 5000 publish words); tiles that straddle time rows; exact tiles; no marker at all;
# no boot row; more rounds than the grid has workgroups, over-length cells in both passes over the grid (R.big_counters)
VALUE_CASES = [(128, "M6"), (256, "M540"), (128, "M80"), (256, "M540-wide"), (128, "quiet"), (256, "noboot"),
               (256, dict(D=17, A=6, act="tanh", tanh=True, N=530, T=17, seed=78, counters=R.big_counters, ep_cap=8))]


@pytest.mark.parametrize("H,kw", VALUE_CASES, ids=["H%d-%s" % (h, k if isinstance(k, str) else "rounds") for h, k in VALUE_CASES])
def test_value_pass_vs_float64(H, kw, errlog):
    kw = dict(dict(R.VALUE_CASES)[kw]) if isinstance(kw, str) else dict(kw)
    kw.pop("tanh")
    c = wide_case(H, "gauss", *[kw.pop(k) for k in ("D", "A", "act", "N", "T")], "host", kw.pop("seed"), **kw)
    check(R.verify(c, launch(Launcher(c))), "wide value pass H=%d M=%d" % (H, c["N"] * c["T"]), errlog)


def test_value_pass_without_a_critic():
    """vf_params NULL (a ZeroNet): values and the boot row are zeros, the rewards of cells that were not flagged and everything
    the rollout stores are the bits of the launch with a critic, the header is published."""
    c = wide_case(256, "gauss", 17, 6, "tanh", 45, 12, "host", 79)
    with_vf, without = launch(Launcher(c)), launch(Launcher(c), zero_net=True)
    rows = R.ring_rows(c)
    assert (without["values"][rows] == 0.0).all() and (without["boot"] == 0.0).all()
    assert (without["pub_dst"] == c["pub_src"][:c["publish"]]).all()
    for k in ("obs", "next_obs", "acts", "terminals", "time_limits", "old_logp"):
        assert np.array_equal(without[k][rows], with_vf[k][rows]), k
    plain = with_vf["terminals"][rows] == 0.0
    assert plain.any() and not plain.all() and np.array_equal(without["rewards"][rows][plain], with_vf["rewards"][rows][plain])


# ---------------------------------------------------------------- 3. two launches continue one state
@pytest.mark.parametrize("H,head", [(128, "gauss"), (256, "cat"), (256, "sd")])
def test_two_launches_continue_one_state(H, head, errlog):
    """Device noise keyed from noise_step0 = 100; the second launch (7 steps) continues the key, the ring and the env state the
    first one persisted on the device."""
    c = wide_case(H, head, 17, 6, "tanh", 40, 5, "device", 480 + H, noise_step0=100, rows=15, top=8)
    run = Launcher(c)
    o = launch(run)
    check(R.verify(c, o), "wide %s launch 1" % head, errlog)
    run.c = R.continue_case(c, o, T=7)
    for v in run.ring.values():
        v.fill_(R.SENT)
    run.ep_count.zero_()
    run.ep_log.fill_(R.SENT)
    check(R.verify(run.c, launch(run)), "wide %s launch 2" % head, errlog)


# ---------------------------------------------------------------- 4. the collector's route
def make_collector(head, hidden, D, A, N, T, horizon, seed, noise_mode, add_ln=False, obs_norm=False):
    from torchrl_amd import networks, policies
    from torchrl_amd.collector.on_policy import VecOnPolicyCollector
    from torchrl_amd.env import get_vec_env
    from torchrl_amd.env.synth import SynthVecEnv
    from torchrl_amd.replay_buffers.on_policy import OnPolicyReplayBuffer
    torch.manual_seed(seed)
    net = dict(hidden_shapes=list(hidden), append_hidden_shapes=[], base_type=networks.MLPBase, add_ln=add_ln,
               activation_func=torch.nn.Tanh)
    if head == "gauss":
        pf = policies.GuassianContPolicyBasicBias(input_shape=D, output_shape=A, tanh_action=True, **net)
    elif head == "cat":
        pf = policies.CategoricalDisPolicy(input_shape=D, output_shape=A, **net)
    else:
        pf = policies.GuassianContPolicy(input_shape=D, output_shape=2 * A, tanh_action=True, **net)
    vf = networks.Net(input_shape=(D,), output_shape=1, **net)
    with torch.no_grad():
        for n_ in (pf, vf):
            n_.seq_append_fcs[-1].weight.mul_(30.0)
    if obs_norm:
        env, eval_env = (get_vec_env("SynthHalfCheetah-v0", {"reward_scale": 1, "obs_norm": True}, N, device=DEV) for _ in range(2))
    else:
        env, eval_env = (SynthVecEnv(N, obs_dim=D, act_dim=A, device=DEV, discrete=head == "cat") for _ in range(2))
    for e in (env, eval_env):
        e.horizon = horizon
    env.seed(seed)
    buf = OnPolicyReplayBuffer(N * T, env_nums=N, time_limit_filter=True)
    col = VecOnPolicyCollector(vf, env=env, eval_env=eval_env, pf=pf, replay_buffer=buf, device=DEV, train_render=False,
                               epoch_frames=N * T, max_episode_frames=999, eval_episodes=1, noise_mode=noise_mode)
    return pf, vf, env, buf, col


def clean_env(monkeypatch, switch):
    for k in ("TRL_GENERIC_PPO", "TRL_NO_RT_ROLLOUT", "TRL_PREFETCH_NOISE", "TRL_LN_FUSED_ROLLOUT", SWITCH):
        monkeypatch.delenv(k, raising=False)
    if switch:
        monkeypatch.setenv(SWITCH, "1")


@pytest.mark.parametrize("H,head,D,A", [(128, "gauss", 17, 6), (256, "sd", 27, 8), (256, "cat", 17, 6)])
def test_fused_route_vs_per_step_collection(H, head, D, A, monkeypatch):
    """Switch set: the fused route, one `_C.rollout_wide` per rollout, no per-step launch sequence; switch unset: the per-step
    route (what the parent commit takes) on the same nets, env seed and Philox noise; ring, env state, episodes and greedy
    evaluation at the tolerances of the sibling fused-vs-per-step tests."""
    from torchrl_amd import _C
    N, T, horizon, seed = 33, 4, 3, 40 + H
    clean_env(monkeypatch, True)
    pf, vf, env, buf, col = make_collector(head, [H, H], D, A, N, T, horizon, seed, "device")
    assert col._spec == (D, H, A, _C.ACT_TANH) and col._wide and not col._ln        # (`_spec` is None on the parent commit)
    calls, real = [], _C.rollout_wide
    monkeypatch.setattr(_C, "rollout_wide", lambda *a: (calls.append(a[1]), real(*a))[1])
    monkeypatch.setattr(col, "_step_launches", lambda *a, **k: pytest.fail("a per-step launch sequence on the fused route"))
    fused, ev = collect(col, buf), col.eval_one_epoch()
    assert calls == [HEAD_ID[head]] * 2
    monkeypatch.undo()
    clean_env(monkeypatch, False)
    pf2, vf2, env2, buf2, col2 = make_collector(head, [H, H], D, A, N, T, horizon, seed, "device" if head == "cat" else "host")
    assert col2._spec is None and not col2._wide
    if head != "cat":
        col2._host_noise = lambda n, e: rr.device_noise(n, N, A, seed, step0=col2.global_step).to(e.device).contiguous()
    step, ev2 = collect(col2, buf2), col2.eval_one_epoch()
    for k, (rtol, atol) in rr.TOL.items():
        ratio, err = rr.worst_ratio(fused[k], step[k], rtol, atol)
        print("H%d %s %s: max abs err %.3e, worst err / bound %.4f" % (H, head, k, err, ratio))
        assert ratio <= 1.0, k
    assert fused["terminals"].sum() > 0 and fused["episodes"] and len(fused["episodes"]) == len(step["episodes"])
    np.testing.assert_allclose(fused["episodes"], step["episodes"], rtol=0, atol=1e-5 * horizon)
    assert fused["epoch_reward"] == pytest.approx(step["epoch_reward"], abs=1e-5 * T * N)
    np.testing.assert_allclose(env.cur_obs.cpu().numpy(), env2.cur_obs.cpu().numpy(), rtol=0, atol=1e-5)
    for k in ("t_env", "cur_step", "episode_idx"):
        assert torch.equal(getattr(env, k).cpu(), getattr(env2, k).cpu()), k
    assert len(ev["eval_rewards"]) == N and ev["eval_traj_length"] == ev2["eval_traj_length"] == horizon
    np.testing.assert_allclose(ev["eval_rewards"], ev2["eval_rewards"], rtol=0, atol=1e-5 * horizon)


def test_what_stays_on_the_per_step_route(monkeypatch):
    clean_env(monkeypatch, True)
    mk = lambda hidden, **kw: make_collector("gauss", hidden, 17, 6, 16, 4, 9, 50, "device", **kw)[4]
    assert mk([128, 128])._wide and mk([256, 256])._wide
    for col in (mk([128, 128], add_ln=True), mk([128, 128], obs_norm=True), mk([128, 256]), mk([192, 192])):
        assert col._spec is None and not col._wide
    assert mk([64, 64])._spec is not None and not mk([64, 64])._wide               # the 64-wide kernel keeps its pairs
    monkeypatch.setenv("TRL_NO_RT_ROLLOUT", "1")
    assert mk([128, 128])._spec is None


@pytest.mark.parametrize("algo,H", [("PPO", 128), ("A2C", 256)])
def test_whole_iterations_on_the_fused_collection(algo, H, monkeypatch):
    """The rollout reads the block the generic engine steps: `flat_params()` is a view of the engine's flat vector."""
    from torchrl_amd import _C, algo as algos
    clean_env(monkeypatch, True)
    N, T = 32, 16
    np.random.seed(4)
    pf, vf, env, buf, col = make_collector("gauss", [H, H], 17, 6, N, T, 9, 60, "device")
    assert col._wide
    logger = _Log()
    general = dict(tau=0.95, shuffle=True, discount=0.99, num_epochs=10, batch_size=256, gae=True, env=env, replay_buffer=buf,
                   collector=col, logger=logger, device=DEV, save_dir=None)
    if algo == "PPO":
        agent = algos.PPO(pf=pf, vf=vf, plr=3e-4, vlr=3e-4, clip_para=0.2, opt_epochs=2, entropy_coeff=0.005, **general)
    else:
        agent = algos.A2C(pf=pf, vf=vf, plr=3e-4, vlr=1e-3, entropy_coeff=0.01, **general)
    eng = agent.engine()
    before, p0 = _C.eager_fallback_count(), pf.flat_params().clone()
    for epoch in range(2):
        assert pf.flat_params().data_ptr() == eng.flat.data_ptr() and vf.flat_params().data_ptr() == eng.flat.data_ptr() + 4 * eng.P_pf
        res = col.train_one_epoch()
        agent.current_epoch = epoch
        agent.update_per_epoch()
        assert np.isfinite(res["train_epoch_reward"]) and len(res["train_rewards"]) > 0
    torch.cuda.synchronize()
    assert len(logger.infos) > 0 and all(np.isfinite(list(i.values())).all() for i in logger.infos)
    assert _C.eager_fallback_count() == before and not torch.equal(p0, pf.flat_params())


# ---------------------------------------------------------------- 5. refusals
@pytest.mark.parametrize("what,edit,match", [
    ("H64", lambda a: setattr(a, "H", 64), "outside the head's range"), ("H192", lambda a: setattr(a, "H", 192), "outside the head's range"),
    ("D33", lambda a: setattr(a, "D", 33), "outside the head's range"), ("A9", lambda a: setattr(a, "A", 9), "outside the head's range"),
    ("norm_state", lambda a: setattr(a, "norm_state", 64), "no running observation normaliser")])
def test_refusals_launch_nothing(what, edit, match):
    from torchrl_amd import _C
    lib, act = _C.lib(), _C.ACT_TANH
    assert lib.trl_rollout_wide_supported(0, 17, 128, 6, act) == 1 and lib.trl_rollout_wide_supported(2, 32, 256, 8, act) == 1
    assert not any(lib.trl_rollout_wide_supported(0, D, H, A, act) for D, H, A in ((17, 64, 6), (17, 192, 6), (33, 128, 6), (17, 128, 9)))
    assert lib.trl_rollout_wide_supported(1, 17, 128, 1, act) == 0 and lib.trl_rollout_wide_supported(0, 17, 128, 6, 99) == 0
    run = Launcher(wide_case(128, "gauss", 17, 6, "tanh", 17, 5, "host", 90))
    with pytest.raises(_C.TrlError, match=match):
        launch(run, edit=edit)
    torch.cuda.synchronize()
    assert run.untouched()
