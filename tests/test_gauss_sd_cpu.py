"""State-dependent-std Gaussian policies on the CPU side: the torch restatement of the kernels' arithmetic
(tests/_gauss_sd_ref.py) reproduces the reference fixture (tests/golden/gauss_sd_update.npz, written by
tests/golden/make_golden_gauss_sd.py from the reference's own GuassianContPolicy / A2C / PPO), the product's policy class
draws the reference's initial parameters and follows its protocol, and the new refusals raise with their messages."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import _gauss_sd_ref as ref                                                   # noqa: E402


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(REPO, "tests", "golden", "gauss_sd_update.npz"))


def assert_info(info, g, prefix):
    """rel 1e-4 / abs 1e-5 on every key the reference logged."""
    want = ref.info_of(g, prefix)
    assert sorted(info) == sorted(want)
    for k in want:
        assert info[k] == pytest.approx(want[k], rel=1e-4, abs=1e-5), k


def assert_params(got, g, prefix):
    err = max((a.detach() - b).abs().max().item() for a, b in zip(got, ref.params_from(g, prefix)))
    print("%s max parameter error %.3e" % (prefix, err))
    assert err <= 1e-6, (prefix, err)


def test_fixture_covers_the_clip_the_norm_clip_and_the_upper_clamp(g):
    r = ref.info_of(g, "t_s17_ppo_info0")
    assert r["ratio/max"] > 1.2 and r["ratio/min"] < 0.8 and r["grad_norm/pf"] > 0.5
    assert ref.info_of(g, "n_s17_ppo_info0")["log_std/max"] == 2.0
    raw = g["n_s17_upd_log_std"]
    assert 0 < (raw == 2.0).sum() < raw.size


@pytest.mark.parametrize("tag", ref.TAGS)
def test_restatement_policy_outputs_match_reference(g, tag):
    tanh = bool(g[f"{tag}_args"][4])
    pf = ref.MLP(ref.params_from(g, f"{tag}_pf0_"))
    obs, acts = torch.from_numpy(g[f"{tag}_batch_obs"]), torch.from_numpy(g[f"{tag}_batch_acts"])
    with torch.no_grad():
        head = pf(obs)
        lp, ent = ref.logp(head, acts, tanh)
        mean, ls, _ = ref.parts(head)
        det, _ = ref.explore(head, None, tanh)
    np.testing.assert_allclose(mean.numpy(), g[f"{tag}_upd_mean"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(ls.numpy(), g[f"{tag}_upd_log_std"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(lp.numpy()[:, None], g[f"{tag}_upd_log_prob"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(ent.numpy()[:, None], g[f"{tag}_upd_ent"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(det.numpy(), g[f"{tag}_eval_act"], rtol=0, atol=1e-6)


@pytest.mark.parametrize("tag", ref.TAGS)
def test_restatement_a2c_update_matches_reference(g, tag):
    o = ref.SdUpdate(ref.params_from(g, f"{tag}_pf0_"), ref.params_from(g, f"{tag}_vf0_"), plr=3e-4, vlr=1e-3,
                     entropy_coeff=0.01, tanh=bool(g[f"{tag}_args"][4]))
    info = o.update(ref.batch_of(g, tag), ref.LOSS_A2C)
    assert_info(info, g, f"{tag}_a2c_info")
    assert_params(o.pf.params, g, f"{tag}_a2c_pf1_")
    assert_params(o.vf.params, g, f"{tag}_a2c_vf1_")


@pytest.mark.parametrize("tag", ref.TAGS)
def test_restatement_ppo_chain_matches_reference(g, tag):
    o = ref.SdUpdate(ref.params_from(g, f"{tag}_pf0_"), ref.params_from(g, f"{tag}_vf0_"), plr=3e-4, vlr=3e-4,
                     entropy_coeff=0.005, tanh=bool(g[f"{tag}_args"][4]), clip_para=0.2,
                     target_params=ref.params_from(g, f"{tag}_ppo_tpf0_"))
    for s, clipv in enumerate(g[f"{tag}_ppo_clipv"]):
        info = o.update(ref.batch_of(g, tag), ref.LOSS_PPO_CLIP, clipped_value_loss=bool(clipv))
        assert_info(info, g, f"{tag}_ppo_info{s}")
        assert_params(o.pf.params, g, f"{tag}_ppo_pf{s + 1}_")
        assert_params(o.vf.params, g, f"{tag}_ppo_vf{s + 1}_")


def test_restatement_gradients_in_float64_are_the_closed_form():
    """A check of the ORACLE, not of the kernels (it passes on a build without them): autograd on the restatement's
    objective == the formulas the kernel header states, the clamp gate included -- so that the float64 gradients the GPU
    tests compare the kernels with are the stated ones."""
    rs = np.random.RandomState(3)
    B, A = 40, 3
    head = torch.from_numpy(rs.randn(B, 2 * A))
    head[:5, A] = -25.0
    head[5:9, A + 1] = 3.0
    acts = ref.explore(head, torch.from_numpy(rs.randn(B, A)), False)[0]
    advs, rets, v = (torch.from_numpy(rs.randn(B)) for _ in range(3))
    old = ref.logp(head, acts, False)[0] + 0.3 * torch.from_numpy(rs.randn(B))
    r = ref.losses(head, v, acts, advs, rets, None, old, 0.2, 0.01, False, ref.LOSS_PPO_CLIP, False)
    mean, ls, std = ref.parts(head)
    advn = ref.adv_normalize(advs)
    ratio = r["ratio"]
    g_lp = torch.where(ratio * advn <= ratio.clamp(0.8, 1.2) * advn, -advn * ratio / B, torch.zeros_like(ratio))[:, None]
    zc, ivv = acts - mean, torch.exp(-2 * ls)
    gate = ((head[:, A:] >= -20) & (head[:, A:] <= 2)).double()
    want = torch.cat([g_lp * zc * ivv, gate * (g_lp * (zc * zc * ivv - 1) - 0.01 / B)], dim=1)
    assert torch.isfinite(r["d_head"]).all()
    np.testing.assert_allclose(r["d_head"].numpy(), want.numpy(), rtol=1e-9, atol=1e-12)
    assert (r["d_head"][:5, A] == 0).all() and (r["d_head"][5:9, A + 1] == 0).all()


@pytest.mark.parametrize("tag", ref.TAGS)
def test_policy_constructs_with_the_reference_draw_and_follows_its_protocol(g, tag):
    from torchrl_amd import networks, policies
    D, A, H, B, tanh = (int(x) for x in g[f"{tag}_args"])
    torch.manual_seed(5 + D)
    net = dict(hidden_shapes=[H, H], append_hidden_shapes=[], base_type=networks.MLPBase, activation_func=torch.nn.Tanh)
    pf = policies.GuassianContPolicy(input_shape=D, output_shape=2 * A, tanh_action=bool(tanh), **net)
    vf = networks.Net(input_shape=(D,), output_shape=1, **net)
    assert pf.continuous is True and not hasattr(pf, "logstd")
    sd = vf.state_dict()
    for k, v in sd.items():
        assert np.array_equal(v.numpy(), g[f"{tag}_vf0_" + k.replace(".", "__")]), k
    # the fixture's policy is that draw with its log_std rows overwritten: load it, then the CPU protocol (torch modules;
    # the kernels take over on a GPU)
    pf.load_state_dict({k: torch.from_numpy(g[f"{tag}_pf0_" + k.replace(".", "__")].copy()) for k in pf.state_dict()})
    obs, acts = torch.from_numpy(g[f"{tag}_batch_obs"]), torch.from_numpy(g[f"{tag}_batch_acts"])
    with torch.no_grad():
        out = pf.update(obs, acts)
        ex = pf.explore(obs, return_log_probs=True)
    assert out["log_prob"].shape == (B, 1) and out["ent"].shape == (B, 1)
    for k in ("mean", "log_std", "log_prob", "ent"):
        np.testing.assert_allclose(out[k].numpy(), g[f"{tag}_upd_{k}"], rtol=1e-5, atol=2e-6, err_msg=k)
    np.testing.assert_allclose(pf.eval_act(obs), g[f"{tag}_eval_act"], rtol=0, atol=1e-6)
    assert ex["action"].shape == (B, A) and ex["log_prob"].shape == (B, 1)


def _sd_nets(A=2, D=4):
    from torchrl_amd import networks, policies
    net = dict(base_type=networks.MLPBase, hidden_shapes=[8, 8])
    return (policies.GuassianContPolicy(input_shape=D, output_shape=2 * A, tanh_action=True, **net),
            networks.Net(input_shape=(D,), output_shape=1, **net))


class _Stub:
    epoch_frames = 0


def _agent(cls, pf, vf, **kw):
    from oracle.synth_env import SynthVecEnvCPU
    return cls(pf=pf, vf=vf, tau=0.95, shuffle=True, discount=0.99, num_epochs=10, batch_size=8, gae=True,
               env=SynthVecEnvCPU(4), replay_buffer=None, collector=_Stub(), logger=None, device=torch.device("cpu"),
               save_dir=None, **kw)


def test_trpo_and_vmpo_refuse_the_head():
    from torchrl_amd import _C
    from torchrl_amd.algo import TRPO, VMPO
    pf, vf = _sd_nets()
    with pytest.raises(_C.TrlError, match="TRPO with a state-dependent-std policy is not built"):
        TRPO(max_kl=0.01, cg_damping=0.1, v_opt_times=1, cg_iters=10, residual_tol=1e-10, pf=pf, vf=vf)
    with pytest.raises(_C.TrlError, match="VMPO with a state-dependent-std policy is not built"):
        VMPO(pf=pf, vf=vf)


def test_engine_selection_and_refusals_on_the_cpu(monkeypatch):
    """The head is routed to the generic engine -- which, without a GPU, says so (the old message named the policy as
    unsupported) -- and refuses several ranks and more than 32 action dimensions before it looks at the device."""
    from torchrl_amd import _C, dist
    from torchrl_amd.algo import A2C, PPO
    from torchrl_amd.algo.on_policy import ppo as ppo_mod
    pf, vf = _sd_nets()
    assert ppo_mod.is_state_std(pf) and not ppo_mod.is_state_std(vf)
    for cls in (A2C, PPO):
        with pytest.raises(_C.TrlError, match="needs a GPU"):
            _agent(cls, *_sd_nets()).engine()
    monkeypatch.setattr(dist, "collectives_active", lambda: True)
    with pytest.raises(_C.TrlError, match="PPO / A2C with a state-dependent-std policy runs on one rank"):
        _agent(PPO, *_sd_nets()).engine()
    monkeypatch.undo()
    with pytest.raises(_C.TrlError, match="1 <= A <= 32"):
        _agent(A2C, *_sd_nets(A=33)).engine()
    # the bindings refuse the same sizes before they touch a pointer, and the library has no workspace for them
    head = torch.zeros(4, 66)
    for call in (lambda: _C.gauss_sd_explore(head, None, False), lambda: _C.gauss_sd_logp(head, torch.zeros(4, 33), False),
                 lambda: _C.gauss_sd_losses(head, *([None] * 13), info=None)):
        with pytest.raises(_C.TrlError, match="1 <= A <= 32"):
            call()
    assert _C.lib().trl_gauss_sd_losses_workspace(64, 33) < 0 and _C.lib().trl_gauss_sd_losses_workspace(64, 0) < 0
    assert _C.lib().trl_gauss_sd_losses_workspace(300, 32) == 2 * 21
    assert _C.lib().trl_gauss_sd_explore_f32(None, None, None, None, 4, 33, 0, None) != 0
    assert "1 <= A <= 32" in _C.lib().trl_last_error().decode()
