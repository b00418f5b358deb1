"""SAC / TwinSAC (the soft actor-critics with a value network) without a GPU: the float64 restatement
(tests/_sac_v_ref.py) against the fixture the reference's own classes wrote, its gradients against CPU autograd, the
fixture's layout, the public names and the refusals that come before the device check."""
import inspect
import json

import numpy as np
import pytest
import torch

import _sac_v_ref as R


@pytest.fixture(scope="module")
def g():
    return R.load_fixture()


@pytest.mark.parametrize("tag", R.CASES)
def test_restated_update_reproduces_the_reference(g, tag):
    """Two chained updates by explicit chain rule in float64 against the reference's fp32 run: the bounds the GPU path
    is held to (info values rtol 2e-4 / atol 5e-5, parameters and target 3e-6, log_alpha 1e-6)."""
    up, B, steps = R.update_from_fixture(g, tag)
    for s in range(steps):
        batch = {k: g["%s_s%d_batch_%s" % (tag, s, k)] for k in R.BATCH_KEYS}
        info = up.update(batch, g["%s_s%d_eps" % (tag, s)])
        keys = [str(k) for k in g["%s_s%d_info_keys" % (tag, s)]]
        assert sorted(info) == keys
        np.testing.assert_allclose([info[k] for k in keys], g["%s_s%d_info_vals" % (tag, s)], rtol=2e-4, atol=5e-5)
    names = R.net_names(g, tag)
    mine = dict(zip(names, [up.pf] + up.qfs + [up.vf]), tvf=up.tvf)
    for name, layers in mine.items():
        for (w, b), (w_ref, b_ref) in zip(layers, R.layers_of(g, "%s_%s1_" % (tag, name))):
            assert np.abs(w - w_ref).max() < 3e-6 and np.abs(b - b_ref).max() < 3e-6, (tag, name)
    if tag + "_log_alpha" in g:
        np.testing.assert_allclose(up.log_alpha, g[tag + "_log_alpha"], atol=1e-6)
    else:
        assert up.log_alpha[0] == 0.0


@pytest.mark.parametrize("twin", [True, False])
def test_restated_loss_gradients_equal_autograd(twin):
    """dq, dv and dq_n of `losses_ref` against float64 autograd of the same three losses, with exact ties q1n == q2n
    (torch.min hands each side half) among the rows."""
    rs = np.random.RandomState(3)
    B, gamma, alpha = 37, 0.97, 0.3
    arr = lambda: rs.randn(B)
    q1, q2, tv, rew, v, q1n, q2n, logp = (arr() for _ in range(8))
    term = (rs.rand(B) < 0.3).astype(np.float64)
    q2n[::5] = q1n[::5]                                                   # planted ties
    if not twin:
        q2 = q2n = None
    ref = R.losses_ref(q1, q2, tv, rew, term, v, q1n, q2n, logp, alpha, gamma, B)
    t = lambda a, grad=False: None if a is None else torch.tensor(a, dtype=torch.float64, requires_grad=grad)
    Q1, Q2, V, Q1n, Q2n = t(q1, True), t(q2, True), t(v, True), t(q1n, True), t(q2n, True)
    qt = t(rew) + (1.0 - t(term)) * gamma * t(tv)
    qn = torch.min(Q1n, Q2n) if twin else Q1n
    losses = [((Q1 - qt) ** 2).mean(), ((V - (qn - alpha * t(logp)).detach()) ** 2).mean(), (alpha * t(logp) - qn).mean()]
    if twin:
        losses.append(((Q2 - qt) ** 2).mean())
    torch.stack(losses).sum().backward()
    pairs = [("dq1", Q1), ("dv", V), ("dq1n", Q1n)] + ([("dq2", Q2), ("dq2n", Q2n)] if twin else [])
    for key, leaf in pairs:
        np.testing.assert_allclose(ref[key], leaf.grad.numpy(), rtol=1e-13, atol=1e-15, err_msg=key)
    if twin:
        assert np.all(ref["dq1n"][::5] * B == -0.5) and np.all(ref["dq2n"][::5] * B == -0.5)
        assert np.all((ref["dq1n"] + ref["dq2n"]) * B == -1.0)
    want = [losses[0].item() * B, losses[3].item() * B if twin else 0.0, losses[1].item() * B, losses[2].item() * B, rew.sum()]
    np.testing.assert_allclose(ref["sums"], want, rtol=1e-13)


def test_restated_sample_equals_torch_distributions():
    """`samples_ref` against a TanhNormal written with torch.distributions, and its critic inputs."""
    rs = np.random.RandomState(5)
    B, D, A = 33, 4, 3
    head, eps, obs, acts = rs.randn(B, 2 * A), rs.randn(B, A), rs.randn(B, D), rs.randn(B, A)
    head[:, A:] *= 6.0                                                    # some log_std outside [-20, 2]
    new_a, logp, x_sa, x_new = R.samples_ref(head, eps, obs, acts)
    mean, ls = torch.tensor(head[:, :A]), torch.tensor(head[:, A:]).clamp(-20.0, 2.0)
    z = mean + ls.exp() * torch.tensor(eps)
    lp = torch.distributions.Normal(mean, ls.exp()).log_prob(z) - torch.log(1.0 - torch.tanh(z) ** 2 + 1e-6)
    np.testing.assert_allclose(new_a, torch.tanh(z).numpy(), rtol=1e-14, atol=1e-15)
    np.testing.assert_allclose(logp, lp.sum(1).numpy(), rtol=1e-9, atol=1e-9)
    assert np.array_equal(x_sa, np.concatenate([obs, acts], 1)) and np.array_equal(x_new, np.concatenate([obs, new_a], 1))


def test_fixture_layout(g):
    meta = json.loads(str(g["meta"]))
    assert meta["optimize"] == 1 and "torch" in meta and "numpy" in meta and "assert" in meta["why_optimize"]
    assert tuple(str(t) for t in g["cases"]) == R.CASES
    # the init seed is the first from 31 on at which the reference's own fp32 error leaves two thirds of the 3e-6 bound
    assert meta["reference_error_max"] == 1e-6 and meta["init_seed"] == 31 + len(meta["rejected_init_seeds"])
    assert all(err >= 1e-6 for err in meta["rejected_init_seeds"].values())
    want = {"sac_h128": ("SAC", 128, 256, 0.0, 0.0, 1), "twin_h128": ("TwinSAC", 128, 256, 0.0, 0.0, 1),
            "sac_reg": ("SAC", 64, 96, 1e-3, 1.0, 1), "twin_reg": ("TwinSAC", 64, 96, 1e-3, 1.0, 1),
            "twin_fixed": ("TwinSAC", 64, 96, 0.0, 0.0, 0)}
    for tag, (cls, H, B, w_reg, clip, tune) in want.items():
        assert str(g[tag + "_class"]) == cls
        assert g[tag + "_args"].tolist() == [H, B, w_reg, clip, tune, 2]
        names = R.net_names(g, tag)
        assert names == (("pf", "qf", "vf") if cls == "SAC" else ("pf", "qf1", "qf2", "vf"))
        shapes = {"pf": [(H, R.D), (H, H), (2 * R.A, H)], "vf": [(H, R.D), (H, H), (1, H)]}
        for name in names + ("tvf",):
            for stage in ("0", "1"):
                if name == "tvf" and stage == "0":
                    continue
                layers = R.layers_of(g, "%s_%s%s_" % (tag, name, stage))
                assert [w.shape for w, _ in layers] == shapes.get(name if name != "tvf" else "vf",
                                                                   [(H, R.D + R.A), (H, H), (1, H)]), (tag, name)
                assert all(b.shape == (w.shape[0],) for w, b in layers)
        for s in range(2):
            pre = "%s_s%d_" % (tag, s)
            for key, width in zip(R.BATCH_KEYS, (R.D, R.D, R.A, 1, 1)):
                assert g[pre + "batch_" + key].shape == (B, width) and g[pre + "batch_" + key].dtype == np.float32
            assert g[pre + "eps"].shape == (B, R.A)
            term = g[pre + "batch_terminals"]
            assert set(np.unique(term)) == {0.0, 1.0} and 0.1 < term.mean() < 0.3          # a fifth of them set
            keys = [str(k) for k in g[pre + "info_keys"]]
            assert g[pre + "info_vals"].shape == (len(keys),) and np.isfinite(g[pre + "info_vals"]).all()
            assert ("Alpha" in keys) == bool(tune) and ("Alpha_loss" in keys) == bool(tune)
            assert ("Training/vf_grad_norm" in keys) == (clip > 0) and "Training/vf_loss" in keys
            assert ("Training/qf_loss" in keys) == (cls == "SAC") and ("Training/qf2_loss" in keys) == (cls == "TwinSAC")
        assert (tag + "_log_alpha" in g) == bool(tune)
        # the target moved: it is not the initial V, and not the final one
        t1, v0, v1 = (R.layers_of(g, "%s_%s_" % (tag, n))[0][0] for n in ("tvf1", "vf0", "vf1"))
        assert np.abs(t1 - v0).max() > 0 and np.abs(t1 - v1).max() > 0


def test_exported_names_and_constructor_parameters():
    import torchrl.algo
    import torchrl_amd.algo
    import torchrl_amd.algo.off_policy as off
    from torchrl.algo import SAC, TwinSAC
    assert SAC is off.SAC is torchrl_amd.algo.SAC and TwinSAC is off.TwinSAC is torchrl_amd.algo.TwinSAC
    assert SAC.__module__ == "torchrl_amd.algo.off_policy.sac_v"
    tail = ["plr", "vlr", "qlr", "optimizer_class", "policy_std_reg_weight", "policy_mean_reg_weight", "reparameterization",
            "automatic_entropy_tuning", "target_entropy", "noise_mode", "kwargs"]
    assert list(inspect.signature(SAC.__init__).parameters) == ["self", "pf", "vf", "qf"] + tail
    assert list(inspect.signature(TwinSAC.__init__).parameters) == ["self", "pf", "vf", "qf1", "qf2"] + tail
    assert inspect.signature(SAC.__init__).parameters["noise_mode"].default == "host"
    for cls in (SAC, TwinSAC):
        for name in ("update", "update_deferred", "update_epoch_deferred", "resolve_updates", "static_batch", "log_alpha"):
            assert hasattr(cls, name), (cls, name)


def _nets(add_ln=False, twin=True):
    import torchrl.networks as networks
    import torchrl.policies as policies
    net = dict(hidden_shapes=[16, 16], append_hidden_shapes=[], base_type=networks.MLPBase, activation_func=torch.nn.ReLU)
    extra = dict(add_ln=True) if add_ln else {}
    nets = dict(pf=policies.GuassianContPolicy(input_shape=5, output_shape=4, tanh_action=True, **net),
                vf=networks.Net(input_shape=5, output_shape=1, **net, **extra))
    for name in (("qf1", "qf2") if twin else ("qf",)):
        nets[name] = networks.QNet(input_shape=7, output_shape=1, **net)
    return nets


def _agent(cls, nets, **kw):
    from oracle.synth_env import SynthVecEnvCPU

    class Stub:
        epoch_frames = 0
    args = dict(plr=3e-4, vlr=3e-4, qlr=3e-4, env=SynthVecEnvCPU(4), replay_buffer=None, collector=Stub(), logger=None,
                device=torch.device("cpu"), save_dir=None, batch_size=8)
    args.update(kw)
    return cls(**nets, **args)


@pytest.mark.parametrize("twin", [True, False])
def test_refusals_come_before_the_device_check(twin, monkeypatch):
    from torchrl_amd import _C, dist
    from torchrl.algo import SAC, TwinSAC
    cls = TwinSAC if twin else SAC
    with pytest.raises(NotImplementedError, match="reparameterization=False.*not built"):
        _agent(cls, _nets(twin=twin), reparameterization=False)
    with pytest.raises(_C.TrlError, match="torch.optim.Adam only, got SGD"):
        _agent(cls, _nets(twin=twin), optimizer_class=torch.optim.SGD)
    with pytest.raises(_C.TrlError, match="without LayerNorm"):
        _agent(cls, _nets(add_ln=True, twin=twin))
    with pytest.raises(ValueError, match="noise_mode"):
        _agent(cls, _nets(twin=twin), noise_mode="both")
    agent = _agent(cls, _nets(twin=twin))                                 # on the CPU: built, but there is no CPU path
    assert [n for n, _ in agent.snapshot_networks] == (["pf", "qf1", "qf2", "vf"] if twin else ["pf", "qf", "vf"])
    assert agent.target_networks == [(agent.vf, agent.target_vf)] and agent.networks[-1] is agent.target_vf
    assert len(agent.networks) == (5 if twin else 4) and agent.target_vf is not agent.vf
    assert agent.target_entropy == -6.0                                   # SynthVecEnvCPU: six action dimensions
    with pytest.raises(_C.TrlError, match="%s networks live on cpu" % cls.__name__):
        agent.engine()
    monkeypatch.setattr(dist, "collectives_active", lambda: True)
    with pytest.raises(_C.TrlError, match="%s runs on one rank" % cls.__name__):
        agent.engine()                                                    # ... a process group that came up later
    with pytest.raises(_C.TrlError, match="runs on one rank"):
        _agent(cls, _nets(twin=twin))


def test_loss_kernel_argument_checks_launch_nothing():
    """B <= 0, a NULL required pointer and q2 without q2n come back as a negative code with a message; no pointer is
    touched (the ones passed here are not device memory)."""
    from torchrl_amd import _C
    lib = _C.lib()
    p = 4096                                                              # a non-NULL pointer nobody dereferences

    def call(B=8, n=8, q1=p, q2=p, q2n=p, dq2=p, dq2n=p, sums=p, alpha=p):
        return lib.trl_sacv_losses_f32(q1, q2, p, p, p, p, p, q2n, p, alpha, 0.99, B, n, p, dq2, p, p, dq2n, sums, None, None,
                                       0.0, 0.0, 0.9, 0.999, 1e-8, None, 0, None, None)
    for kw, text in ((dict(B=0), "empty batch"), (dict(B=-3), "empty batch"), (dict(n=4), "global batch"),
                     (dict(q1=None), "null input"), (dict(sums=None), "null output"),
                     (dict(q2n=None), "q2 and q2n come together"), (dict(q2=None), "q2 and q2n come together"),
                     (dict(dq2=None), "dq2 / dq2n go with q2 / q2n"), (dict(alpha=None), "alpha")):
        assert call(**kw) < 0, kw
        assert text in lib.trl_last_error().decode(), (kw, lib.trl_last_error().decode())
    assert lib.trl_sacv_samples_f32(None, p, None, 0, p, p, p, p, p, p, 8, 17, 6, 1, None, None) < 0
    assert "null input" in lib.trl_last_error().decode()
    assert lib.trl_sacv_samples_f32(p, p, None, 0, p, p, p, p, p, p, 8, 17, 9, 1, None, None) < 0
    assert "A <= 8" in lib.trl_last_error().decode()
