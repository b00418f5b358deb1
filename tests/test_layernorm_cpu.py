"""LayerNorm MLPs (`add_ln=True`), CPU half: the numpy restatement (tests/_layernorm_ref.py) against the reference fixture
(tests/golden/layernorm_update.npz), the structure of the repo's own module lists, and the statistics case that tells a
two-pass variance from E[x^2] - mean^2.  The GPU half (tests/test_layernorm_gpu.py) compares the kernels and the engine with
the same restatement and fixture."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _layernorm_ref as ref                                                  # noqa: E402

SCALAR_REL, SCALAR_ABS, PARAM_ABS = 1e-4, 1e-5, 1e-6


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(HERE, "golden", "layernorm_update.npz"))


def close(got, want):
    return np.abs(np.asarray(got, dtype=np.float64) - want) <= SCALAR_ABS + SCALAR_REL * np.abs(want)


def policy_outputs(g, tag, dtype):
    """{name: (restated, fixture)} of the policy's update / eval_act outputs and the value net's forward."""
    kind = ref.STRUCT[tag][0]
    tanh = bool(int(g[tag + "_args"][3]))
    b = ref.batch_of(g, tag)
    obs, acts = b["obs"].astype(dtype), b["acts"].astype(dtype)
    pf, vf = ref.net_from(g, tag + "_pf0_", tag, dtype), ref.net_from(g, tag + "_vf0_", tag, dtype)
    head = pf.forward(obs)[0]
    logstd = g[tag + "_pf0_logstd"].astype(dtype) if kind == "bb" else None
    lp, ent = ref.policy_logp(kind, head, logstd, acts, tanh)
    out = {"v0": (vf.forward(obs)[0], g[tag + "_v0"])}
    if kind == "cat":
        out["log_prob"] = (lp, g[tag + "_upd_log_prob"].reshape(-1))
        out["ent"] = (ent, g[tag + "_upd_ent"].reshape(-1))
        out["probs"] = (ref.cat_terms(head, acts)[1], g[tag + "_probs"])
        assert np.array_equal(head.argmax(axis=1), g[tag + "_eval_act"].reshape(-1))
        return out
    A = head.shape[1] // 2 if kind == "sd" else head.shape[1]
    mean = head[:, :A]
    out["mean"] = (mean, g[tag + "_upd_mean"])
    out["log_prob"] = (lp, g[tag + "_upd_log_prob"].reshape(-1))
    out["ent"] = (ent, g[tag + "_upd_ent"].reshape(-1))
    out["eval_act"] = (np.tanh(mean) if tanh else mean, g[tag + "_eval_act"])
    if kind == "sd":
        out["log_std"] = (np.clip(head[:, A:], -20.0, 2.0), g[tag + "_upd_log_std"])
    else:
        out["log_std"] = (logstd, g[tag + "_upd_log_std"])
    return out


def run_updates(g, tag, dtype):
    """{update name: worst parameter error against the fixture} of the A2C update and the four chained PPO updates."""
    errs = {}
    b = ref.batch_of(g, tag)
    u = ref.Update(g, tag, dtype, tag + "_pf0_", tag + "_vf0_", plr=3e-4, vlr=1e-3, c_ent=0.01)
    u.update(b, ref.LOSS_A2C)
    errs["a2c_pf"] = ref.param_errors(u.pf, u.logstd, g, tag + "_a2c_pf1_", tag)
    errs["a2c_vf"] = ref.param_errors(u.vf, None, g, tag + "_a2c_vf1_", tag)
    u = ref.Update(g, tag, dtype, tag + "_pf0_", tag + "_vf0_", plr=3e-4, vlr=3e-4, c_ent=0.005,
                   target_prefix=tag + "_ppo_tpf0_")
    for s, clipv in enumerate(g[tag + "_ppo_clipv"]):
        u.update(b, ref.LOSS_PPO_CLIP, bool(clipv))
        errs["ppo%d_pf" % s] = ref.param_errors(u.pf, u.logstd, g, "%s_ppo_pf%d_" % (tag, s + 1), tag)
        errs["ppo%d_vf" % s] = ref.param_errors(u.vf, None, g, "%s_ppo_vf%d_" % (tag, s + 1), tag)
    return errs


@pytest.mark.parametrize("tag", ref.TAGS)
def test_restatement_policy_outputs_match_the_fixture(g, tag):
    """float64: rel 1e-4 / abs 1e-5 on every output; the float32 restatement's worst errors are printed (and recorded in
    profiles/NOTES_layernorm.md)."""
    for name, (got, want) in policy_outputs(g, tag, np.float64).items():
        assert close(got, want).all(), (tag, name, np.abs(got - want).max())
    for name, (got, want) in policy_outputs(g, tag, np.float32).items():
        err = np.abs(got.astype(np.float64) - want)
        print("%s float32 %s: max abs err %.3e, worst err / bound %.3f"
              % (tag, name, err.max(), (err / (SCALAR_ABS + SCALAR_REL * np.abs(want))).max()))
        assert close(got, want).all(), (tag, name)


@pytest.mark.parametrize("tag", ref.TAGS)
def test_restatement_updates_match_the_fixture(g, tag):
    """Post-step parameters of the A2C update and of the four chained PPO updates (the third with the clipped value loss;
    `update` itself applies no learning-rate schedule): abs 1e-6 in float64.  The float32
    restatement has to be comfortably inside the same bound (a case that is not gets another seed, not another bound)."""
    e64, e32 = run_updates(g, tag, np.float64), run_updates(g, tag, np.float32)
    for k in e64:
        print("%s %s: float64 %.3e float32 %.3e" % (tag, k, e64[k], e32[k]))
    assert all(v <= PARAM_ABS for v in e64.values()), e64
    assert all(v <= 0.5 * PARAM_ABS for v in e32.values()), e32


def test_updates_move_every_layernorm_parameter(g):
    for tag in ref.TAGS:
        names = _ln_names(tag)
        assert len(names) == 2 * (1 + len(ref.STRUCT[tag][3]))
        for name in names:
            for net in ("pf", "vf"):
                k0 = "%s_%s0_%s" % (tag, net, name.replace(".", "__"))
                assert not np.array_equal(g[k0], g[k0.replace("%s0_" % net, "ppo_%s4_" % net)]), k0
                assert g[k0].std() > 0.05                                     # neither gamma == 1 nor beta == 0


def _ln_names(tag):
    _, _, hidden, append = ref.STRUCT[tag]
    out = []
    for seq, i, post in ref.structure(hidden, append):
        if post == "ln":
            out += ["%s.%d.weight" % (seq, i + 2), "%s.%d.bias" % (seq, i + 2)]
    return out


# ---------------------------------------------------------------- structure, from the repo's own modules
def repo_net(tag, D=7, out=3):
    from torchrl_amd import networks
    _, act, hidden, append = ref.STRUCT[tag]
    return networks.Net(input_shape=(D,), output_shape=out, base_type=networks.MLPBase, hidden_shapes=list(hidden),
                        append_hidden_shapes=list(append), activation_func={"tanh": torch.nn.Tanh, "relu": torch.nn.ReLU}[act],
                        add_ln=True)


@pytest.mark.parametrize("tag", ref.TAGS)
def test_module_lists_and_plan_have_the_reference_structure(g, tag):
    """One LayerNorm for [H1, H2], the last hidden layer activated twice, and with an appended layer a LayerNorm whose
    output feeds the head; state_dict keys as in the fixture; ops.net_plan reads exactly that off the module lists."""
    from torchrl_amd import ops, _C
    _, act, hidden, append = ref.STRUCT[tag]
    net = repo_net(tag)
    A = torch.nn.Tanh if act == "tanh" else torch.nn.ReLU
    trunk = list(net.base.seq_fcs)
    assert sum(isinstance(m, torch.nn.LayerNorm) for m in trunk) == len(hidden) - 1 == 1
    assert [type(m) for m in trunk] == [torch.nn.Linear, A, torch.nn.LayerNorm, torch.nn.Linear, A, A]
    tail = list(net.seq_append_fcs)
    assert [type(m) for m in tail] == [torch.nn.Linear, A, torch.nn.LayerNorm] * len(append) + [torch.nn.Linear]
    vf_keys = sorted(k[len(tag + "_vf0_"):].replace("__", ".") for k in g.files if k.startswith(tag + "_vf0_"))
    assert sorted(net.state_dict()) == vf_keys
    assert sorted(ref.param_names(tag)) == vf_keys
    plan = ops.net_plan(net)
    posts = [None if p is None else p[0] for _, _, p in plan]
    assert posts == [p for _, _, p in ref.structure(hidden, append)]
    assert posts[:2] == ["ln", "act"] and posts[-1] is None and (not append or posts[-2] == "ln")
    assert plan[0][2][1] is trunk[2].weight and plan[0][2][2] is trunk[2].bias
    layers, code = ops.net_layers(net)
    assert ops.has_post(layers) and code == ops.ACT_OF[A]
    assert [tuple(p.shape) for p in ops.plan_params(layers)] == [tuple(p.shape) for p in net.parameters()]
    assert net.mlp2_spec() is None
    with pytest.raises(_C.TrlError, match="LayerNorm"):                    # the engines that do not carry the norms keep refusing
        ops.act_code(net)


def test_plan_of_a_plain_net_and_the_width_limit():
    from torchrl_amd import networks, ops, _C
    kw = dict(input_shape=(5,), output_shape=2, base_type=networks.MLPBase, append_hidden_shapes=[], activation_func=torch.nn.Tanh)
    plain = networks.Net(hidden_shapes=[8, 8], **kw)
    assert [p for _, _, p in ops.net_plan(plain)] == [None, None, None]
    layers, code = ops.net_layers(plain)
    assert all(len(l) == 2 for l in layers) and code == _C.ACT_TANH
    wide = networks.Net(hidden_shapes=[1025, 8], add_ln=True, **kw)
    with pytest.raises(_C.TrlError, match="1024"):
        ops.net_plan(wide)
    one = ops.net_plan(networks.Net(hidden_shapes=[8], add_ln=True, **kw))   # its only norm is popped: Linear, act, act
    assert [p for _, _, p in one] == [("act",), None]


# ---------------------------------------------------------------- the restated backward against autograd
@pytest.mark.parametrize("tag", ref.TAGS)
def test_restated_backward_is_autograd_in_float64(g, tag):
    _, act, hidden, append = ref.STRUCT[tag]
    net = repo_net(tag).double()
    rs = np.random.RandomState(3)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.copy_(torch.from_numpy(1 + 0.3 * rs.randn(*m.weight.shape)))
                m.bias.copy_(torch.from_numpy(0.2 * rs.randn(*m.bias.shape)))
    x, d_out = rs.randn(13, 7), rs.randn(13, 3)
    out = net(torch.from_numpy(x))
    out.backward(torch.from_numpy(d_out))
    sd = {k.replace(".", "__"): v.detach().numpy() for k, v in net.state_dict().items()}
    mine = ref.net_from(sd, "", tag, np.float64)
    y, tape = mine.forward(x)
    np.testing.assert_allclose(y, out.detach().numpy(), rtol=1e-12, atol=1e-13)
    want = dict(net.named_parameters())
    for name, got in zip(ref.param_names(tag), mine.backward(tape, d_out)):
        np.testing.assert_allclose(got, want[name].grad.numpy(), rtol=1e-10, atol=1e-12, err_msg=name)


# ---------------------------------------------------------------- statistics far from zero
def stats_case():
    """Rows of mean 100 and std 0.5, H = 64 (also used by the GPU test): float32 values, so float64 sees the same rows."""
    rs = np.random.RandomState(77)
    a = (100.0 + 0.5 * rs.randn(256, 64)).astype(np.float32)
    gamma = (1.0 + 0.3 * rs.randn(64)).astype(np.float32)
    beta = (0.2 * rs.randn(64)).astype(np.float32)
    return a, gamma, beta


def stats_case_bound():
    """4 x the float32 two-pass restatement's worst error against float64 on y (another summation order is allowed for)."""
    a, gamma, beta = stats_case()
    y64 = ref.ln_fwd(a.astype(np.float64), gamma.astype(np.float64), beta.astype(np.float64))[0]
    y32 = ref.ln_fwd(a, gamma, beta)[0]
    return 4.0 * float(np.abs(y32.astype(np.float64) - y64).max()), y64


def test_two_pass_statistics_hold_where_one_pass_fails():
    a, gamma, beta = stats_case()
    bound, y64 = stats_case_bound()
    one = ref.ln_fwd(a, gamma, beta, stats=ref.ln_stats_one_pass)[0]
    err_one = float(np.abs(one.astype(np.float64) - y64).max())
    print("statistics case: bound (4 x float32 two-pass error) %.3e, float32 one-pass error %.3e" % (bound, err_one))
    assert bound > 0.0
    assert err_one > bound
    # H = 1: xhat = 0, y = beta, da = 0
    a1 = np.array([[3.0], [-2.0]])
    y, mean, rstd = ref.ln_fwd(a1, np.array([1.7]), np.array([0.4]))
    assert np.array_equal(y, np.full((2, 1), 0.4))
    dz, dg, db = ref.ln_bwd(np.ones((2, 1)), a1, mean, rstd, np.array([1.7]), "none")
    assert np.array_equal(dz, np.zeros((2, 1))) and dg[0] == 0.0 and db[0] == 2.0
