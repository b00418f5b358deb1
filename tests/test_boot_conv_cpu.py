"""Bootstrapped DQN over conv trunks (TRL_BOOT_CONV=1) without a GPU: the float64 restatement of the update against the
fixture (tests/golden/boot_dqn_conv_update.npz, written from the unmodified reference classes), state-dict names and
order, what the switch opens and what stays refused, and the float32 run of the restatement of trl_boot_head_dx_f32, which
yields the bound constant the GPU kernel test uses (tests/_boot_conv_ref.py)."""
import functools
import json

import numpy as np
import pytest
import torch

import _boot_conv_ref as R
import _optim_ref

F32, F64 = R.F32, R.F64
A, K = 3, 3
SHAPE = (4, 44, 44)
CONVS = [[8, [8, 8], [4, 4], [0, 0]], [8, [4, 4], [2, 2], [0, 0]], [16, [3, 3], [1, 1], [0, 0]]]


@pytest.fixture(scope="module")
def g():
    return R.load_fixture()


@pytest.fixture
def on(monkeypatch):
    monkeypatch.setenv("TRL_BOOT_CONV", "1")


def make_net(append, seed=None, **kw):
    from torchrl import networks
    if seed is not None:
        torch.manual_seed(seed)
    args = dict(output_shape=A, head_num=K, append_hidden_shapes=append, activation_func=torch.nn.ReLU,
                base_type=functools.partial(networks.CNNBase, input_shape=SHAPE, hidden_shapes=CONVS))
    args.update(kw)
    return networks.BootstrappedNet(**args)


def make_algo(qf, **kw):
    from torchrl.algo import BootstrappedDQN
    from torchrl.policies import BootstrappedDQNDiscretePolicy
    import gym

    class Env:
        action_space = gym.spaces.Discrete(A)

    class Stub:
        epoch_frames = 0
    pf = BootstrappedDQNDiscretePolicy(qf=qf, head_num=K, action_shape=A)
    args = dict(head_num=K, bernoulli_p=0.5, qf=qf, pf=pf, qlr=1e-3, env=Env(), replay_buffer=None, collector=Stub(),
                logger=None, batch_size=4, device="cpu", save_dir=None)
    args.update(kw)
    return BootstrappedDQN(**args), pf


# ------------------------------------------------------------------ the restatement against the fixture
@pytest.mark.parametrize("tag", R.CASES)
def test_restatement_matches_the_reference_update(g, tag):
    up, a = R.update_from_fixture(g, tag)
    assert a["K"] == K and a["steps"] == 2
    q0 = R.q_all(up.net, R.frames_to_float(g["batch_s0_obs"]))[0]
    np.testing.assert_allclose(q0, g[tag + "_q0"], rtol=1e-5, atol=1e-7)
    names = [k[len(tag + "_qf0_"):] for k in g if k.startswith(tag + "_qf0_")]
    for s in range(a["steps"]):
        info = up.update(R.batch_of(g, s))
        want = dict(zip([str(k) for k in g[f"{tag}_s{s}_info_keys"]], g[f"{tag}_s{s}_info_vals"]))
        assert sorted(info) == sorted(want) == ["Reward_Mean", "Training/qf_loss"]
        for k in want:
            assert info[k] == pytest.approx(want[k], rel=1e-4, abs=1e-5), k
        for mine, name in ((up.params, "qf%d" % (s + 1)), (up.tparams, "tqf%d" % (s + 1))):
            for x, y in zip(mine, R.params_of(R.net_of(g, f"{tag}_{name}_", K))):
                assert np.abs(x - y).max() < 1e-6
        for sn, arrays in up.state().items():                            # the optimiser's state under torch's names
            for x, pn in zip(arrays, names):
                want_s = g[f"{tag}_state{s + 1}_{sn}_{pn}"]
                assert np.abs(x - want_s).max() <= 1e-6 * max(1.0, float(np.abs(want_s).max()) / float(np.abs(g[f"{tag}_qf0_{pn}"]).max()))
        stored = {sn for sn in ("exp_avg", "exp_avg_sq", "square_avg", "momentum_buffer", "grad_avg")
                  if any(k.startswith(f"{tag}_state{s + 1}_{sn}_base") for k in g)}
        assert stored == set(up.state())
    if tag == "rms":                                                     # period 2: the target IS the online net after update 2
        assert a["opt"] == ("rmsprop", 0.95, 0.01) and not a["soft"] and a["period"] == 2
        for pn in names:
            assert np.array_equal(g["rms_tqf2_" + pn], g["rms_qf2_" + pn]), pn
            assert np.array_equal(g["rms_tqf1_" + pn], g["rms_qf0_" + pn]), pn     # ... and untouched after update 1


def test_restated_actions_match_the_reference_policy(g):
    """`explore` under head k and `eval_act` on the first batch's frame stacks are the restated arg-max under a head and of
    the ensemble vote, and no top-two gap is small enough for a float32 Q network to flip (the GPU test asks for equality)."""
    import _boot_dqn_ref as RB
    for tag in R.CASES:
        q = R.q_all(R.net_of(g, tag + "_qf0_", K), R.frames_to_float(g["batch_s0_obs"]))[0]
        for k in range(K):
            assert np.array_equal(RB.boot_act_ref(q, np.full(q.shape[1], k))[0], g[tag + "_explore"][k])
        assert np.array_equal(RB.boot_act_ref(q, None)[0], g[tag + "_eval"].reshape(-1))
        top = np.sort(np.concatenate([q, q.mean(0)[None]]), axis=2)
        assert (top[..., -1] - top[..., -2]).min() > 4e-6


def test_conv_chain_rule_equals_autograd():
    """The numpy conv forward / backward of the restatement against torch's conv2d + autograd in float64."""
    rs = np.random.RandomState(4)
    convs = [(rs.randn(5, 4, 8, 8) * 0.1, rs.randn(5) * 0.1, (4, 4)), (rs.randn(6, 5, 4, 4) * 0.1, rs.randn(6) * 0.1, (2, 2)),
             (rs.randn(7, 6, 3, 3) * 0.1, rs.randn(7) * 0.1, (1, 1))]
    x = rs.randn(3, 4, 44, 44)
    feat, tape = R.conv_forward(convs, x)
    d_feat = rs.randn(*feat.shape)
    grads = R.conv_backward(convs, tape, d_feat)
    ws = [(torch.tensor(w, requires_grad=True), torch.tensor(b, requires_grad=True)) for w, b, _ in convs]
    h = torch.tensor(x)
    for (w, b), (_, _, s) in zip(ws, convs):
        h = torch.relu(torch.nn.functional.conv2d(h, w, b, stride=s))
    np.testing.assert_allclose(h.flatten(1).detach().numpy(), feat, rtol=1e-12, atol=1e-14)
    (h.flatten(1) * torch.tensor(d_feat)).sum().backward()
    for (w, b), gw, gb in zip(ws, grads[0::2], grads[1::2]):
        np.testing.assert_allclose(w.grad.numpy(), gw, rtol=1e-10, atol=1e-13)
        np.testing.assert_allclose(b.grad.numpy(), gb, rtol=1e-10, atol=1e-13)


# ------------------------------------------------------------------ the switch
def test_nothing_constructs_with_the_switch_unset(monkeypatch):
    from torchrl_amd import _C, ops
    monkeypatch.delenv("TRL_BOOT_CONV", raising=False)
    assert not ops.boot_conv()
    with pytest.raises(_C.TrlError):
        make_net([])


@pytest.mark.parametrize("tag", R.CASES)
def test_net_policy_and_algo_construct_on_the_cpu(g, tag, on):
    """Seeded construction equals the reference's; state-dict names and ORDER are the fixture's; the eager CPU forward is the
    reference's; the algorithm takes RMSprop and the policy frame batches (both refuse only for want of a GPU)."""
    from torchrl_amd import _C, ops
    assert ops.boot_conv()
    a = R.case_args(g, tag)
    seed = int(json.loads(str(g["meta"]))["init_seed"])
    qf = make_net(a["append"], seed)
    prefix = tag + "_qf0_"
    assert [k.replace(".", "__") for k in qf.state_dict()] == [k[len(prefix):] for k in g if k.startswith(prefix)]
    assert list(qf.state_dict())[:2] == ["base.seq_convs.0.weight", "base.seq_convs.0.bias"]
    assert [k for k in qf.state_dict() if k.startswith("head")][0] == "head0.0.weight"
    for k, v in qf.state_dict().items():
        assert np.array_equal(v.numpy(), g[prefix + k.replace(".", "__")]), k
    plist = qf.param_list()
    assert [tuple(p.shape) for p in plist[:6]] == [(8, 4, 8, 8), (8,), (8, 8, 4, 4), (8,), (16, 8, 3, 3), (16,)]
    assert all(p is q for p, q in zip(plist, qf.parameters())) and len(plist) == len(list(qf.parameters()))
    assert len(qf.trunk_layers()) == 3 and len(qf.head_layers(0)) == len(a["append"]) + 1 and qf.is_conv
    frames = torch.from_numpy(R.frames_to_float(g["batch_s0_obs"]).astype(F32))
    with torch.no_grad():
        out = qf(frames, range(K))
    for k in range(K):
        np.testing.assert_allclose(out[k].numpy(), g[tag + "_q0"][k], rtol=1e-5, atol=1e-6)
    cls = torch.optim.Adam if a["opt"][0] == "adam" else torch.optim.RMSprop
    info = {} if a["opt"][0] == "adam" else dict(alpha=a["opt"][1], eps=a["opt"][2])
    algo, pf = make_algo(qf, optimizer_class=cls, optimizer_info=info)
    assert type(algo.qf_optimizer) is cls and algo.target_qf.is_conv
    with pytest.raises(_C.TrlError, match="needs a GPU"):
        algo.update({})
    with pytest.raises(_C.TrlError, match="needs a GPU"):
        pf.explore(torch.zeros((2,) + SHAPE, dtype=torch.uint8))
    assert tuple(pf._rows(torch.zeros((1, 2) + SHAPE)).shape) == (2,) + SHAPE


def test_mlp_trunks_take_rmsprop_and_sgd_under_the_switch(on):
    from torchrl import networks
    from torchrl_amd import _C
    for cls in (torch.optim.RMSprop, torch.optim.SGD):
        qf = networks.BootstrappedNet(output_shape=A, head_num=K, base_type=networks.MLPBase, input_shape=5, hidden_shapes=[8])
        algo, _ = make_algo(qf, optimizer_class=cls)
        with pytest.raises(_C.TrlError, match="needs a GPU"):            # (not "Adam only")
            algo.update({})


def test_refusals_that_stay_under_the_switch(on):
    from torchrl import networks
    from torchrl_amd import _C
    with pytest.raises(_C.TrlError, match="add_ln"):
        make_net([], add_ln=True)
    padded = [[8, [8, 8], [4, 4], [1, 1]]]
    with pytest.raises(_C.TrlError, match="padding 0"):
        make_net([], base_type=functools.partial(networks.CNNBase, input_shape=SHAPE, hidden_shapes=padded))
    with pytest.raises(_C.TrlError, match="differs from the heads'"):
        make_net([], base_type=functools.partial(networks.CNNBase, input_shape=SHAPE, hidden_shapes=CONVS,
                                                 last_activation_func=torch.nn.Tanh))
    with pytest.raises(_C.TrlError, match="1..64 heads"):
        make_net([], head_num=65)


# ------------------------------------------------------------------ trl_boot_head_dx_f32: the float32 run and its constant
def test_float32_head_dx_yields_the_bound_constant():
    """The largest err / (U sum|terms|) of the float32 numpy run over every case of the GPU kernel test, times the margin,
    rounded up to a power of two, is covered by the constant the GPU test uses; masked-out elements are exact zeros."""
    worst, plain = 0.0, 0.0
    for (K_, B, C, P, H1) in R.head_shapes():
        for act in (R.ACT_RELU, R.ACT_TANH):
            c = R.head_case(K_, B, C, P, H1, act)
            ref, got = R.head_dx_ref(c), R.head_dx_ref(c, F32)
            assert got["out"].dtype == F32 and got["out"].shape == (B, P, C)
            worst = max(worst, R.head_dx_ratio(got["out"], ref))
            if act == R.ACT_TANH:
                plain = max(plain, R.head_dx_plain_ratio(got["out"], ref))
            if B > 3:
                assert np.all(got["out"][3::4] == 0.0) and np.all(ref["mag"][3::4] == 0.0)      # masked in every head
            assert (ref["mag"] > 0).any()
    print("float32 head_dx: worst err / (U sum|terms|) = %.3f" % worst)
    print("float32 head_dx, Tanh cells under the plain |act'| sum|terms| (information only): %.1f" % plain)
    assert worst > 0.0
    assert R.MARGIN * worst <= R.K_HEAD_DX == _optim_ref.pow2_at_least(R.K_HEAD_DX), worst       # it still covers


def test_head_dx_restatement_is_the_three_step_composition():
    """Against the explicit (K, B, F) stack, its fold and the gated transpose, in float64."""
    c = R.head_case(3, 5, 16, 4, 32, R.ACT_TANH)
    K_, B, C, P = 3, 5, 16, 4
    dz = c["dz"].astype(F64) * R.dact(R.ACT_TANH, c["gates"].astype(F64))
    stack = np.stack([dz[k] @ c["w"][k].astype(F64) for k in range(K_)])
    folded = stack.sum(0).reshape(B, C, P)
    want = (folded * R.dact(R.ACT_TANH, c["y_top"].astype(F64))).transpose(0, 2, 1)
    np.testing.assert_allclose(R.head_dx_ref(c)["out"], want, rtol=1e-13, atol=1e-15)
