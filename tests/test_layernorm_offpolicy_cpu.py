"""`add_ln=True` networks on the off-policy engines, the part that needs no GPU: the fixture
tests/golden/layernorm_offpolicy*.npz (the reference's own float32-vs-float64 distance stays within a quarter of the bounds
its consumers use; keys and shapes as documented in tests/_layernorm_offpolicy.py), the layer plans and parameter order the
engines home (`ops.net_layers` / `ops.plan_params`, `_engine.net_home`), and that every gradient view -- dgamma / dbeta
included -- lies inside the flat gradient buffer the ranks exchange."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _layernorm_offpolicy as lo                                             # noqa: E402
import _layernorm_ref as ref                                                  # noqa: E402


@pytest.fixture(scope="module")
def fx():
    return lo.load_fixture()


@pytest.fixture(autouse=True)
def offpolicy_layernorm_on(monkeypatch):
    """The off-policy engines carry `add_ln` nets under TRL_OFFPOLICY_LN=1 only (unset: their refusal, as before)."""
    monkeypatch.setenv("TRL_OFFPOLICY_LN", "1")


def test_fixture_files_stay_below_the_size_limit():
    for part in lo.PARTS:
        assert os.path.getsize(os.path.join(HERE, "golden", lo.NAME + part + ".npz")) < 1 << 20


def test_reference_float32_is_within_a_quarter_of_the_bounds(fx):
    """meta["distance"]: per case the largest distance between the reference's float32 run and its float64 run on the
    same stored inputs, over all four updates, as a fraction of the bound (parameters abs 1e-6, info rel 1e-4 / abs 1e-5)."""
    g, meta = fx
    assert [str(t) for t in g["cases"]] == lo.TAGS and sorted(meta["distance"]) == sorted(lo.TAGS)
    b = meta["bounds"]
    assert (b["params_abs"], b["info_rel"], b["info_abs"], b["keep_fraction"]) == (lo.PARAM_BOUND, lo.INFO_REL, lo.INFO_ABS, 0.25)
    for tag, d in meta["distance"].items():
        print("%-15s seed %5d parameters %.3f info %.3f of the bound" % (tag, d["seed"], d["params"], d["info"]))
        assert 0 < d["params"] <= 0.25 and 0 <= d["info"] <= 0.25, (tag, d)
        assert d["seed"] == lo.args_of(g, tag)["seed"]
    for tag, seeds in meta["rejected"].items():
        assert all(max(v["params"], v["info"]) > 0.25 for v in seeds.values()), tag


@pytest.mark.parametrize("tag", lo.TAGS)
def test_fixture_keys_and_shapes(fx, tag):
    """Every documented key is there with its shape; the state dicts are those of the repo's networks of the case (torch's
    names, gamma / beta included), for trained networks and targets, before and after each of the four updates; every
    LayerNorm parameter and every target moves with every update of its network."""
    g, _ = fx
    a = lo.args_of(g, tag)
    B, D, A = a["B"], a["D"], a["A"]
    assert a["steps"] == 4
    batch = lo.batch_of(g, tag)
    assert batch["obs"].shape == batch["next_obs"].shape == (B, D) and batch["rewards"].shape == batch["terminals"].shape == (B, 1)
    assert batch["acts"].shape == {"DQN": (B, 1), "QRDQN": (B,)}.get(a["algo"], (B, A))
    nets = lo.build_nets(a)
    assert list(nets) == a["nets"]
    target_of = {"tqf1": "qf1", "tqf2": "qf2", "tqf": "qf", "tvf": "vf", "tpf": "pf"}
    used = {tag + "_args"} | {f"{tag}_batch_{k}" for k in lo.BATCH_KEYS}
    for s in range(4):
        for k in a["noise"]:
            assert g[f"{tag}_s{s}_{k}"].shape == (B, A) and g[f"{tag}_s{s}_{k}"].dtype == np.float32
            used.add(f"{tag}_s{s}_{k}")
        info = lo.info_of(g, tag, s)
        assert info and all(np.isfinite(v) for v in info.values())
        used |= {f"{tag}_info{s}_keys", f"{tag}_info{s}_vals"}
        if a["algo"] in ("TwinSACQ", "SAC", "TwinSAC"):
            assert g[f"{tag}_log_alpha{s + 1}"].shape == (1,)
            used.add(f"{tag}_log_alpha{s + 1}")
    for name in a["nets"] + a["targets"]:
        mod = nets[target_of.get(name, name)]
        n_ln = sum(isinstance(m, torch.nn.LayerNorm) for m in mod.modules())
        want_ln = (a["pf_ln"] if target_of.get(name, name) == "pf" else a["q_ln"]) * (len(a["hidden"]) - 1 + len(a["append"]))
        assert n_ln == want_ln
        ln_keys = [n + "." + k for n, m in mod.named_modules() if isinstance(m, torch.nn.LayerNorm) for k in ("weight", "bias")]
        for i in range(5):
            sd = lo.state_of(g, f"{tag}_{name}{i}_")
            assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in mod.state_dict().items()}
            assert all(v.dtype == torch.float32 for v in sd.values())
            used |= {f"{tag}_{name}{i}_{k.replace('.', '__')}" for k in sd}
        # TD3 (policy_update_delay 2): the policy steps at updates 0 and 2 only, and every target moves with it (td3.py:124-148)
        lags = a["algo"] == "TD3" and (name == "pf" or name in a["targets"])
        steps = [0, 2] if lags else [0, 1, 2, 3]
        if lags:
            assert all(torch.equal(v, lo.state_of(g, f"{tag}_{name}2_")[k]) for k, v in lo.state_of(g, f"{tag}_{name}1_").items())
        for s in steps:
            before, after = lo.state_of(g, f"{tag}_{name}{s}_"), lo.state_of(g, f"{tag}_{name}{s + 1}_")
            moved = ln_keys or list(before)[:1]
            assert all(not torch.equal(before[k], after[k]) for k in moved), (name, s)
    assert used == {k for k in g if k.startswith(tag + "_")}


@pytest.mark.parametrize("tag", lo.TAGS)
def test_plans_and_parameter_order_of_the_fixture_structures(fx, tag):
    """`ops.net_layers` of every network of a case: post-ops where the reference's module list has them (a LayerNorm behind
    every hidden layer but the trunk's last, which is activated twice; behind every appended layer), the head bare; a
    plain net keeps its (W, b) list; `ops.plan_params` is W, b, gamma, beta per layer == `parameters()` order == the order
    of the state dict's keys."""
    from torchrl_amd import ops
    g, _ = fx
    a = lo.args_of(g, tag)
    want = [post for _, _, post in ref.structure(a["hidden"], a["append"])]
    for name, mod in lo.build_nets(a).items():
        layers, code = ops.net_layers(mod)
        assert code == ops.ACT_OF[getattr(torch.nn, a["act"])]
        ln = a["pf_ln"] if name == "pf" else a["q_ln"]
        if not ln:
            assert all(len(l) == 2 for l in layers) and not ops.has_post(layers)
        else:
            assert [None if l[2] is None else l[2][0] for l in layers] == want
            assert ops.has_post(layers)
        params = ops.plan_params(layers)
        assert [id(p) for p in params] == [id(p) for p in mod.parameters()]
        assert [tuple(p.shape) for p in params] == [tuple(v.shape) for v in mod.state_dict().values()]


def _home(tag, g, mismatch=None):
    from torchrl_amd.algo.off_policy._engine import net_home
    a = lo.args_of(g, tag)
    nets = lo.build_nets(a)
    if mismatch:
        nets[mismatch] = lo.build_nets(a, pf_ln=not a["pf_ln"], q_ln=not a["q_ln"])[mismatch]
    trained = [(n, nets[n]) for n in a["nets"]]
    source = {"tqf1": "qf1", "tqf2": "qf2", "tqf": "qf", "tvf": "vf", "tpf": "pf"}
    targets = [("target_" + source[t], copy.deepcopy(nets[source[t]])) for t in a["targets"]]
    opts = [torch.optim.Adam(m.parameters(), lr=1e-3) for _, m in trained]
    twins = tuple(n for n in a["nets"] if n in ("qf1", "qf2"))
    return nets, targets, net_home(trained, targets, opts, same=(twins,) if len(twins) == 2 else ())


@pytest.mark.parametrize("tag", lo.TAGS)
def test_every_gradient_view_lies_inside_the_flat_gradient_buffer(fx, tag):
    """The home every off-policy engine builds (`_engine.net_home`, here on CPU modules): the parameters are views of `flat`
    in W, b, gamma, beta order, the targets of `tflat` in the same order, and `layer_views` cuts `grads` into one tuple per
    layer -- (dW, db) or (dW, db, dgamma, dbeta) -- that tile it without gaps: what several ranks exchange (the flat
    gradient buffer) carries the norms' gradients with nothing new, and dbeta starts where dgamma ends, which is what lets
    a fold plan take [dgamma | dbeta] as one entry."""
    from torchrl_amd import ops
    g, _ = fx
    nets, targets, (layers, tlayers, act, home) = _home(tag, g)
    views = home.layer_views(layers)
    lo_, pos = home.grads.data_ptr(), 0
    for ls, vs, size in zip(layers, views, home.sizes):
        start = pos
        for l, v in zip(ls, vs):
            ps = ops.plan_params([l])
            assert len(v) == len(ps) == (4 if len(l) > 2 and l[2] is not None and l[2][0] == "ln" else 2)
            for p, t in zip(ps, v):
                assert t.shape == p.shape and t.data_ptr() == lo_ + 4 * pos       # inside `grads`, in order, no gap
                assert p.data_ptr() == home.flat.data_ptr() + 4 * pos             # the parameter: the same place of `flat`
                pos += t.numel()
            if len(v) == 4:
                assert v[3].data_ptr() == v[2].data_ptr() + 4 * v[2].numel()
        assert pos - start == size
    assert pos == home.grads.numel() == home.flat.numel()
    tpos = 0
    for ls in tlayers:
        for p in ops.plan_params(ls):
            assert p.data_ptr() == home.tflat.data_ptr() + 4 * tpos
            tpos += p.numel()
    assert tpos == home.tflat.numel() == sum(home.sizes[len(layers) - len(tlayers):])
    # state_dict() keeps torch's names and reads the flat buffer
    for name, mod in nets.items():
        assert list(mod.state_dict()) == [k for k, _ in mod.named_parameters()]
    with torch.no_grad():
        home.flat.fill_(0.25)
    assert all(bool((v == 0.25).all()) for mod in nets.values() for v in mod.state_dict().values())


def test_mismatched_networks_are_refused_by_name(fx):
    """Twin critics run as one grouped launch per layer: LayerNorm on one of them only is refused with both names; so is a
    target that does not have its network's structure.  The policy may differ from the critics (critic_only_ln)."""
    from torchrl_amd import _C
    from torchrl_amd.algo.off_policy._engine import net_home
    g, _ = fx
    for tag in ("sacq_relu", "twinsacv", "td3_relu_app"):
        with pytest.raises(_C.TrlError, match="qf1 and qf2 .*add_ln"):
            _home(tag, g, mismatch="qf2")
    _home("critic_only_ln", g)
    a = lo.args_of(g, "dqn_relu")
    qf, plain = lo.build_nets(a)["qf"], lo.build_nets(a, q_ln=False)["qf"]
    with pytest.raises(_C.TrlError, match="qf and its target target_qf differ"):
        net_home([("qf", qf)], [("target_qf", plain)], [torch.optim.Adam(qf.parameters())])
    tanh = lo.build_nets(dict(a, act="Tanh"))["qf"]
    with pytest.raises(_C.TrlError, match="same activation"):
        net_home([("qf", qf)], [("target_qf", tanh)], [torch.optim.Adam(qf.parameters())])


def test_group_structure_errors_name_the_layer():
    """`mlp_forward_group` of layer lists that differ in their post-ops names the first layer that differs (checked before
    any launch, so on the CPU too)."""
    from torchrl_amd import _C, networks, ops
    mk = lambda ln: networks.Net(input_shape=(5,), output_shape=2, hidden_shapes=[8, 12], append_hidden_shapes=[6],
                                 base_type=networks.MLPBase, activation_func=torch.nn.Tanh, **({"add_ln": True} if ln else {}))
    with_ln, plain = ops.net_layers(mk(True))[0], ops.net_layers(mk(False))[0]
    x = torch.zeros(3, 5)
    with pytest.raises(_C.TrlError, match="behind layer 0"):
        ops.mlp_forward_group([with_ln, plain], [x, x], _C.ACT_TANH)
    mixed = [with_ln[0], (with_ln[1][0], with_ln[1][1], None)] + with_ln[2:]
    with pytest.raises(_C.TrlError, match="behind layer 1"):
        ops.mlp_forward_group([with_ln, mixed], [x, x], _C.ACT_TANH)
    with pytest.raises(_C.TrlError, match="one depth"):
        ops.mlp_forward_group([with_ln, with_ln[1:]], [x, x], _C.ACT_TANH)


def test_without_the_switch_the_engines_refuse_as_before(fx, monkeypatch):
    """TRL_OFFPOLICY_LN unset: the home of every engine, the constructors of SAC / TwinSAC and the collector's policy pass
    refuse an `add_ln` net with the dense kernels' "without LayerNorm" message; plain nets are untouched by the switch."""
    from torchrl_amd import _C, ops
    from torchrl_amd.collector.base import _policy_mlp
    monkeypatch.delenv("TRL_OFFPOLICY_LN")
    g, _ = fx
    for tag in ("sacq_relu", "critic_only_ln", "ddpg_tanh", "dqn_relu"):
        with pytest.raises(_C.TrlError, match="without LayerNorm"):
            _home(tag, g)
    with pytest.raises(_C.TrlError, match="without LayerNorm"):
        lo.build_agent(g, "sacv", "cpu")
    pf = lo.build_nets(lo.args_of(g, "sacq_relu"))["pf"]
    with pytest.raises(_C.TrlError, match="without LayerNorm"):
        _policy_mlp(pf, torch.zeros(2, 11))
    plain = lo.build_nets(lo.args_of(g, "sacq_relu"), pf_ln=False, q_ln=False)["qf1"]
    for on in ("1", None):
        if on:
            monkeypatch.setenv("TRL_OFFPOLICY_LN", on)
        else:
            monkeypatch.delenv("TRL_OFFPOLICY_LN")
        layers, _ = ops.offpolicy_layers(plain)
        assert all(len(l) == 2 for l in layers)
