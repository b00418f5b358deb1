"""One-launch rollouts for 128- and 256-wide `add_ln=True` networks (trl_rollout_synth_wide_ln_f32; rollout_wide_kernel /
value_pass_wide_kernel with LN = true, torchrl_amd/csrc/trl_rollout_wide.h) through the collector's opt-in route: stored cells
against the float64 restatement of tests/_layernorm_rollout_ref.py (bounds unchanged), a value pass of more rounds than
workgroups, the fused route against per-step collection, routing and refusals, whole PPO iterations.

Measured worst err / bound per quantity: profiles/NOTES_wide_layernorm_rollout.md."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import test_layernorm_rollout_gpu as LT                                       # noqa: E402
import _gauss_sd_rollout_ref as rr                                            # noqa: E402
import _layernorm_rollout_ref as L                                            # noqa: E402
from _rollout_ref import F32, U                                               # noqa: E402
from test_layernorm_rollout_gpu import RING_KEYS, _Log, collect, noise_of     # noqa: E402

SWITCH = "TRL_WIDE_LN_FUSED_ROLLOUT"                                          # the fused route is opt-in
wcase = lambda H, *a, **kw: dict(LT.case(*a, **kw), H=H)
case_id = lambda c: "H%d-%s" % (c["H"], LT.case_id(c))
# pairwise over H x head x (policy LN, critic LN) x D in {3, 17, 27} x A in {head minimum, 6, 8} x act x N in {16, 17, 40}; a
# ZeroNet critic; at each width the two planted first layers (zero variance: W1 = 0, constant b1; large mean: ReLU, b1 = 64 + U)
CELL_CASES = [wcase(128, "gauss", 3, 1, "tanh", 16, 1, 1, 1), wcase(256, "gauss", 17, 6, "relu", 17, 1, 0, 2, tanh=False),
              wcase(128, "gauss", 27, 8, "tanh", 40, 0, 1, 3), wcase(256, "cat", 3, 2, "relu", 40, 1, 1, 4),
              wcase(128, "cat", 17, 8, "tanh", 16, 0, 1, 5), wcase(256, "cat", 27, 6, "tanh", 17, 1, 0, 6),
              wcase(128, "sd", 3, 8, "tanh", 17, 1, 0, 7), wcase(256, "sd", 17, 1, "relu", 16, 0, 1, 8),
              wcase(128, "sd", 27, 6, "relu", 40, 1, 1, 9), wcase(256, "gauss", 17, 6, "tanh", 17, 1, 0, 10, zero=True),
              wcase(128, "gauss", 17, 6, "tanh", 16, 1, 1, 11, plant="zero-variance"),
              wcase(256, "sd", 27, 6, "tanh", 17, 1, 1, 12, plant="zero-variance"),
              wcase(128, "sd", 27, 6, "relu", 17, 1, 1, 13, plant="large-mean"),
              wcase(256, "gauss", 17, 8, "relu", 40, 1, 1, 14, plant="large-mean")]


def nets_of(c, H):
    """`test_layernorm_rollout_gpu.nets_of` at width H: gamma in +-[0.5, 2], beta in [-1, 1], heads x 30, the planted layers."""
    from torchrl_amd import networks, policies
    torch.manual_seed(c["seed"])
    D, A = c["D"], c["A"]
    net = lambda ln: dict(hidden_shapes=[H, H] if isinstance(H, int) else list(H), append_hidden_shapes=[],
                          base_type=networks.MLPBase, add_ln=bool(ln),
                          activation_func={"tanh": torch.nn.Tanh, "relu": torch.nn.ReLU}[c["act"]])
    if c["head"] == "gauss":
        pf = policies.GuassianContPolicyBasicBias(input_shape=D, output_shape=A, tanh_action=c["tanh"], **net(c["pf_ln"]))
    elif c["head"] == "cat":
        pf = policies.CategoricalDisPolicy(input_shape=D, output_shape=A, **net(c["pf_ln"]))
    else:
        pf = policies.GuassianContPolicy(input_shape=D, output_shape=2 * A, tanh_action=c["tanh"], **net(c["pf_ln"]))
    vf = networks.ZeroNet() if c["zero"] else networks.Net(input_shape=(D,), output_shape=1, **net(c["vf_ln"]))
    with torch.no_grad():
        for n_ in (pf, vf):
            for m in n_.modules():
                if isinstance(m, torch.nn.LayerNorm):
                    w = m.weight.numel()
                    m.weight.copy_((0.5 + 1.5 * torch.rand(w)) * (1.0 - 2.0 * (torch.rand(w) < 0.3).float()))
                    m.bias.uniform_(-1.0, 1.0)
            if not isinstance(n_, networks.ZeroNet):
                first, last = n_.base.seq_fcs[0], n_.seq_append_fcs[-1]
                last.weight.mul_(30.0)
                if c["plant"] == "zero-variance":
                    first.weight.zero_()
                    first.bias.fill_(0.3)
                elif c["plant"] == "large-mean":
                    first.bias.copy_(64.0 + torch.rand(first.bias.numel()) - 0.5)
        if c["head"] == "gauss":
            pf.logstd.fill_(-1.5)
        elif c["head"] == "sd":
            pf.seq_append_fcs[-1].bias[A:].fill_(-1.5)
    return pf, vf


@pytest.fixture
def route(monkeypatch):
    """`LT.make_collector` over this file's nets; `route(on)` clears the rollout switches and sets this route's."""
    monkeypatch.setattr(LT, "nets_of", lambda c: nets_of(c, c["H"]))
    def set_route(on=True, **env):
        LT.clean_env(monkeypatch, switch=False)
        for k in ("TRL_WIDE_FUSED_ROLLOUT", SWITCH):
            monkeypatch.delenv(k, raising=False)
        for k, v in dict({SWITCH: "1"} if on else {}, **env).items():
            monkeypatch.setenv(k, v)
    return set_route


def test_float32_restatement_stays_inside_the_bounds():
    """`LT.test_float32_restatement_stays_inside_the_bounds` over this file's cases, each at both widths (no GPU)."""
    for c in [dict(c, H=H) for c in CELL_CASES for H in (128, 256)]:
        pf, vf = nets_of(c, c["H"])
        P, V = L.params_of(pf), None if c["zero"] else L.params_of(vf)
        rs, M = np.random.RandomState(c["seed"]), 3 * c["N"]
        obs, nxt = (0.5 * rs.randn(M, c["D"])).astype(np.float32), np.tanh(rs.randn(M, c["D"])).astype(np.float32)
        eps = noise_of(c, 3, c["N"])
        if c["head"] == "cat":
            acts = rs.randint(0, c["A"], (M, 1)).astype(np.float32)
        else:
            acts = L.quantities(c, P, V, obs, nxt, eps, np.zeros((M, c["A"])), np.float32)["act"]
        r = L.ratios(L.quantities(c, P, V, obs, nxt, eps, acts, np.float32), L.quantities(c, P, V, obs, nxt, eps, acts))
        print(case_id(c), {k: round(v, 4) for k, v in r.items()})
        assert all(v <= 1.0 for v in r.values()), (case_id(c), r)


@pytest.mark.gpu
@pytest.mark.parametrize("c", CELL_CASES, ids=case_id)
def test_stored_cells_vs_float64_restatement(c, route):
    route()
    N, T = c["N"], LT.T_CELLS
    pf, vf, env, buf, col = LT.make_collector(c, N, T, LT.HORIZON, LT.MAX_FRAMES)
    assert col._spec is not None and col._ln == (bool(c["pf_ln"]), bool(c["vf_ln"]))     # (`_spec` is None on the parent commit)
    g = collect(col, buf)
    assert all(np.isfinite(g[k]).all() for k in RING_KEYS)
    flat = lambda k: g[k].reshape(T * N, -1)
    over = flat("terminals")[:, 0] == 1.0
    assert over.reshape(T, N)[1].all() and over.sum() == N and g["time_limits"].sum() == 0
    q = L.quantities(c, L.params_of(pf), None if c["zero"] else L.params_of(vf), flat("obs"), flat("next_obs"), noise_of(c, T, N),
                     flat("acts"))
    got = dict(logp=flat("old_logp")[:, 0], v=flat("values")[:, 0])
    if c["head"] == "cat":
        assert q["allowed"].all(), "a stored index is neither the restated draw nor its neighbour across a close prefix sum"
    else:
        got["act"] = flat("acts")
    r = L.ratios(got, q)
    if c["plant"] == "zero-variance":                                  # the normed row is beta exactly, whatever the input
        # (the float64 restatement of equal rows: equal up to the last bit of a 256-term BLAS dot, which depends on the row's place)
        assert np.ptp(q["v"]) <= 4.0 * np.finfo(np.float64).eps * np.abs(q["v"]).max()
        assert np.ptp(flat("values")) <= 2.0 * q["b_v"][0]
    # rewards: the raw reward from the stored next_obs / actions, + discount V(next_obs) on the over-length cells; boot
    a = np.ones((T * N, 1)) if c["head"] == "cat" else flat("acts").astype(np.float64)
    asq, scale, disc = (a * a).sum(-1), F32(env.effective_reward_scale), F32(col.discount)
    raw = flat("next_obs")[:, 0].astype(np.float64) - F32(0.1) * asq
    want = scale * raw + over * disc * q["v2"]
    b = scale * U * (6.0 * F32(0.1) * asq + 2.0 * np.abs(raw)) + over * (disc * q["b_v2"] + U * (np.abs(disc * q["v2"]) + np.abs(want)))
    r["rewards"] = float((np.abs(flat("rewards")[:, 0] - want) / b).max())
    last = slice((T - 1) * N, T * N)
    r["boot"] = float((np.abs(buf._boot.cpu().numpy().reshape(N) - q["v2"][last]) / q["b_v2"][last]).max())
    print(case_id(c), {k: round(v, 4) for k, v in r.items()})
    assert all(v <= 1.0 for v in r.values()), r


@pytest.mark.gpu
@pytest.mark.parametrize("H,T", [(128, 32), (256, 17)])
def test_value_pass_walks_more_rounds_than_workgroups(H, T, route):
    """530 envs: 265 rounds of 4 column tiles (H = 128), 282 of 2 (H = 256), on a grid capped at 256; critic normed, policy plain."""
    route()
    c, N = wcase(H, "gauss", 17, 6, "tanh", 530, 0, 1, 15), 530
    pf, vf, env, buf, col = LT.make_collector(c, N, T, LT.HORIZON, LT.MAX_FRAMES)
    assert col._spec is not None and col._ln == (False, True)
    g = collect(col, buf)
    V = L.params_of(vf)
    for got, x in ((g["values"].reshape(-1), g["obs"].reshape(T * N, -1)),
                   (buf._boot.cpu().numpy().reshape(N), g["next_obs"].reshape(T, N, -1)[T - 1])):
        v, amp = L.forward(V, x, "tanh")
        ratio = float((np.abs(got - v[:, 0]) / (1e-5 * (1.0 + np.abs(v[:, 0])) * amp)).max())
        print("H%d rounds: worst err / bound %.4f over %d values" % (H, ratio, len(got)))
        assert ratio <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("H,head,D,A,ln", [(128, "gauss", 17, 6, (1, 1)), (256, "sd", 27, 8, (1, 0)), (128, "cat", 17, 6, (0, 1))])
def test_fused_route_vs_per_step_collection(H, head, D, A, ln, route, monkeypatch):
    """Switch set: one `_C.rollout_wide_ln` per rollout and no per-step launch sequence; switch unset: the per-step route (what
    the parent commit takes) on the same nets, env seed and Philox noise."""
    from torchrl_amd import _C
    N, T, horizon = 33, 4, 3
    c = wcase(H, head, D, A, "tanh", N, ln[0], ln[1], 40 + H)
    route()
    pf, vf, env, buf, col = LT.make_collector(c, N, T, horizon, 999, noise_mode="device")
    assert col._spec is not None and col._ln == (bool(ln[0]), bool(ln[1]))
    calls, real = [], _C.rollout_wide_ln
    monkeypatch.setattr(_C, "rollout_wide_ln", lambda *a: (calls.append(a[1:4]), real(*a))[1])
    monkeypatch.setattr(col, "_step_launches", lambda *a, **k: pytest.fail("a per-step launch sequence on the fused route"))
    fused, ev = collect(col, buf), col.eval_one_epoch()
    assert calls == [({"gauss": 0, "cat": 1, "sd": 2}[head], bool(ln[0]), bool(ln[1]))] * 2
    route(on=False)
    pf2, vf2, env2, buf2, col2 = LT.make_collector(c, N, T, horizon, 999, noise_mode="device" if head == "cat" else "host")
    assert col2._spec is None
    if head != "cat":
        col2._host_noise = lambda n, e: rr.device_noise(n, N, A, c["seed"], step0=col2.global_step).to(e.device).contiguous()
    step, ev2 = collect(col2, buf2), col2.eval_one_epoch()
    for k, (rtol, atol) in rr.TOL.items():
        ratio, err = rr.worst_ratio(fused[k], step[k], rtol, atol)
        print("%s %s: max abs err %.3e, worst err / bound %.4f" % (case_id(c), k, err, ratio))
        assert ratio <= 1.0, k
    assert fused["terminals"].sum() > 0 and fused["episodes"] and len(fused["episodes"]) == len(step["episodes"])
    np.testing.assert_allclose(fused["episodes"], step["episodes"], rtol=0, atol=1e-5 * horizon)
    assert fused["epoch_reward"] == pytest.approx(step["epoch_reward"], abs=1e-5 * T * N)
    for k in ("t_env", "cur_step", "episode_idx"):
        assert torch.equal(getattr(env, k).cpu(), getattr(env2, k).cpu()), k
    assert len(ev["eval_rewards"]) == N and ev["eval_traj_length"] == ev2["eval_traj_length"] == horizon
    np.testing.assert_allclose(ev["eval_rewards"], ev2["eval_rewards"], rtol=0, atol=1e-5 * horizon)


@pytest.mark.gpu
def test_routing_and_refusals(route):
    from torchrl_amd import _C
    from _rollout_launch import DEV, Launcher
    from test_wide_rollout_gpu import wide_case
    c = wcase(128, "gauss", 17, 6, "tanh", 16, 1, 1, 50)
    mk = lambda c, **kw: LT.make_collector(c, 16, 4, 9, 99, **kw)[4]
    route()
    assert mk(c)._ln == (True, True) and mk(dict(c, H=256, vf_ln=0))._ln == (True, False)
    for off in (dict(c, H=(128, 256)), dict(c, H=192), dict(c, pf_ln=0, vf_ln=0), dict(c, H=64)):
        col = mk(off)
        assert col._spec is None and not col._ln, off["H"]
    assert mk(c, obs_norm=True)._spec is None
    route(TRL_NO_RT_ROLLOUT="1")
    assert mk(c)._spec is None
    route(on=False)
    assert mk(c)._spec is None and mk(c)._ln is None
    run = Launcher(wide_case(128, "gauss", 17, 6, "tanh", 17, 5, "host", 90))
    for field, value, match in (("H", 64, "outside the head's range"), ("D", 33, "outside the head's range"),
                                ("A", 9, "outside the head's range"), ("norm_state", 64, "no running observation normaliser")):
        a = run.args()
        a.H = 128
        setattr(a, field, value)
        with pytest.raises(_C.TrlError, match=match):
            _C.rollout_wide_ln(a, 0, True, True, 0, 0, DEV)
        torch.cuda.synchronize()
        assert run.untouched(), field


@pytest.mark.gpu
def test_two_ppo_iterations_on_the_shipped_shape(route):
    """17 -> 128 -> 128 `add_ln` (config/ppo_synth_halfcheetah_ln.json): the rollout reads the block the generic engine steps."""
    from torchrl_amd import _C, algo as algos
    route()
    N, T = 32, 16
    np.random.seed(4)
    pf, vf, env, buf, col = LT.make_collector(wcase(128, "gauss", 17, 6, "tanh", N, 1, 1, 60), N, T, 9, 999, noise_mode="device")
    assert col._spec == (17, 128, 6, _C.ACT_TANH) and col._ln == (True, True)
    logger = _Log()
    agent = algos.PPO(pf=pf, vf=vf, plr=3e-4, vlr=3e-4, clip_para=0.2, opt_epochs=2, entropy_coeff=0.005, tau=0.95, shuffle=True,
                      discount=0.99, num_epochs=10, batch_size=256, gae=True, env=env, replay_buffer=buf, collector=col,
                      logger=logger, device=torch.device("cuda:0"), save_dir=None)
    eng = agent.engine()
    before, p0 = _C.eager_fallback_count(), pf.flat_plan_params().clone()
    for epoch in range(2):
        assert pf.flat_plan_params().data_ptr() == eng.flat.data_ptr()
        res = col.train_one_epoch()
        agent.current_epoch = epoch
        agent.update_per_epoch()
        assert np.isfinite(res["train_epoch_reward"]) and len(res["train_rewards"]) > 0
    torch.cuda.synchronize()
    assert len(logger.infos) > 0 and all(np.isfinite(list(i.values())).all() for i in logger.infos)
    assert _C.eager_fallback_count() == before and not torch.equal(p0, pf.flat_plan_params())
