"""The TRPO / V-MPO kernels of the categorical and the state-dependent-std head (torchrl_amd/csrc/k_trpo.hip, k_vmpo.hip),
each entry point called directly and compared element by element with the float64 restatement
(tests/_vmpo_trpo_heads_ref.py) on identical float32 inputs: n = 1, 2, 255, 256, 257, 1025 (one, two and five blocks and
both sides of each), A = 2 / 6 / 64 logits and 1 / 6 / 32 action dimensions, both tanh_action values, the log_std clamp
and its closed gate, logits spread until a probability is zero, actions taken with log pi ~ -18 and ~ -30, stored actions
outside [0, A), eta at its floor, equal advantages, both kl_reduce values; the Fisher-vector product through the engine's
`_fvp` against double backward.

Bounds: err <= K M + 2^-126 per element, M the element's running magnitude and K = 4 x the deviation of the float32 run of
the restatement from its float64 run (tests/_vmpo_trpo_heads_ref.py::K; tests/test_vmpo_trpo_heads_cpu.py holds that run to
the same bounds).  Every test prints its worst err / (K M); profiles/NOTES_vmpo_trpo_heads.md has them from one run."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _vmpo_trpo_heads_ref as ref                                            # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = 7.0
TRPO_CASES = ref.trpo_cases()
VMPO_CASES = ref.vmpo_cases()


def dev(x):
    return x.to(DEV).contiguous()


def run_surrogate(kind, c, tanh):
    from torchrl_amd import _C
    info = torch.full((6,), SENTINEL, dtype=torch.float64, device=DEV)
    if kind == "cat":
        d = _C.trpo_surrogate_cat(dev(c["head"]), dev(c["acts"]), dev(c["adv"]), ref.C_ENT, info)
    else:
        d = _C.trpo_surrogate_sd(dev(c["head"]), dev(c["acts"]), dev(c["adv"]), tanh, ref.C_ENT, info)
    torch.cuda.synchronize()
    info = info.cpu().numpy()
    assert info[5] == SENTINEL                                                # five slots, as the Gaussian entry point
    return dict(d_head=d.cpu(), info=info[:5])


def run_vmpo(kind, c, tanh, dual, red):
    from torchrl_amd import _C
    dual_d = torch.from_numpy(np.asarray(dual, dtype=np.float32).copy()).to(DEV)
    info = torch.full((13,), SENTINEL, dtype=torch.float64, device=DEV)
    h = ref.HYPER
    if kind == "cat":
        d = _C.vmpo_losses_cat(dev(c["head"]), dev(c["thead"]), dev(c["acts"]), dev(c["adv"]), dual_d, red, h["eta_eps"],
                               h["alpha_eps"], h["lr"], info)
    else:
        d = _C.vmpo_losses_sd(dev(c["head"]), dev(c["thead"]), dev(c["acts"]), dev(c["adv"]), dual_d, tanh, red, h["eta_eps"],
                              h["alpha_eps"], h["lr"], info)
    torch.cuda.synchronize()
    info = info.cpu().numpy()
    assert info[12] == SENTINEL
    return dict(d_head=d.cpu(), info=info[:12], dual=dual_d.cpu().double().numpy())


@pytest.mark.parametrize("name", sorted(TRPO_CASES))
def test_trpo_surrogate_vs_float64(name):
    kind, c, tanh = TRPO_CASES[name]
    want = ref.trpo_surrogate(kind, c["head"].double(), c["acts"].double(), c["adv"].double(), tanh, ref.C_ENT)
    got = run_surrogate(kind, c, tanh)
    r_d = ref.ratio(got["d_head"], want["d_head"], want["mag"]["d_head"]) / ref.K["trpo_%s_d_head" % kind]
    r_i = ref.ratio(got["info"], want["info"], want["mag"]["info"]) / ref.K["trpo_%s_info" % kind]
    print("trpo surrogate %s: err / bound  d_head %.3f  info %.3f" % (name, r_d, r_i))
    assert r_d <= 1.0 and r_i <= 1.0
    again = run_surrogate(kind, c, tanh)                                       # fixed fold order: the same bits
    assert torch.equal(again["d_head"], got["d_head"]) and np.array_equal(again["info"], got["info"], equal_nan=True)


@pytest.mark.parametrize("name", sorted(TRPO_CASES))
def test_fisher_scale_vs_float64(name):
    from torchrl_amd import _C
    kind, c, _ = TRPO_CASES[name]
    t = ref.F32(np.random.RandomState(5).randn(*c["head"].shape))
    want, mag = ref.fisher_scale(kind, t.double(), c["head"].double())
    got = (_C.fisher_scale_cat if kind == "cat" else _C.fisher_scale_sd)(dev(t), dev(c["head"])).cpu()
    r = ref.ratio(got, want, mag) / ref.K["fisher_" + kind]
    print("fisher scale %s: err / bound %.3f" % (name, r))
    assert r <= 1.0
    if kind == "cat":                                                          # rows of (diag(p) - p p^T) t sum to zero
        assert got.double().sum(-1).abs().max().item() <= 8 * ref.U * mag.sum(-1).max().item()


@pytest.mark.parametrize("name", sorted(VMPO_CASES))
def test_vmpo_losses_vs_float64(name):
    kind, c, tanh, dual, red = VMPO_CASES[name]
    dual32 = np.asarray(dual, dtype=np.float32)
    want = ref.vmpo_losses(kind, c["head"].double(), c["thead"].double(), c["acts"].double(), c["adv"].double(), dual32,
                           tanh, red, **ref.HYPER)
    got = run_vmpo(kind, c, tanh, dual, red)
    r_d = ref.ratio(got["d_head"], want["d_head"], want["mag"]["d_head"]) / ref.K["vmpo_%s_d_head" % kind]
    r_i = ref.ratio(got["info"][:10], want["info"][:10], want["mag"]["info"]) / ref.K["vmpo_%s_info" % kind]
    bound = ref.dual_bounds(want, dual32, ref.HYPER["lr"], ref.K["vmpo_%s_g" % kind])
    err = np.abs(got["dual"] - np.asarray(want["dual"]))
    r_dual = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    print("vmpo losses %s: err / bound  d_head %.3f  info %.3f  dual %.3f" % (name, r_d, r_i, r_dual))
    assert r_d <= 1.0 and r_i <= 1.0 and r_dual <= 1.0
    assert got["info"][10] == got["dual"][1] and got["info"][11] == got["dual"][0]   # alpha, eta after the step
    assert got["dual"][6] == dual32[6] + 1.0 and got["dual"][0] >= np.float32(1e-8)
    # ---- the KL slots of the two reductions ----
    n = c["head"].shape[0]
    if red == ref.KL_SUM:
        assert np.isnan(got["info"][6]) and got["info"][5] == got["info"][7] == got["info"][8]
    else:
        assert np.isnan(got["info"][6]) == (n == 1) and got["info"][8] <= got["info"][5] <= got["info"][7]
    assert np.isnan(got["info"][2]) == (n == 1)
    again = run_vmpo(kind, c, tanh, dual, red)
    assert torch.equal(again["d_head"], got["d_head"]) and np.array_equal(again["info"], got["info"], equal_nan=True)
    assert np.array_equal(again["dual"], got["dual"])


def test_gaussian_entry_point_keeps_its_bits_beside_the_head_kernels():
    """The shared fold gained `kl_reduce`; trl_vmpo_losses_f32 passes the mean: its KL slots are those of a mean
    (tests/test_vmpo_trpo_kernels_gpu.py holds every value of that entry point to its float64 restatement)."""
    from torchrl_amd import _C
    import _vmpo_trpo_ref as gref
    c = gref.vmpo_case(300, 6, True)
    dual = torch.tensor(gref.DUAL0, device=DEV)
    info = torch.zeros(12, dtype=torch.float64, device=DEV)
    _C.vmpo_losses(*[dev(c[k]) for k in ("mean", "tmean", "logstd", "tlogstd", "acts", "adv")], dual, True, 0.02, 0.1, 1e-3,
                   torch.zeros(6, device=DEV), info)
    i = info.cpu().numpy()
    assert np.isfinite(i).all() and i[8] < i[5] < i[7] and i[6] > 0


# ---------------------------------------------------------------- F v through the engine
class _Stub:
    epoch_frames = 0


def _trpo_agent(kind, D, H, seed):
    import torchrl.networks as networks
    import torchrl.policies as policies
    from torchrl.algo import TRPO
    from torchrl.env import get_vec_env
    from torchrl.env.synth import SynthVecEnv
    net = dict(hidden_shapes=[H, H], append_hidden_shapes=[], base_type=networks.MLPBase, activation_func=torch.nn.Tanh)
    cls = policies.CategoricalDisPolicy if kind == "cat" else policies.GuassianContPolicy
    pf = cls(input_shape=D, output_shape=6, **net)
    vf = networks.Net(input_shape=(D,), output_shape=1, **net)
    params = ref.small_mlp(D, H, 6, seed)
    lin = [m for m in list(pf.base.seq_fcs) + list(pf.seq_append_fcs) if isinstance(m, torch.nn.Linear)]
    with torch.no_grad():
        for m, (w, b) in zip(lin, zip(params[0::2], params[1::2])):
            m.weight.copy_(w); m.bias.copy_(b)
    if kind == "cat":                                                          # (only the kind of its action space is read)
        env = get_vec_env("SynthCheetahDiscrete-v0", {"reward_scale": 1, "obs_norm": False}, 4, device=DEV)
    else:
        env = SynthVecEnv(4, obs_dim=D, act_dim=3, device=DEV)
    agent = TRPO(pf=pf, vf=vf, plr=3e-4, vlr=1e-3, max_kl=0.01, cg_damping=0.1, cg_iters=10, residual_tol=1e-10,
                 entropy_coeff=0.01, shuffle=True, v_opt_times=2, tau=0.95, discount=0.99, num_epochs=10, batch_size=64,
                 gae=True, env=env, replay_buffer=None, collector=_Stub(),
                 logger=None, device=DEV, save_dir=None)
    return agent, params


@pytest.mark.parametrize("net", sorted(ref.FVP_NETS))
@pytest.mark.parametrize("kind", ["cat", "sd"])
def test_fisher_vector_product_through_the_engine(kind, net):
    D, H, n = ref.FVP_NETS[net]
    agent, params = _trpo_agent(kind, D, H, 77 + D)
    eng = agent.engine()
    rs = np.random.RandomState(78 + D)
    obs = ref.F32(rs.randn(n, D))
    eng.obs, eng.n, eng.tanh_action = obs.to(DEV), n, False
    _, eng.tape = eng._forward(eng.pf_layers)
    P = sum(p.numel() for p in params)
    assert eng.P_pf == P                                                       # no logstd tail behind the head layer
    p64 = [p.double() for p in params]
    u, v = ref.F32(rs.randn(P)), ref.F32(rs.randn(P))
    damp = agent.cg_damping
    fu = eng._fvp(u.to(DEV)).cpu().double() - damp * u.double()
    fv = eng._fvp(v.to(DEV)).cpu().double() - damp * v.double()
    worst = 0.0
    for vec, got in ((u, fu), (v, fv)):
        want = ref.fvp_double_backward(kind, p64, obs.double(), vec.double())
        tol = ref.FVP_TOL * max(1.0, want.abs().max().item())
        worst = max(worst, (got - want).abs().max().item() / tol)
    sym = abs((u.double() @ fv - v.double() @ fu).item())
    sym_tol = ref.FVP_TOL * (u.abs().sum().item() * max(1.0, fv.abs().max().item())
                             + v.abs().sum().item() * max(1.0, fu.abs().max().item()))
    print("F v %s %s: err / bound %.3f  |u.Fv - v.Fu| / bound %.3f  v.Fv %.3e" % (kind, net, worst, sym / sym_tol,
                                                                              (v.double() @ fv).item()))
    assert worst <= 1.0 and sym <= sym_tol
    assert (v.double() @ fv).item() >= 0.0 and (u.double() @ fu).item() >= 0.0


def test_refusals_of_the_entry_points():
    from torchrl_amd import _C
    lib = _C.lib()
    x = torch.zeros(8, 6, device=DEV)
    a = torch.zeros(8, device=DEV)
    info = torch.zeros(12, dtype=torch.float64, device=DEV)
    ws = torch.zeros(64, dtype=torch.float64, device=DEV)
    dual = torch.tensor(ref.DUAL0, device=DEV)
    p = lambda t: t.data_ptr()
    assert lib.trl_trpo_surrogate_cat_f32(p(x), p(a), p(a), 8, 6, 0.0, None, p(info), p(ws), None) != 0        # null output
    assert lib.trl_trpo_surrogate_cat_f32(p(x), p(a), p(a), 0, 6, 0.0, p(x), p(info), p(ws), None) != 0        # empty batch
    assert lib.trl_vmpo_losses_cat_f32(p(x), p(x), p(a), p(a), p(dual), 8, 6, 2, 0.02, 0.1, 1e-3, p(x), p(info), p(ws), None) != 0
    assert lib.trl_vmpo_losses_sd_f32(p(x), p(x), p(x), p(a), p(dual), 8, 3, 0, 5, 0.02, 0.1, 1e-3, p(x), p(info), p(ws), None) != 0
    assert lib.trl_fisher_scale_sd_f32(p(x), None, 8, 3, p(x), None) != 0
