"""Categorical policies on the CPU side: the torch restatement of the two kernels' arithmetic
(tests/_categorical_ref.py) reproduces the reference fixture (tests/golden/categorical_update.npz, written by
tests/golden/make_golden_categorical.py from the reference's own CategoricalDisPolicy / A2C / PPO), the product's
policy class draws the reference's initial parameters, and the restatement's sampling rule is a sampler."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import _categorical_ref as ref                                                # noqa: E402

TAGS = ["s4", "s17"]


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(REPO, "tests", "golden", "categorical_update.npz"))


def batch_of(g, tag):
    return {k: g[f"{tag}_batch_{k}"] for k in ("obs", "acts", "advs", "values", "estimate_returns")}


def assert_info(info, g, prefix, absent=()):
    """rel 1e-4 / abs 1e-5 on every key the reference logged, minus the `absent` prefixes (which must not be there)."""
    keys = [str(k) for k in g[prefix + "_keys"]]
    want = dict(zip(keys, g[prefix + "_vals"]))
    kept = [k for k in keys if not k.startswith(tuple(absent))] if absent else keys
    assert sorted(info) == sorted(kept)
    for k in kept:
        assert info[k] == pytest.approx(want[k], rel=1e-4, abs=1e-5), k


def assert_params(got, g, prefix):
    for a, b in zip(got, ref.params_from(g, prefix)):
        np.testing.assert_allclose(a.detach().numpy(), b.numpy(), rtol=0, atol=1e-6)


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_policy_outputs_match_reference(g, tag):
    pf = ref.MLP(ref.params_from(g, f"{tag}_pf0_"))
    obs, acts = torch.from_numpy(g[f"{tag}_batch_obs"]), torch.from_numpy(g[f"{tag}_batch_acts"])
    with torch.no_grad():
        logits = pf(obs)
        lp, ent, probs = ref.cat_logp(logits, acts)
        a_det = ref.cat_act(logits, deterministic=True)[0]
    np.testing.assert_allclose(lp.numpy()[:, None], g[f"{tag}_upd_log_prob"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(ent.numpy(), g[f"{tag}_upd_ent"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(probs.numpy(), g[f"{tag}_probs"], rtol=1e-5, atol=1e-7)
    assert np.array_equal(a_det.numpy(), g[f"{tag}_eval_act"])


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_a2c_update_matches_reference(g, tag):
    o = ref.CatUpdate(ref.params_from(g, f"{tag}_pf0_"), ref.params_from(g, f"{tag}_vf0_"), plr=3e-4, vlr=1e-3,
                      entropy_coeff=0.01)
    info = o.update(batch_of(g, tag), ref.LOSS_A2C)
    assert_info(info, g, f"{tag}_a2c_info")
    assert_params(o.pf.params, g, f"{tag}_a2c_pf1_")
    assert_params(o.vf.params, g, f"{tag}_a2c_vf1_")


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_ppo_chain_matches_reference(g, tag):
    o = ref.CatUpdate(ref.params_from(g, f"{tag}_pf0_"), ref.params_from(g, f"{tag}_vf0_"), plr=3e-4, vlr=3e-4,
                      entropy_coeff=0.005, clip_para=0.2, target_params=ref.params_from(g, f"{tag}_ppo_tpf0_"))
    for s, clipv in enumerate(g[f"{tag}_ppo_clipv"]):
        info = o.update(batch_of(g, tag), ref.LOSS_PPO_CLIP, clipped_value_loss=bool(clipv))
        assert_info(info, g, f"{tag}_ppo_info{s}", absent=("log_std/",))
        assert_params(o.pf.params, g, f"{tag}_ppo_pf{s + 1}_")
        assert_params(o.vf.params, g, f"{tag}_ppo_vf{s + 1}_")


@pytest.mark.parametrize("tag", TAGS)
def test_policy_constructs_with_the_reference_draw(g, tag):
    """Fails on a build whose CategoricalDisPolicy is the stub that raises at construction."""
    from torchrl_amd import networks, policies
    D, A, H, B = (int(x) for x in g[f"{tag}_args"])
    torch.manual_seed(5 + D)
    net = dict(hidden_shapes=[H, H], append_hidden_shapes=[], base_type=networks.MLPBase, activation_func=torch.nn.Tanh)
    pf = policies.CategoricalDisPolicy(input_shape=D, output_shape=A, **net)
    vf = networks.Net(input_shape=(D,), output_shape=1, **net)
    assert pf.continuous is False
    for prefix, mod in ((f"{tag}_pf0_", pf), (f"{tag}_vf0_", vf)):
        sd = mod.state_dict()
        assert sorted(k.replace(".", "__") for k in sd) == sorted(k[len(prefix):] for k in g.files if k.startswith(prefix))
        for k, v in sd.items():
            assert np.array_equal(v.numpy(), g[prefix + k.replace(".", "__")]), k
    # the CPU protocol (torch modules; the kernels take over on a GPU): forward = the reference's probabilities
    obs = torch.from_numpy(g[f"{tag}_batch_obs"])
    with torch.no_grad():
        np.testing.assert_allclose(pf(obs).numpy(), g[f"{tag}_probs"], rtol=1e-5, atol=1e-7)
        out = pf.update(obs, torch.from_numpy(g[f"{tag}_batch_acts"]))
    assert out["log_prob"].shape == (B, 1) and out["ent"].shape == (B,)
    np.testing.assert_allclose(out["log_prob"].numpy(), g[f"{tag}_upd_log_prob"], rtol=1e-5, atol=2e-6)
    assert np.array_equal(pf.eval_act(obs), g[f"{tag}_eval_act"])


def test_refusals_on_the_cpu():
    from torchrl_amd import _C, networks, policies
    from torchrl_amd.algo import TRPO, VMPO
    with pytest.raises(_C.TrlError, match="not built"):
        policies.CategoricalDisPolicy()
    with pytest.raises(_C.TrlError, match="not built"):
        policies.CategoricalDisPolicy(output_shape=3)
    with pytest.raises(_C.TrlError, match="CNN"):
        policies.CategoricalDisPolicy(input_shape=(4, 84, 84), output_shape=6, base_type=networks.CNNBase,
                                      hidden_shapes=[[32, [8, 8], [4, 4], [0, 0]]])
    pf = policies.CategoricalDisPolicy(input_shape=4, output_shape=2, base_type=networks.MLPBase, hidden_shapes=[8, 8])
    vf = networks.Net(input_shape=(4,), output_shape=1, base_type=networks.MLPBase, hidden_shapes=[8, 8])
    with pytest.raises(_C.TrlError, match="TRPO with a categorical policy"):
        TRPO(max_kl=0.01, cg_damping=0.1, v_opt_times=1, cg_iters=10, residual_tol=1e-10, pf=pf, vf=vf)
    with pytest.raises(_C.TrlError, match="VMPO with a categorical policy"):
        VMPO(pf=pf, vf=vf)


def test_sampling_rule_is_a_sampler():
    """2^20 Philox uniforms through the restatement's rule on fixed logits: every empirical frequency within
    5 sqrt(p (1 - p) / n) of p."""
    n = 1 << 20
    logits = torch.tensor([[0.3, -1.2, 2.0, 0.0, -3.0, 1.1]]).expand(n, 6).contiguous()
    u = ref.uniforms(0xC011, 7, 1, n)[0]
    assert u.dtype == np.float32 and u.min() > 0.0 and u.max() < 1.0
    a = ref.cat_act(logits, u)[0].numpy()
    p = torch.softmax(logits[0].double(), dim=-1).numpy()
    freq = np.bincount(a, minlength=6) / n
    for k in range(6):
        assert abs(freq[k] - p[k]) <= 5.0 * np.sqrt(p[k] * (1.0 - p[k]) / n), (k, freq[k], p[k])


@pytest.mark.parametrize("A", [2, 6, 18])
def test_borderline_rows_of_the_action_cases_stay_under_the_cap(A):
    """The GPU test lets rows whose threshold lies within 1e-5 S of a prefix sum differ, at most 1 % of them: with its
    seeded logits the restatement alone must be far below that cap (expected share ~ 2 A 1e-5)."""
    logits, seed, counter = ref.act_case(A)
    u = ref.uniforms(seed, counter, 1, logits.shape[0])[0]
    a, lp, pre, S = ref.cat_act(logits, u)
    share = ref.borderline(u, pre, S).float().mean().item()
    print("A=%d borderline share %.5f" % (A, share))
    assert share <= 0.01
    assert int(a.min()) >= 0 and int(a.max()) < A
