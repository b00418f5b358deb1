"""The policy head as one parameter, without a GPU: the `*_supported`, `*_partial_stride` and `*_reduce_adam_workspace`
entry points of the three heads (Gaussian with a free logstd, categorical, state-dependent-std Gaussian) against closed
forms written out here, over the whole grid of shapes around their limits; and `head_kind`, the one place the Python
layer decides which head a policy has."""
import pytest

EUNSUPPORTED = -2
RED_CHUNK = 64                                        # parameters per block of the fold launches (k_ppo.hip)
INVALID_ACT = 7
# head: (prefix of the update entry points, prefix of the rollout's, smallest A, largest A, head rows per A, logstd tail per A)
HEADS = {"gauss": ("trl_ppo_", "trl_rollout_", 1, 8, 1, 1),
         "cat": ("trl_ppo_cat_", "trl_rollout_cat_", 2, 8, 1, 0),
         "sd": ("trl_ppo_sd_", "trl_rollout_sd_", 1, 8, 2, 0)}
GRID = [(D, H, A) for D in range(1, 34) for H in (32, 64) for A in range(0, 10)]


@pytest.fixture(scope="module")
def built_lib():
    from torchrl_amd import build
    return build.build(verbose=False)


def _shape_ok(head, D, H, A):
    lo, hi = HEADS[head][2:4]
    return H == 64 and 2 <= D <= 32 and lo <= A <= hi


def _stride(head, D, H, A):
    R, tail = HEADS[head][4] * A, HEADS[head][5] * A
    p_vf = H * D + H + H * H + H + H + 1
    p_pf = H * D + H + H * H + H + R * H + R + tail
    return (max(p_pf, p_vf) + 63) // 64 * 64


@pytest.mark.parametrize("head", sorted(HEADS))
def test_supported_truth_table(built_lib, head):
    from torchrl_amd import _C
    lib = _C.lib()
    names = [HEADS[head][1] + "supported"] + ([] if head == "gauss" else [HEADS[head][0] + "supported"])
    for name in names:
        fn = getattr(lib, name)
        for D, H, A in GRID:
            for act in (_C.ACT_TANH, _C.ACT_RELU, INVALID_ACT):
                want = int(_shape_ok(head, D, H, A) and act in (_C.ACT_TANH, _C.ACT_RELU))
                assert fn(D, H, A, act) == want, (name, D, H, A, act)


@pytest.mark.parametrize("head", sorted(HEADS))
def test_partial_stride_and_workspace(built_lib, head):
    from torchrl_amd import _C
    lib = _C.lib()
    stride = getattr(lib, HEADS[head][0] + "partial_stride")
    workspace = getattr(lib, HEADS[head][0] + "reduce_adam_workspace")
    wrapper = getattr(_C, HEADS[head][0][4:] + "partial_stride")                  # _C.ppo_[cat_|sd_]partial_stride
    for D, H, A in GRID:
        if _shape_ok(head, D, H, A):
            want = _stride(head, D, H, A)
            assert stride(D, H, A) == want, (D, H, A)
            assert wrapper(D, H, A) == want
            assert workspace(D, H, A) == 16 + 4 * -(-want // RED_CHUNK), (D, H, A)
        else:
            assert stride(D, H, A) == EUNSUPPORTED, (D, H, A)
            assert b"not instantiated" in lib.trl_last_error()
            assert workspace(D, H, A) == EUNSUPPORTED, (D, H, A)
            with pytest.raises(_C.TrlError, match="not instantiated"):
                wrapper(D, H, A)
    # the benchmark shape is a compile-time instantiation of the Gaussian head: its stride is the template's constant
    assert lib.trl_ppo_partial_stride(17, 64, 6) == 5760 == _stride("gauss", 17, 64, 6)
    assert lib.trl_ppo_reduce_adam_workspace(17, 64, 6) == 16 + 4 * 90


def test_sd_scalar_stride_and_largest_strides(built_lib):
    from torchrl_amd import _C
    lib = _C.lib()
    assert lib.trl_ppo_sd_scalar_stride() == 24 == _C.ppo_sd_scalar_stride()     # 8 of every head + 16 of its own
    assert lib.trl_ppo_sd_partial_stride(17, 64, 8) == 6400 and lib.trl_ppo_sd_partial_stride(32, 64, 8) == 7360
    assert lib.trl_ppo_partial_stride(32, 64, 8) == 6848 and lib.trl_ppo_cat_partial_stride(32, 64, 8) == 6848


def _nets(add_ln):
    import torch
    from torchrl_amd import networks, policies
    net = dict(base_type=networks.MLPBase, hidden_shapes=[8, 8], activation_func=torch.nn.Tanh, add_ln=add_ln)
    return {"gauss": policies.GuassianContPolicyBasicBias(input_shape=4, output_shape=2, **net),
            "cat": policies.CategoricalDisPolicy(input_shape=4, output_shape=3, **net),
            "sd": policies.GuassianContPolicy(input_shape=4, output_shape=4, **net),
            "vf": networks.Net(input_shape=(4,), output_shape=1, **net),
            "det": policies.DetContPolicy(input_shape=4, output_shape=2, **net)}


@pytest.mark.parametrize("add_ln", [False, True])
def test_head_kind(add_ln):
    from torchrl_amd import _C
    from torchrl_amd.algo.on_policy import ppo as ppo_mod
    from torchrl_amd.policies.continuous_policy import HEAD_CAT, HEAD_GAUSS, HEAD_SD, head_kind, is_state_std
    assert len({HEAD_GAUSS, HEAD_CAT, HEAD_SD}) == 3
    nets = _nets(add_ln)
    for name, want in (("gauss", HEAD_GAUSS), ("cat", HEAD_CAT), ("sd", HEAD_SD)):
        assert head_kind(nets[name]) == want, name
        assert head_kind(nets[name], refuse="never raised") == want
        assert (head_kind(nets[name]) == HEAD_SD) == is_state_std(nets[name]) == ppo_mod.is_state_std(nets[name])
    # a value network and a policy without `logstd` / `logits` have none of the heads: None where the caller does not
    # refuse, the caller's own message where it does
    msg = "PPO / A2C kernels need a GuassianContPolicyBasicBias, a GuassianContPolicy or a CategoricalDisPolicy"
    for name in ("vf", "det"):
        assert not is_state_std(nets[name])
        assert head_kind(nets[name]) is None
        with pytest.raises(_C.TrlError, match=msg):
            head_kind(nets[name], refuse=msg)


def test_callers_refuse_with_their_own_message():
    """The engines and the collector word their refusal of a head-less policy as before."""
    import torch
    from torchrl_amd import _C
    from torchrl_amd.algo import PPO
    from torchrl_amd.collector.on_policy import VecOnPolicyCollector
    from oracle.synth_env import SynthVecEnvCPU
    nets = _nets(False)

    class _Stub:
        epoch_frames = 0
    agent = PPO(pf=nets["det"], vf=nets["vf"], tau=0.95, shuffle=True, discount=0.99, num_epochs=10, batch_size=8, gae=True,
                env=SynthVecEnvCPU(4), replay_buffer=None, collector=_Stub(), logger=None, device=torch.device("cpu"),
                save_dir=None)
    with pytest.raises(_C.TrlError, match="PPO / A2C kernels need a GuassianContPolicyBasicBias, a GuassianContPolicy or a "
                                          "CategoricalDisPolicy"):
        agent.engine()
    col = VecOnPolicyCollector.__new__(VecOnPolicyCollector)
    col.pf, col.vf, col.noise_mode = nets["det"], nets["vf"], "device"
    with pytest.raises(_C.TrlError, match="the on-policy collector supports GuassianContPolicyBasicBias"):
        col._check_shapes()
