"""LayerNorm MLPs (`add_ln=True`) on the HIP path: trl_layernorm_fwd_f32 / trl_layernorm_bwd_f32 / trl_act2_*_f32 against
the numpy restatement in float64 (tests/_layernorm_ref.py), Net.forward and the ops tape against torch autograd in float64,
the PPO / A2C engine against the reference fixture (tests/golden/layernorm_update.npz), one whole iteration under
TRL_STRICT=1, and the engines that keep refusing such nets.  Without k_layernorm.hip every test but the last fails."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _layernorm_ref as ref                                                  # noqa: E402
from test_layernorm_cpu import stats_case, stats_case_bound                  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ACTS = {"tanh": 0, "relu": 1, "none": 2}
MS, HS = [1, 7, 64, 300], [1, 3, 24, 64, 100, 256, 1000]


class _Stub:
    epoch_frames = 0


class _Log:
    def __init__(self): self.infos = []
    def add_update_info(self, d): self.infos.append(dict(d))
    def add_epoch_info(self, *a, **k): pass
    def log(self, *a): pass
    def finish(self): pass


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(HERE, "golden", "layernorm_update.npz"))


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV).contiguous()


def offset_like(t):
    """A contiguous device tensor of t's shape whose data pointer is 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
    out = buf[1:].view(t.shape)
    assert out.data_ptr() % 16 == 4
    return out


def xhat_scale(a64, mean, rstd):
    """|xhat| plus the size its float32 absolute error scales with, rstd (|a| + |mean|) (test_backward_kernel_vs_float64)."""
    return np.abs((a64 - mean) * rstd) + rstd * (np.abs(a64) + np.abs(mean))


def kernel_case(M, H, act, seed=0):
    """Activation outputs a = act(N(0, 1)) (what the norm sees in a net), dy ~ N(0, 1), gamma = 1 + 0.3 N, beta = 0.2 N."""
    rs = np.random.RandomState(1000 * M + H + seed)
    z = rs.randn(M, H).astype(np.float32)
    a = ref.act_fn(z, act).astype(np.float32)
    return a, rs.randn(M, H).astype(np.float32), (1 + 0.3 * rs.randn(H)).astype(np.float32), (0.2 * rs.randn(H)).astype(np.float32)


# ---------------------------------------------------------------- 3. forward kernel
@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("M", MS)
def test_forward_kernel_vs_float64(M, H):
    """y: rel 1e-4 / abs 1e-5 (the project's bound for a network output); the row statistics: mean abs 1e-6 + rel 1e-6, rstd
    rel 1e-5 (two fp32 passes over at most 1000 values of size <= 5)."""
    from torchrl_amd import _C
    a, _, gamma, beta = kernel_case(M, H, "tanh" if H % 2 else "relu")
    y, stats = _C.layernorm_fwd(dev(a), dev(gamma), dev(beta))
    torch.cuda.synchronize()
    want, mean, rstd = ref.ln_fwd(a.astype(np.float64), gamma.astype(np.float64), beta.astype(np.float64))
    err = np.abs(y.cpu().numpy() - want)
    print("M=%d H=%d y max abs err %.3e" % (M, H, err.max()))
    assert (err <= 1e-5 + 1e-4 * np.abs(want)).all()
    st = stats.cpu().numpy().astype(np.float64)
    assert (np.abs(st[:, :1] - mean) <= 1e-6 + 1e-6 * np.abs(mean)).all()
    assert (np.abs(st[:, 1:] - rstd) <= 1e-5 * rstd).all()
    if H == 1:
        assert np.array_equal(y.cpu().numpy(), np.broadcast_to(beta, (M, 1)))


@pytest.mark.parametrize("M,H", [(7, 64), (300, 256)])
def test_forward_kernel_unaligned_output(M, H):
    """y 4 bytes past a 16-byte boundary: the 4-byte route (a lane owns other columns there, so the row sums are added in
    another order: the same bounds, not the same bits)."""
    from torchrl_amd import _C
    a, _, gamma, beta = kernel_case(M, H, "tanh")
    a_d, g_d, b_d = dev(a), dev(gamma), dev(beta)
    y0, st0 = _C.layernorm_fwd(a_d, g_d, b_d)
    y1, st1 = _C.layernorm_fwd(a_d, g_d, b_d, y=offset_like(y0))
    assert y1.data_ptr() % 16 == 4 and y0.data_ptr() % 16 == 0
    np.testing.assert_allclose(st1.cpu().numpy(), st0.cpu().numpy(), rtol=1e-5, atol=1e-6)
    want = ref.ln_fwd(a.astype(np.float64), gamma.astype(np.float64), beta.astype(np.float64))[0]
    for y in (y0, y1):
        assert (np.abs(y.cpu().numpy() - want) <= 1e-5 + 1e-4 * np.abs(want)).all()


def test_forward_kernel_statistics_case():
    """Rows of mean 100, std 0.5: the bound is 4 x the float32 two-pass restatement's own error (tests/test_layernorm_cpu.py
    shows that E[x^2] - mean^2 in float32 misses it by two orders of magnitude)."""
    from torchrl_amd import _C
    a, gamma, beta = stats_case()
    bound, y64 = stats_case_bound()
    y, _ = _C.layernorm_fwd(dev(a), dev(gamma), dev(beta))
    err = float(np.abs(y.cpu().numpy() - y64).max())
    print("statistics case: kernel error %.3e, bound %.3e" % (err, bound))
    assert err <= bound


def test_widths_past_1024_raise():
    from torchrl_amd import _C
    lib = _C.lib()
    assert lib.trl_layernorm_supported(1) and lib.trl_layernorm_supported(1024)
    assert not lib.trl_layernorm_supported(1025) and not lib.trl_layernorm_supported(0)
    a = torch.zeros(4, 1025, device=DEV)
    v = torch.zeros(1025, device=DEV)
    with pytest.raises(_C.TrlError, match="1024"):
        _C.layernorm_fwd(a, v, v)
    with pytest.raises(_C.TrlError, match="1024"):
        _C.layernorm_bwd(a, a, torch.zeros(4, 2, device=DEV), v, 0, v.clone(), v.clone())
    assert lib.trl_layernorm_fwd_f32(a.data_ptr(), v.data_ptr(), v.data_ptr(), a.data_ptr(), v.data_ptr(), 4, 1025, None) != 0
    assert "1024" in lib.trl_last_error().decode()
    assert lib.trl_layernorm_bwd_workspace(4, 1025) < 0


# ---------------------------------------------------------------- 4. backward kernel
@pytest.mark.parametrize("act", ["tanh", "relu"])
@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("M", MS)
def test_backward_kernel_vs_float64(M, H, act):
    """dz, dgamma, dbeta against float64 on the same float32 inputs, with the kernel's own forward statistics.

    Bounds, from the float32 arithmetic: dz = rstd (g - m1 - xhat m2) act'(a) -- three terms of size up to
    G (1 + |xhat|) with G = max_row |g|, each carrying a few roundings (6e-8 relative) and the row means a wave-tree sum of
    H <= 1000 terms: absolute error below 1e-6 rstd G (1 + |xhat|); the test allows ten times that, plus rel 1e-4.
    dgamma / dbeta are sums over M <= 300 rows (one row per sub-group of lanes, 4 or 16 sub-groups per workgroup, up to 75
    slabs added as sixteen interleaved runs): at most ~40 sequential additions, so 40 x 6e-8 = 2.4e-6 of the column's sum of
    absolute terms, plus the terms' own error.  A term dy xhat carries xhat's ABSOLUTE error: xhat = (a - mean) rstd with a mean that is a fp32 sum of H values
    (error up to ~1e-6 |mean|) and a subtraction that cancels where a is near the mean, so xhat is off by up to
    ~1e-6 rstd (|a| + |mean|) however small xhat itself is (`xhat_scale` below adds that to |xhat|).  Hence
    abs 1e-5 x sum_rows |dy| xhat_scale for dgamma and abs 1e-5 x sum_rows |dy| for dbeta, plus rel 1e-4.
    M = 300 is 75 workgroups of four rows (19 of sixteen rows for H <= 64, where a wave takes four rows) -- the fewest rows
    per workgroup the kernel uses -- so 75 (19) slabs are folded; two calls give the same bits."""
    from torchrl_amd import _C
    a, dy, gamma, beta = kernel_case(M, H, act, seed=5)
    a_d, dy_d, g_d = dev(a), dev(dy), dev(gamma)
    _, stats = _C.layernorm_fwd(a_d, g_d, dev(beta))
    dg, db = torch.zeros(H, device=DEV), torch.zeros(H, device=DEV)
    dz = _C.layernorm_bwd(dy_d, a_d, stats, g_d, ACTS[act], dg, db)
    dg2, db2 = torch.full((H,), 7.0, device=DEV), torch.full((H,), 7.0, device=DEV)
    dz2 = _C.layernorm_bwd(dy_d, a_d, stats, g_d, ACTS[act], dg2, db2)
    torch.cuda.synchronize()
    assert torch.equal(dg, dg2) and torch.equal(db, db2) and torch.equal(dz, dz2)
    assert _C.lib().trl_layernorm_bwd_workspace(M, H) == -(-M // (16 if H <= 64 else 4)) * 2 * H     # one slab per workgroup
    a64, dy64, g64 = a.astype(np.float64), dy.astype(np.float64), gamma.astype(np.float64)
    mean, rstd = ref.ln_stats(a64)
    w_dz, w_dg, w_db = ref.ln_bwd(dy64, a64, mean, rstd, g64, act)
    xhat = (a64 - mean) * rstd
    G = np.abs(dy64 * g64).max(axis=1, keepdims=True)
    err = np.abs(dz.cpu().numpy() - w_dz)
    tol = 1e-4 * np.abs(w_dz) + 1e-5 * rstd * G * (1 + np.abs(xhat))
    print("M=%d H=%d %s dz max abs err %.3e, worst err / bound %.3f" % (M, H, act, err.max(), (err / np.maximum(tol, 1e-30)).max()))
    assert (err <= tol).all()
    for name, got, want, l1 in (("dgamma", dg, w_dg, (np.abs(dy64) * xhat_scale(a64, mean, rstd)).sum(axis=0)),
                                 ("dbeta", db, w_db, np.abs(dy64).sum(axis=0))):
        e = np.abs(got.cpu().numpy() - want)
        t = 1e-4 * np.abs(want) + 1e-5 * l1
        print("  %s max abs err %.3e, worst err / bound %.3f" % (name, e.max(), (e / np.maximum(t, 1e-30)).max()))
        assert (e <= t).all(), name
    if H == 1:
        assert bool((dz == 0).all()) and float(dg[0]) == 0.0


@pytest.mark.parametrize("M,H", [(33000, 24), (8300, 100)])
def test_kernels_with_several_rows_per_wave(M, H):
    """Past the rows one grid takes at a time -- the forward's 2048 workgroups x 16 (H <= 64) or 4 rows, the backward's 1024:
    waves walk several row blocks, add them into their dgamma / dbeta registers, and 1024 slabs are folded.  dz and y as
    above; the column sums see up to 9 + 16 + 64 + 16 additions in sequence (105 x 6e-8 = 6.3e-6 of the sum of absolute
    terms) beside the terms' own error: abs 2e-5 x sum_rows |term|."""
    from torchrl_amd import _C
    a, dy, gamma, beta = kernel_case(M, H, "tanh", seed=11)
    a_d, dy_d, g_d = dev(a), dev(dy), dev(gamma)
    y, stats = _C.layernorm_fwd(a_d, g_d, dev(beta))
    assert _C.lib().trl_layernorm_bwd_workspace(M, H) == 1024 * 2 * H
    outs = []
    for _ in range(2):
        dg, db = torch.zeros(H, device=DEV), torch.zeros(H, device=DEV)
        outs.append((_C.layernorm_bwd(dy_d, a_d, stats, g_d, ACTS["tanh"], dg, db), dg, db))
    assert all(torch.equal(p, q) for p, q in zip(*outs))
    a64, dy64, g64 = a.astype(np.float64), dy.astype(np.float64), gamma.astype(np.float64)
    want_y, mean, rstd = ref.ln_fwd(a64, g64, beta.astype(np.float64))
    assert (np.abs(y.cpu().numpy() - want_y) <= 1e-5 + 1e-4 * np.abs(want_y)).all()
    w_dz, w_dg, w_db = ref.ln_bwd(dy64, a64, mean, rstd, g64, "tanh")
    xhat = (a64 - mean) * rstd
    tol = 1e-4 * np.abs(w_dz) + 1e-5 * rstd * np.abs(dy64 * g64).max(axis=1, keepdims=True) * (1 + np.abs(xhat))
    dz, dg, db = outs[0]
    assert (np.abs(dz.cpu().numpy() - w_dz) <= tol).all()
    for name, got, want, l1 in (("dgamma", dg, w_dg, (np.abs(dy64) * xhat_scale(a64, mean, rstd)).sum(axis=0)),
                                 ("dbeta", db, w_db, np.abs(dy64).sum(axis=0))):
        e = np.abs(got.cpu().numpy() - want)
        print("M=%d H=%d %s max abs err %.3e, worst err / bound %.3f" % (M, H, name, e.max(), (e / (1e-4 * np.abs(want) + 2e-5 * l1)).max()))
        assert (e <= 1e-4 * np.abs(want) + 2e-5 * l1).all(), name


def test_backward_kernel_unaligned_and_ungated():
    """dz 4 bytes past a 16-byte boundary (the 4-byte route) meets the bound of the aligned call; TRL_ACT_NONE leaves da
    ungated.  Bound as in test_backward_kernel_vs_float64, with |xhat| <= 8 = sqrt(H) and G <= 6."""
    from torchrl_amd import _C
    M, H = 64, 64
    a, dy, gamma, beta = kernel_case(M, H, "tanh", seed=9)
    a_d, dy_d, g_d = dev(a), dev(dy), dev(gamma)
    _, stats = _C.layernorm_fwd(a_d, g_d, dev(beta))
    outs = []
    for dz in (None, offset_like(a_d)):
        dg, db = torch.zeros(H, device=DEV), torch.zeros(H, device=DEV)
        outs.append((_C.layernorm_bwd(dy_d, a_d, stats, g_d, ACTS["none"], dg, db, dz=dz), dg, db))
    a64, dy64, g64 = a.astype(np.float64), dy.astype(np.float64), gamma.astype(np.float64)
    mean, rstd = ref.ln_stats(a64)
    want, w_dg, w_db = ref.ln_bwd(dy64, a64, mean, rstd, g64, "none")
    xhat = (a64 - mean) * rstd
    tol = 1e-4 * np.abs(want) + 1e-5 * rstd * np.abs(dy64 * g64).max(axis=1, keepdims=True) * (1 + np.abs(xhat))
    for dz, dg, db in outs:
        assert (np.abs(dz.cpu().numpy() - want) <= tol).all()
        assert (np.abs(dg.cpu().numpy() - w_dg) <= 1e-4 * np.abs(w_dg) +
                1e-5 * (np.abs(dy64) * xhat_scale(a64, mean, rstd)).sum(axis=0)).all()
        assert (np.abs(db.cpu().numpy() - w_db) <= 1e-4 * np.abs(w_db) + 1e-5 * np.abs(dy64).sum(axis=0)).all()


@pytest.mark.parametrize("n,offset", [(1, False), (5, False), (7000, False), (7000, True), (4096, False)])
def test_second_tanh_forward_and_backward(n, offset):
    """t2 = tanh(t1): the kernels' tanh has an absolute error below 2e-7 (csrc/trl_mlp.h), so abs 3e-7.  The backward is
    three multiplications of the STORED t1, t2: rel 1e-6 + abs 1e-7 against float64 on the same stored values.  A second
    ReLU is the identity: the forward returns its input's values, the backward gates once."""
    from torchrl_amd import _C
    rs = np.random.RandomState(n)
    t1 = np.tanh(rs.randn(n)).astype(np.float32)
    d = rs.randn(n).astype(np.float32)
    t1_d = dev(t1)
    out = offset_like(t1_d) if offset else None
    t2 = _C.act2_fwd(t1_d, ACTS["tanh"], out=out)
    assert (np.abs(t2.cpu().numpy() - np.tanh(t1.astype(np.float64))) <= 3e-7).all()
    dz = _C.act2_bwd(dev(d), t1_d, t2, ACTS["tanh"], out=offset_like(t1_d) if offset else None)
    want = ref.act2_bwd(d.astype(np.float64), t1.astype(np.float64), t2.cpu().numpy().astype(np.float64), "tanh")
    assert (np.abs(dz.cpu().numpy() - want) <= 1e-7 + 1e-6 * np.abs(want)).all()
    r1 = dev(np.maximum(rs.randn(n), 0).astype(np.float32))
    assert torch.equal(_C.act2_fwd(r1, ACTS["relu"]), r1)
    assert torch.equal(_C.act2_bwd(dev(d), r1, r1, ACTS["relu"]), dev(d) * (r1 > 0))


# ---------------------------------------------------------------- 5. network and tape against autograd
def repo_nets(g, tag, prefix_pf="_pf0_", prefix_vf="_vf0_"):
    """The repo's policy / value net of a fixture case, with the fixture's parameters loaded."""
    from torchrl_amd import networks, policies
    kind, act, hidden, append = ref.STRUCT[tag]
    D, A, B, tanh = (int(x) for x in g[tag + "_args"])
    net = dict(hidden_shapes=list(hidden), append_hidden_shapes=list(append), base_type=networks.MLPBase,
               activation_func={"tanh": torch.nn.Tanh, "relu": torch.nn.ReLU}[act], add_ln=True)
    if kind == "bb":
        pf = policies.GuassianContPolicyBasicBias(input_shape=D, output_shape=A, tanh_action=bool(tanh), **net)
    elif kind == "sd":
        pf = policies.GuassianContPolicy(input_shape=D, output_shape=2 * A, tanh_action=bool(tanh), **net)
    else:
        pf = policies.CategoricalDisPolicy(input_shape=D, output_shape=A, **net)
    vf = networks.Net(input_shape=(D,), output_shape=1, **net)
    for mod, prefix in ((pf, tag + prefix_pf), (vf, tag + prefix_vf)):
        mod.load_state_dict(state_of(g, prefix))
    return pf, vf


def state_of(g, prefix):
    return {k[len(prefix):].replace("__", "."): torch.from_numpy(g[k].copy()) for k in g.files if k.startswith(prefix)}


@pytest.mark.parametrize("tag", ref.TAGS)
def test_net_forward_and_tape_vs_autograd_in_float64(g, tag, monkeypatch):
    """Net.forward (kernels only, also under TRL_STRICT=1) and ops.mlp_forward / mlp_backward of the policy network of each
    fixture structure against torch autograd in float64 on the CPU: the output rel 1e-4 / abs 1e-5; every parameter's
    gradient, gamma / beta included, within rel 1e-4 of the element plus 1e-5 of the tensor's largest gradient (fp32 GEMM
    reductions over B <= 96 rows: 96 x 6e-8 = 6e-6 of the largest terms)."""
    from torchrl_amd import _C, networks, ops
    monkeypatch.setenv("TRL_STRICT", "1")
    pf, _ = repo_nets(g, tag)
    obs = g[tag + "_batch_obs"]
    cpu = repo_nets(g, tag)[0].double()
    x64 = torch.from_numpy(obs).double()
    out64 = networks.Net.forward(cpu, x64)
    rs = np.random.RandomState(4)
    d_out = rs.randn(*out64.shape).astype(np.float32)
    out64.backward(torch.from_numpy(d_out).double())
    pf.to(DEV)
    before = _C.eager_fallback_count()
    with torch.no_grad():
        y = networks.Net.forward(pf, dev(obs))
    layers, code = ops.net_layers(pf)
    assert ops.has_post(layers)
    y2, tape = ops.mlp_forward(layers, dev(obs), code)
    assert torch.equal(y, y2)
    grads = [torch.zeros_like(p) for p in ops.plan_params(layers)]
    views, it = [], iter(grads)
    for l in layers:
        views.append(tuple(next(it) for _ in ops.plan_params([l])))
    dx = ops.mlp_backward(tape, dev(d_out), grads=views, need_input=True)
    torch.cuda.synchronize()
    assert _C.eager_fallback_count() == before
    want = out64.detach().numpy()
    assert (np.abs(y.cpu().numpy() - want) <= 1e-5 + 1e-4 * np.abs(want)).all()
    names = dict((id(p), n) for n, p in pf.named_parameters())
    ref_grads = dict(cpu.named_parameters())
    for p, got in zip(ops.plan_params(layers), grads):
        w = ref_grads[names[id(p)]].grad.numpy()
        e = np.abs(got.cpu().numpy() - w)
        print("%s %s grad max abs err %.3e (max |grad| %.3e)" % (tag, names[id(p)], e.max(), np.abs(w).max()))
        assert (e <= 1e-4 * np.abs(w) + 1e-5 * np.abs(w).max()).all(), names[id(p)]
    assert dx.shape == (obs.shape[0], obs.shape[1]) and torch.isfinite(dx).all()
    assert len(tape.stats) == len(layers) and sum(s is not None for s in tape.stats) == 1 + len(ref.STRUCT[tag][3])


# ---------------------------------------------------------------- 6. updates against the fixture
def fixture_agent(g, tag, algo_cls, **kw):
    from torchrl_amd.env.synth import SynthVecEnv
    D, A, B, tanh = (int(x) for x in g[tag + "_args"])
    pf, vf = repo_nets(g, tag)
    agent = algo_cls(pf=pf, vf=vf, tau=0.95, shuffle=True, discount=0.99, num_epochs=10, batch_size=B, gae=True,
                     env=SynthVecEnv(4, obs_dim=D, act_dim=A, device=DEV, discrete=ref.STRUCT[tag][0] == "cat"),
                     replay_buffer=None, collector=_Stub(), logger=_Log(), device=DEV, save_dir=None, **kw)
    return pf, vf, agent


def param_error(mod, g, prefix):
    return max(float((p.detach().cpu().double() - torch.from_numpy(g[prefix + k.replace(".", "__")]).double()).abs().max())
               for k, p in mod.state_dict().items())


def assert_info(info, g, prefix):
    want = ref.info_of(g, prefix)
    assert sorted(info) == sorted(want)
    bad = []
    for k in sorted(want):
        print("%s %s got %.9g want %.9g (err %.3e, bound %.3e)" % (prefix, k, info[k], want[k], abs(info[k] - want[k]),
                                                                     1e-5 + 1e-4 * abs(want[k])))
        if not info[k] == pytest.approx(want[k], rel=1e-4, abs=1e-5):
            bad.append(k)
    assert not bad, bad


@pytest.mark.parametrize("tag", ref.TAGS)
def test_policy_outputs_vs_fixture(g, tag, monkeypatch):
    """update / eval_act / explore of the three policies and the value net on the GPU, kernels only (TRL_STRICT=1), against
    the reference's outputs: rel 1e-4 / abs 1e-5 (the float32 restatement is within 9e-7, profiles/NOTES_layernorm.md)."""
    from torchrl_amd import _C
    monkeypatch.setenv("TRL_STRICT", "1")
    kind = ref.STRUCT[tag][0]
    pf, vf = repo_nets(g, tag)
    pf.to(DEV), vf.to(DEV)
    obs, acts = dev(g[tag + "_batch_obs"]), dev(g[tag + "_batch_acts"])
    before = _C.eager_fallback_count()
    with torch.no_grad():
        out = pf.update(obs, acts)
        ev = pf.eval_act(obs)
        v = vf(obs)
        if kind != "bb":                                                   # (the basic-bias policy samples through torch.distributions)
            ex = pf.explore(obs, return_log_probs=True)
            assert torch.isfinite(ex["action"]).all()
    assert _C.eager_fallback_count() == before
    cmp = lambda got, want, name: np.testing.assert_allclose(np.asarray(got).reshape(want.shape), want, rtol=1e-4, atol=1e-5,
                                                              err_msg=name)
    cmp(v.cpu().numpy(), g[tag + "_v0"], "v")
    cmp(out["log_prob"].cpu().numpy(), g[tag + "_upd_log_prob"], "log_prob")
    cmp(out["ent"].cpu().numpy(), g[tag + "_upd_ent"], "ent")
    if kind == "cat":
        cmp(out["dis"].cpu().numpy(), g[tag + "_probs"], "probs")
        assert np.array_equal(np.asarray(ev).reshape(-1), g[tag + "_eval_act"].reshape(-1))
    else:
        cmp(out["mean"].cpu().numpy(), g[tag + "_upd_mean"], "mean")
        cmp(out["log_std"].cpu().numpy(), g[tag + "_upd_log_std"], "log_std")
        cmp(ev, g[tag + "_eval_act"], "eval_act")


@pytest.mark.parametrize("tag", ref.TAGS)
def test_a2c_update_vs_fixture(g, tag, errlog):
    """Scalars rel 1e-4 / abs 1e-5, post-step parameters abs 1e-6, every key of the state dict --
    gamma / beta included.  The engine is the generic one and its policy block is ALL of pf.parameters()."""
    from torchrl_amd.algo import A2C
    pf, vf, agent = fixture_agent(g, tag, A2C, plr=3e-4, vlr=1e-3, entropy_coeff=0.01)
    info = agent.update(ref.batch_of(g, tag))
    eng = agent.engine()
    assert type(eng).__name__ == "_GenericPPO"
    assert eng.P_pf == sum(p.numel() for p in pf.parameters()) and eng.P_vf == sum(p.numel() for p in vf.parameters())
    errs = {name: param_error(mod, g, f"{tag}_a2c_{name}1_") for name, mod in (("pf", pf), ("vf", vf))}
    for name, err in errs.items():
        errlog("a2c_%s_%s" % (tag, name), err, 1e-6)
        print("a2c %s %s parameter error %.3e" % (tag, name, err))
    assert_info(info, g, f"{tag}_a2c_info")
    assert all(e <= 1e-6 for e in errs.values()), errs


@pytest.mark.parametrize("tag", ref.TAGS)
def test_ppo_chain_vs_fixture(g, tag, errlog):
    """Four chained PPO.update calls, the third with the clipped value loss; the same bounds for every update."""
    from torchrl_amd.algo import PPO
    pf, vf, agent = fixture_agent(g, tag, PPO, plr=3e-4, vlr=3e-4, clip_para=0.2, opt_epochs=2, entropy_coeff=0.005)
    agent.current_epoch = 3
    agent.target_pf.load_state_dict(state_of(g, f"{tag}_ppo_tpf0_"))
    worst, bad = {}, []
    for s, clipv in enumerate(g[f"{tag}_ppo_clipv"]):
        agent.clipped_value_loss = bool(clipv)
        info = agent.update(ref.batch_of(g, tag))
        for name, mod in (("pf", pf), ("vf", vf)):
            err = param_error(mod, g, f"{tag}_ppo_{name}{s + 1}_")
            errlog("ppo_%s_update%d_%s" % (tag, s, name), err, 1e-6)
            print("ppo %s update %d %s parameter error %.3e" % (tag, s, name, err))
            worst[(s, name)] = err
        try:
            assert_info(info, g, f"{tag}_ppo_info{s}")
        except AssertionError as exc:
            bad.append((s, str(exc)))
    assert not bad, bad
    assert all(e <= 1e-6 for e in worst.values()), worst
    eng = agent.engine()
    assert type(eng).__name__ == "_GenericPPO" and eng.P_pf == sum(p.numel() for p in pf.parameters())
    assert eng.target_flat.numel() == eng.P_pf
    # the target's LayerNorm parameters live in its flat copy: sync_target_pf moves them with everything else
    eng.sync_target_pf()
    for (k, a), b in zip(pf.state_dict().items(), agent.target_pf.state_dict().values()):
        assert torch.equal(a, b), k


def test_policy_and_value_net_need_not_agree_on_add_ln(g):
    """A LayerNorm policy beside a plain value net of the same activation runs; two activations do not."""
    from torchrl_amd import _C, networks
    from torchrl_amd.algo import A2C
    from torchrl_amd.env.synth import SynthVecEnv
    tag = "bb_tanh"
    D, A, B, tanh = (int(x) for x in g[tag + "_args"])
    pf, _ = repo_nets(g, tag)
    mk = lambda act: networks.Net(input_shape=(D,), output_shape=1, hidden_shapes=[16, 16], append_hidden_shapes=[],
                                  base_type=networks.MLPBase, activation_func=act)
    kw = dict(tau=0.95, shuffle=True, discount=0.99, num_epochs=10, batch_size=B, gae=True,
              env=SynthVecEnv(4, obs_dim=D, act_dim=A, device=DEV), replay_buffer=None, collector=_Stub(), logger=_Log(),
              device=DEV, save_dir=None, plr=3e-4, vlr=1e-3, entropy_coeff=0.01)
    agent = A2C(pf=pf, vf=mk(torch.nn.Tanh), **kw)
    info = agent.update(ref.batch_of(g, tag))
    assert all(np.isfinite(v) for v in info.values())
    with pytest.raises(_C.TrlError, match="same activation"):
        A2C(pf=repo_nets(g, tag)[0], vf=mk(torch.nn.ReLU), **kw).engine()


# ---------------------------------------------------------------- 7. one whole iteration
def make_collector(N, T, horizon, seed=3, hidden=(24, 40), append=(20,)):
    from torchrl_amd import networks, policies
    from torchrl_amd.collector.on_policy import VecOnPolicyCollector
    from torchrl_amd.env import get_vec_env
    from torchrl_amd.replay_buffers.on_policy import OnPolicyReplayBuffer
    torch.manual_seed(0)
    net = dict(hidden_shapes=list(hidden), append_hidden_shapes=list(append), base_type=networks.MLPBase,
               activation_func=torch.nn.Tanh, add_ln=True)
    pf = policies.GuassianContPolicyBasicBias(input_shape=17, output_shape=6, tanh_action=True, **net)
    vf = networks.Net(input_shape=(17,), output_shape=1, **net)
    rs = np.random.RandomState(1)
    with torch.no_grad():
        for m in list(pf.modules()) + list(vf.modules()):
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.copy_(torch.from_numpy((1 + 0.3 * rs.randn(*m.weight.shape)).astype(np.float32)))
                m.bias.copy_(torch.from_numpy((0.2 * rs.randn(*m.bias.shape)).astype(np.float32)))
    env, eval_env = (get_vec_env("SynthHalfCheetah-v0", {"reward_scale": 1, "obs_norm": False}, N, device=DEV) for _ in range(2))
    for e in (env, eval_env):
        e.horizon = horizon
    env.seed(seed)
    buf = OnPolicyReplayBuffer(N * T, env_nums=N, time_limit_filter=True)
    col = VecOnPolicyCollector(vf, env=env, eval_env=eval_env, pf=pf, replay_buffer=buf, device=DEV, train_render=False,
                               epoch_frames=N * T, max_episode_frames=999, eval_episodes=1, noise_mode="device")
    return pf, vf, env, buf, col


def ppo_agent(pf, vf, env, buf, col, logger, B, save_dir=None):
    from torchrl_amd.algo import PPO
    return PPO(pf=pf, vf=vf, plr=3e-4, vlr=3e-4, clip_para=0.2, opt_epochs=2, tau=0.95, shuffle=True, entropy_coeff=0.005,
               discount=0.99, num_epochs=10, batch_size=B, gae=True, env=env, replay_buffer=buf, collector=col, logger=logger,
               device=DEV, save_dir=save_dir)


def ln_params(mod):
    return [p for m in mod.modules() if isinstance(m, torch.nn.LayerNorm) for p in (m.weight, m.bias)]


def test_one_ppo_iteration_under_strict_and_snapshot(monkeypatch, tmp_path):
    """N = 8, T = 16, B = 64, two passes, TRL_STRICT=1: collection, evaluation and the updates stay on the kernels; the first
    minibatch meets the policy that collected it (ratio 1 to rounding: the forward runs on N rows there and on B here);
    every LayerNorm parameter moves; a snapshot round-trips them."""
    from torchrl_amd import _C
    monkeypatch.setenv("TRL_STRICT", "1")
    N, T = 8, 16
    np.random.seed(4)
    pf, vf, env, buf, col = make_collector(N, T, horizon=9, seed=2)
    assert col._spec is None and pf.mlp2_spec() is None and vf.mlp2_spec() is None
    logger = _Log()
    agent = ppo_agent(pf, vf, env, buf, col, logger, 64)
    before_ln = [p.detach().clone() for p in ln_params(pf) + ln_params(vf)]
    count = _C.eager_fallback_count()
    col.train_one_epoch()
    agent.current_epoch = 0
    agent.update_per_epoch()
    ev = col.eval_one_epoch()
    torch.cuda.synchronize()
    assert _C.eager_fallback_count() == count
    assert len(ev["eval_rewards"]) == N
    assert len(logger.infos) == 2 * (N * T // 64)
    assert logger.infos[0]["ratio/max"] == pytest.approx(1.0, abs=1e-5) and logger.infos[0]["ratio/min"] == pytest.approx(1.0, abs=1e-5)
    assert all(np.isfinite(list(i.values())).all() for i in logger.infos)
    assert len(before_ln) == 8
    for b, p in zip(before_ln, ln_params(pf) + ln_params(vf)):
        assert torch.isfinite(p).all() and not torch.equal(b, p)
    assert type(agent.engine()).__name__ == "_GenericPPO"
    agent.snapshot(str(tmp_path), 0)
    pf2, vf2, *_ = make_collector(N, T, horizon=9, seed=2)
    for name, src, dst in (("pf", pf, pf2), ("vf", vf, vf2)):
        state = torch.load(os.path.join(str(tmp_path), "model_%s_0.pth" % name), map_location="cpu")
        assert sorted(state) == sorted(src.state_dict())
        dst.load_state_dict(state)
        for (k, a), b in zip(src.state_dict().items(), dst.state_dict().values()):
            assert torch.equal(a.cpu(), b.cpu()), k
        assert sum(k.endswith(".2.weight") for k in state) == 2             # the two LayerNorms' gamma


def test_ppo_epochs_replayed_from_graphs_equal_eager(monkeypatch):
    """train_one_epoch + update_per_epoch, three visits: the third replays the captured rollout and update graphs and leaves
    the parameters of the run that never captured, bit for bit (the dgamma / dbeta folds have a fixed order)."""
    N, T = 8, 16
    finals = []
    for no_graph in ("1", "0"):
        monkeypatch.setenv("TRL_NO_GRAPH", no_graph)
        np.random.seed(4)
        pf, vf, env, buf, col = make_collector(N, T, horizon=9, seed=2)
        logger = _Log()
        agent = ppo_agent(pf, vf, env, buf, col, logger, 64)
        per_epoch = []
        for epoch in range(3):
            res = col.train_one_epoch()
            agent.current_epoch = epoch
            agent.update_per_epoch()
            per_epoch.append((float(res["train_epoch_reward"]),
                              torch.cat([p.detach().reshape(-1) for p in list(pf.parameters()) + list(vf.parameters())]).clone()))
        assert all(np.isfinite(list(i.values())).all() for i in logger.infos)
        if no_graph == "0":
            assert len(agent.engine()._graphs) > 0
        finals.append(per_epoch)
    for (r0, p0), (r1, p1) in zip(*finals):
        assert r0 == r1 and torch.equal(p0, p1)
    assert not torch.equal(finals[0][0][1], finals[0][2][1])


# ---------------------------------------------------------------- 8. the other engines still refuse
def test_other_engines_refuse_layernorm_nets():
    """TRPO, V-MPO, TwinSACQ, DDPG and DQN on an MLP walk the plain layer lists (ops.linear_layers / ops.act_code): they
    refuse an `add_ln` net with the dense kernels' LayerNorm message instead of skipping the norms."""
    from torchrl_amd import _C, networks, policies
    from torchrl_amd.algo import DDPG, DQN, TRPO, TwinSACQ, VMPO
    from torchrl_amd.env.synth import SynthVecEnv
    D, A = 17, 6
    net = dict(hidden_shapes=[16, 16], append_hidden_shapes=[], base_type=networks.MLPBase, activation_func=torch.nn.ReLU,
               add_ln=True)
    env = SynthVecEnv(4, device=DEV)
    on = dict(tau=0.95, shuffle=True, discount=0.99, num_epochs=10, batch_size=8, gae=True, env=env, replay_buffer=None,
              collector=_Stub(), logger=_Log(), device=DEV, save_dir=None)
    off = dict(env=env, replay_buffer=None, collector=_Stub(), logger=_Log(), discount=0.99, num_epochs=10, batch_size=8,
               device=DEV, save_dir=None, tau=0.005, use_soft_update=True, opt_times=1)
    bb = lambda: policies.GuassianContPolicyBasicBias(input_shape=D, output_shape=A, tanh_action=True, **net)
    vf = lambda: networks.Net(input_shape=(D,), output_shape=1, **net)
    q = lambda: networks.QNet(input_shape=D + A, output_shape=1, **net)
    builders = {
        "TRPO": lambda: TRPO(max_kl=0.01, cg_damping=0.1, v_opt_times=1, cg_iters=10, residual_tol=1e-10, pf=bb(), vf=vf(),
                             plr=3e-4, vlr=3e-4, **on),
        "VMPO": lambda: VMPO(pf=bb(), vf=vf(), plr=3e-4, vlr=3e-4, **on),
        "TwinSACQ": lambda: TwinSACQ(pf=policies.GuassianContPolicy(input_shape=D, output_shape=2 * A, tanh_action=True, **net),
                                     qf1=q(), qf2=q(), plr=3e-4, qlr=3e-4, policy_std_reg_weight=0, policy_mean_reg_weight=0,
                                     reparameterization=True, automatic_entropy_tuning=True, **off),
        "DDPG": lambda: DDPG(pf=policies.DetContPolicy(input_shape=D, output_shape=A, tanh_action=True, **net), qf=q(),
                             plr=3e-4, qlr=1e-3, **off),
    }

    def dqn():
        qf = networks.Net(input_shape=(D,), output_shape=A, **net)
        pf = policies.EpsilonGreedyDQNDiscretePolicy(qf=qf, start_epsilon=1, end_epsilon=0.1, decay_frames=1000, action_shape=A)
        return DQN(qf=qf, pf=pf, qlr=2.5e-4, **off)
    builders["DQN"] = dqn
    for name, build in builders.items():
        with pytest.raises(_C.TrlError, match="LayerNorm"):
            build().engine()
