"""TRL_LOSS_REINFORCE, the policy half of TRL_LOSS_A2C without a critic, called through torchrl_amd._C:

  * the three stand-alone loss kernels (trl_ppo_generic_losses_f32, trl_cat_losses_f32, trl_gauss_sd_losses_f32) with all
    four value pointers NULL: against the float64 restatements of tests/_gauss_ref.py, _categorical_ref.py and
    _gauss_sd_ref.py at the bounds their own tests use, bit-equal to an A2C-mode call on the same policy inputs, info slots
    7 and 12..15 exactly 0;
  * the fused gradient launch (trl_ppo_*minibatch_grad_f32) all-policy with rets / old_values / old_logp / vf_params NULL:
    partial-gradient and scalar rows bit-equal to the A2C-mode all-policy launch, and after the policy's fold + clip + Adam
    (trl_ppo_*reduce_adam_net_f32, ONE optimiser group, eps 1e-8) the parameters against a float64 step on float64 autograd
    gradients within the project's 1e-6 on post-step parameters."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _categorical_ref as cat_ref                                            # noqa: E402
import _categorical_update_cases as cu                                        # noqa: E402
import _gauss_ref as gr                                                       # noqa: E402
import _gauss_sd_ref as sd_ref                                                # noqa: E402
import _gauss_sd_update_cases as su                                           # noqa: E402
import _ppo_update_cases as pc                                                # noqa: E402
import _ppo_update_ref as pref                                                # noqa: E402
import _reinforce_ref as R                                                    # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F64 = torch.float64
H = 64
CLIP, C_ENT = 0.2, 0.01
BATCHES = (2, 256, 257, 513)                                                  # the smallest legal n_global, one to three blocks
FILL = -777.25                                                                # pre-fill of every output buffer


def dev(x, dtype=None):
    if x is None:
        return None
    t = torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x)
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


def host(t):
    return t.detach().cpu().double()


def check_modes(reinforce, a2c, grad_keys):
    """The new mode against an A2C-mode call on the same policy inputs: the gradients and the policy's info slots bit for
    bit, the value slots exactly 0."""
    for k in grad_keys:
        assert torch.equal(reinforce[k], a2c[k]), k
    for k in R.POLICY_SLOTS:
        a, b = reinforce["info"][k], a2c["info"][k]
        assert a == b or (np.isnan(a) and np.isnan(b)), (k, a, b)
    assert all(reinforce["info"][k] == 0.0 for k in R.VALUE_SLOTS), reinforce["info"]
    assert any(a2c["info"][k] != 0.0 for k in R.VALUE_SLOTS)
    assert reinforce["d_v"] is None


# ================================================================== 1. the shared-std Gaussian loss kernel
def gauss_losses(c, tanh, mode):
    from torchrl_amd import _C
    A = c["mean"].shape[1]
    critic = mode != R.LOSS_REINFORCE
    d_logstd = torch.full((A,), FILL, dtype=torch.float32, device=DEV)
    info = torch.full((24,), FILL, dtype=F64, device=DEV)
    d_mean, d_v = _C.ppo_generic_losses(dev(c["mean"]), dev(c["logstd"]), dev(c["acts"]), dev(c["advs"]), None,
                                        dev(c["v"]) if critic else None, dev(c["rets"]) if critic else None, None,
                                        dev(c["adv_raw"]), c["n_global"], CLIP, C_ENT, False, tanh, mode, d_logstd, info)
    torch.cuda.synchronize()
    return dict(d_mean=host(d_mean), d_logstd=host(d_logstd), d_v=d_v, info=info.cpu().numpy())


@pytest.mark.parametrize("tanh", [True, False])
@pytest.mark.parametrize("A", [1, 6, 64])
@pytest.mark.parametrize("B,n_mult", [(B, 1) for B in BATCHES] + [(257, 3)])
def test_gauss_losses(B, n_mult, A, tanh):
    c = gr.loss_case(B, A, tanh, 4000 + 7 * A + B + 100000 * n_mult, n_mult)
    got, a2c = gauss_losses(c, tanh, R.LOSS_REINFORCE), gauss_losses(c, tanh, R.LOSS_A2C)
    check_modes(got, a2c, ("d_mean", "d_logstd"))
    want = gr.run_losses_ref(c, tanh, gr.LOSS_A2C, False, F64, clip=CLIP, c_ent=C_ENT)
    want["info"] = R.zero_value_slots(want["info"])
    got["d_v"] = want["d_v"].double()                                         # (no d_v in this mode: nothing to compare)
    r = gr.loss_error_ratios(got, want, B, c["n_global"])
    print("gauss B %d A %d n_global %d: worst err / bound %s" % (B, A, c["n_global"], {k: round(v, 3) for k, v in r.items()}))
    assert all(v <= 1.0 for v in r.values()), r
    assert all(got["info"][k] == FILL for k in (20, 21, 22, 23))             # not written for a Gaussian head


# ================================================================== 2. the categorical loss kernel
def cat_losses(c, mode):
    from torchrl_amd import _C
    critic = mode != R.LOSS_REINFORCE
    B = c["logits"].shape[0]
    info = torch.full((24,), FILL, dtype=F64, device=DEV)
    d_logits, d_v = _C.cat_losses(dev(c["logits"]), dev(c["acts"]), dev(c["advs"]), None, dev(c["v"]) if critic else None,
                                  dev(c["rets"]) if critic else None, None, dev(R.raw_of(c["advs"])), float(B), CLIP, C_ENT,
                                  False, mode, info)
    torch.cuda.synchronize()
    return dict(d_logits=host(d_logits), d_v=d_v, info=info.cpu().numpy())


@pytest.mark.parametrize("A", [2, 64])
@pytest.mark.parametrize("B", BATCHES)
def test_cat_losses(B, A):
    """Bounds of tests/test_categorical_gpu.py::test_cat_losses_gradients_vs_autograd: d_logits rel 1e-4 / abs 1e-6 / B against
    float64 autograd, the entropy and log pi sums rel 1e-5, the surrogate sum rel 1e-4 / abs 1e-3."""
    c = cat_ref_case = R.cat_loss_case(B, A, 5000 + 7 * A + B)
    got, a2c = cat_losses(c, R.LOSS_REINFORCE), cat_losses(c, R.LOSS_A2C)
    check_modes(got, a2c, ("d_logits",))
    l64 = c["logits"].double().requires_grad_(True)
    zero = torch.zeros(B, dtype=F64)
    cat_ref.objective(l64, zero, c["acts"], c["advs"].double(), zero, None, None, CLIP, C_ENT, False, cat_ref.LOSS_A2C).backward()
    err, bound = (got["d_logits"] - l64.grad).abs(), 1e-6 / B + 1e-4 * l64.grad.abs()
    print("cat B %d A %d: d_logits worst err / bound %.3f" % (B, A, float((err / bound).max())))
    assert bool((err <= bound).all())
    r = cat_ref.losses(cat_ref_case["logits"], c["v"], c["acts"], c["advs"], c["rets"], None, None, CLIP, C_ENT, False,
                       cat_ref.LOSS_A2C)
    i = got["info"]
    assert i[20] == pytest.approx(r["ent"].double().sum().item(), rel=1e-5)
    assert i[1] == pytest.approx(r["lp"].double().sum().item(), rel=1e-5)
    assert i[0] == pytest.approx(r["surr"].double().sum().item(), rel=1e-4, abs=1e-3)
    assert all(i[k] == 0.0 for k in (8, 9, 10, 11, 16, 17, 18, 19)) and all(i[k] == FILL for k in (21, 22, 23))


# ================================================================== 3. the state-dependent-std loss kernel
def sd_losses(c, tanh, mode):
    from torchrl_amd import _C
    critic = mode != R.LOSS_REINFORCE
    B = c["head"].shape[0]
    info = torch.full((24,), FILL, dtype=F64, device=DEV)
    d_head, d_v = _C.gauss_sd_losses(dev(c["head"]), dev(c["acts"]), dev(c["advs"]), None, dev(c["v"]) if critic else None,
                                     dev(c["rets"]) if critic else None, None, dev(R.raw_of(c["advs"])), float(B), CLIP, C_ENT,
                                     False, tanh, mode, info)
    torch.cuda.synchronize()
    return dict(d_head=host(d_head), d_v=d_v, info=info.cpu().numpy())


SD_SUM_SLOTS = (0, 1, 2, 7, 12, 13, 20)


@pytest.mark.parametrize("tanh", [True, False])
@pytest.mark.parametrize("A", [1, 32])
@pytest.mark.parametrize("B", BATCHES)
def test_gauss_sd_losses(B, A, tanh):
    """Bounds of tests/test_gauss_sd_gpu.py::test_losses_vs_restatement_in_float64: d_head rel 1e-4 / abs 1e-4 / B, scalars rel
    1e-4 / abs 1e-5 (times B on the slots that hold sums)."""
    c = R.sd_loss_case(B, A, tanh, 6000 + 7 * A + B)
    got, a2c = sd_losses(c, tanh, R.LOSS_REINFORCE), sd_losses(c, tanh, R.LOSS_A2C)
    check_modes(got, a2c, ("d_head",))
    want = sd_ref.losses(c["head"].double(), c["v"].double(), c["acts"].double(), c["advs"].double(), c["rets"].double(), None,
                         None, CLIP, C_ENT, False, sd_ref.LOSS_A2C, tanh)
    err, bound = (got["d_head"] - want["d_head"]).abs(), 1e-4 / B + 1e-4 * want["d_head"].abs()
    print("sd B %d A %d: d_head worst err / bound %.3f" % (B, A, float((err / bound).max())))
    assert bool((err <= bound).all())
    w = R.zero_value_slots(want["info"])
    for k in range(21):
        if np.isnan(w[k]):                                                    # the std of a single element (B * A == 1 never occurs)
            assert np.isnan(got["info"][k]), k
        else:
            assert got["info"][k] == pytest.approx(w[k], rel=1e-4, abs=1e-5 * B if k in SD_SUM_SLOTS else 1e-5), k
    assert all(got["info"][k] == FILL for k in (21, 22, 23))


# ================================================================== 4. what stays refused
def test_other_modes_still_need_the_critic():
    from torchrl_amd import _C
    g, c, s = gr.loss_case(8, 2, True, 2), R.cat_loss_case(8, 3, 3), R.sd_loss_case(8, 2, True, 4)
    info, dl = torch.zeros(24, dtype=F64, device=DEV), torch.zeros(2, device=DEV)
    raw = lambda a: dev(R.raw_of(a))
    for mode in (R.LOSS_A2C, R.LOSS_PPO_CLIP):
        old = lambda x, k: dev(torch.zeros(x[k].shape[0]))
        with pytest.raises(_C.TrlError, match="is None|null"):
            _C.ppo_generic_losses(dev(g["mean"]), dev(g["logstd"]), dev(g["acts"]), dev(g["advs"]), old(g, "mean"), None,
                                  dev(g["rets"]), None, dev(g["adv_raw"]), 8.0, CLIP, C_ENT, False, True, mode, dl, info)
        with pytest.raises(_C.TrlError, match="is None|null"):
            _C.cat_losses(dev(c["logits"]), dev(c["acts"]), dev(c["advs"]), old(c, "logits"), None, dev(c["rets"]), None,
                          raw(c["advs"]), 8.0, CLIP, C_ENT, False, mode, info)
        with pytest.raises(_C.TrlError, match="is None|null"):
            _C.gauss_sd_losses(dev(s["head"]), dev(s["acts"]), dev(s["advs"]), old(s, "head"), None, dev(s["rets"]), None,
                               raw(s["advs"]), 8.0, CLIP, C_ENT, False, True, mode, info)
    with pytest.raises(_C.TrlError, match="clipped_value_loss"):
        _C.cat_losses(dev(c["logits"]), dev(c["acts"]), dev(c["advs"]), None, None, None, None, raw(c["advs"]), 8.0, CLIP, C_ENT,
                      True, R.LOSS_REINFORCE, info)
    torch.cuda.synchronize()


# ================================================================== 5. the fused gradient launch, all-policy
class Fused:
    """One head's input set on the device, the descriptor of its gradient launch, and the float64 policy gradient."""

    def __init__(self, head, c):
        from torchrl_amd import _C
        self.head, sfx = head, {"gauss": "", "cat": "cat_", "sd": "sd_"}[head]
        mod = {"gauss": pc, "cat": cu, "sd": su}[head]
        self.x = x = mod.grad_inputs(c)
        self.mb = mod.minibatch(x)
        self.D, self.A, self.B = x["D"], x["A"], x["rows"] * x["N"]
        self.t = {k: dev(x[k]) for k in ("obs", "acts", "advs", "rets", "old_values", "old_logp")}
        self.row_idx = dev(x["row_idx"])
        pol = list(x["pf"]) + ([x["logstd"]] if head == "gauss" else [])
        self.flat0 = dev(torch.cat([p.reshape(-1) for p in pol + list(x["vf"])]))
        self.P_pf = sum(p.numel() for p in pol)
        self.raw = x["adv_raw"] if head == "gauss" else R.raw_of(self.mb["advs"])
        self.raw_dev = dev(self.raw, F64)
        self.n_global = x["n_global"] if head == "gauss" else float(self.B)
        self.tanh = bool(x.get("tanh", True))
        self.c_ent = mod.C_ENT
        self.ps = getattr(_C, "ppo_%spartial_stride" % sfx)(self.D, H, self.A)
        self.sw = _C.ppo_sd_scalar_stride() if head == "sd" else 8
        self.act = _C.ACT_TANH if x["act"] == "tanh" else _C.ACT_RELU
        lib = _C.lib()
        self.k_grad = getattr(lib, "trl_ppo_%sminibatch_grad_f32" % sfx)
        self.k_fold = getattr(lib, "trl_ppo_%sreduce_adam_net_f32" % sfx)
        self.n_ws = getattr(lib, "trl_ppo_%sreduce_adam_workspace" % sfx)(self.D, H, self.A)

    def launch(self, flat, mode, n_wg):
        """An all-policy gradient launch into pre-filled rows -> (partial, scal)."""
        from torchrl_amd import _C
        g = _C.PpoBatchArgs()
        g.obs, g.acts, g.advs = (self.t[k].data_ptr() for k in ("obs", "acts", "advs"))
        if mode != R.LOSS_REINFORCE:                                          # (the A2C launch gets everything it may name)
            g.rets, g.old_values = self.t["rets"].data_ptr(), self.t["old_values"].data_ptr()
            g.vf_params = flat.data_ptr() + 4 * self.P_pf
        g.row_idx, g.rows_mb, g.N = self.row_idx.data_ptr(), self.x["rows"], self.x["N"]
        g.adv_raw, g.n_global = self.raw_dev.data_ptr(), self.n_global
        g.pf_params = flat.data_ptr()
        g.D, g.H, g.A, g.act = self.D, H, self.A, self.act
        g.clip_para, g.entropy_coeff, g.clipped_value_loss, g.tanh_action = CLIP, self.c_ent, 0, int(self.tanh)
        g.loss_mode = mode
        partial = torch.full((n_wg, self.ps), FILL, device=DEV)
        scal = torch.full((n_wg * self.sw,), FILL, dtype=F64, device=DEV)
        g.partial, g.scal_partial, g.n_wg, g.n_wg_pf = partial.data_ptr(), scal.data_ptr(), n_wg, n_wg
        _C.check(self.k_grad(C.byref(g), _C.stream_ptr(DEV)), "gradient launch")
        return partial, scal

    def fold_adam(self, partial, scal, n_wg, flat, m, v, lr, eps, step):
        from torchrl_amd import _C
        grads = torch.zeros(self.P_pf, device=DEV)
        info = torch.full((24,), FILL, dtype=F64, device=DEV)
        norms = torch.zeros(2, device=DEV)
        ws = torch.zeros(self.n_ws, device=DEV)
        a = _C.adam_args(flat, grads, m, v, (self.P_pf,), (lr,), max_norm=0.5, eps=eps, norms_out=norms.data_ptr(),
                         step_count=step)
        _C.check(self.k_fold(partial.data_ptr(), scal.data_ptr(), n_wg, 0, self.D, H, self.A, grads.data_ptr(), info.data_ptr(),
                             C.byref(a), ws.data_ptr(), _C.stream_ptr(DEV)), "policy fold")
        torch.cuda.synchronize()
        assert int(ws[:1].view(torch.int32).item()) == 0                      # no norm rendezvous timed out
        return grads.cpu().double().numpy(), info.cpu().numpy(), float(norms[0])

    def grad64(self):
        """The policy's flat gradient [W1 b1 W2 b2 W3 b3 (d_logstd)] by float64 autograd of the A2C / REINFORCE objective."""
        x, mb = self.x, self.mb
        if self.head == "gauss":
            w = pref.minibatch_grads(x["pf"], x["logstd"], x["vf"], mb, self.raw, self.n_global, gr.LOSS_A2C, False, self.tanh,
                                     x["act"], F64, CLIP, self.c_ent)
            return w["pf"].double().numpy()
        pf = [p.double().requires_grad_(True) for p in x["pf"]]
        obs, advs = mb["obs"].double(), mb["advs"].double().reshape(-1)
        zero = torch.zeros(self.B, dtype=F64)
        if self.head == "cat":
            loss = cat_ref.objective(cu.forward(pf, obs, x["act"]), zero, mb["acts"].reshape(-1), advs, zero, None, None, CLIP,
                                     self.c_ent, False, cat_ref.LOSS_A2C)
        else:
            loss = sd_ref.objective(su.forward(pf, obs, x["act"]), zero, mb["acts"].double(), advs, zero, None, None, CLIP,
                                    self.c_ent, False, sd_ref.LOSS_A2C, self.tanh)[0]
        loss.backward()
        return torch.cat([p.grad.reshape(-1) for p in pf]).numpy()


# one full tile per time row; a full and a partial tile per row with waves that get no tile (48 samples, 8 waves)
FUSED_CASES = [("gauss", (17, 6, "tanh", "contig1", "plain")), ("gauss", (17, 6, "tanh", "partial", "plain")),
               ("cat", (17, 6, "tanh", "contig")), ("cat", (18, 2, "relu", "partial")),
               ("sd", (17, 6, "tanh", "contig", False)), ("sd", (18, 1, "relu", "partial", False))]


@pytest.mark.parametrize("head,c", FUSED_CASES, ids=lambda v: v if isinstance(v, str) else "_".join(str(k) for k in v))
def test_all_policy_gradient_launch_without_a_critic(head, c):
    assert c in {"gauss": pc.GRAD_CASES, "cat": cu.GRAD_CASES, "sd": su.GRAD_CASES}[head]
    L = Fused(head, c)
    n_wg = 2
    p_r, s_r = L.launch(L.flat0, R.LOSS_REINFORCE, n_wg)
    p_a, s_a = L.launch(L.flat0, R.LOSS_A2C, n_wg)
    torch.cuda.synchronize()
    assert torch.equal(p_r, p_a) and torch.equal(s_r, s_a)
    assert bool(torch.isfinite(p_r[:, :L.P_pf]).all()) and not bool((p_r[:, :L.P_pf] == FILL).any())
    # the policy's fold + clip + Adam on that launch, eps 1e-8, non-trivial moments (so the step is well conditioned)
    rs = np.random.RandomState(17)
    m0 = (rs.randn(L.P_pf) * 1e-3).astype(np.float32)
    v0 = ((rs.rand(L.P_pf) + 0.1) * 1e-5).astype(np.float32)
    lr, eps, step = np.float32(3e-3), 1e-8, 3
    flat, m, v = L.flat0[:L.P_pf].clone(), dev(m0), dev(v0)
    grads, info, norm = L.fold_adam(p_r, s_r, n_wg, flat, m, v, float(lr), eps, step)
    want_g = L.grad64()
    top = np.abs(want_g).max()
    print("%s %s: gradient max abs err %.3e of max %.3e" % (head, c, np.abs(grads - want_g).max(), top))
    assert np.abs(grads - want_g).max() <= 1e-4 * top
    assert norm == pytest.approx(float(np.sqrt((want_g ** 2).sum())), rel=1e-4)
    opt = pref.AdamRef(L.flat0[:L.P_pf].cpu().numpy(), m0, v0, (L.P_pf,), eps=eps)
    opt.step(want_g, (lr,), 0.5, 1.0, step)
    err = float(np.abs(flat.cpu().double().numpy() - opt.p).max())
    print("%s %s: parameters after the step, max abs err %.3e (bound 1e-6)" % (head, c, err))
    assert err <= 1e-6 and not torch.equal(flat, L.flat0[:L.P_pf])
    assert all(info[k] == FILL for k in R.VALUE_SLOTS)                        # the policy's fold leaves the value slots alone
    assert np.isfinite(info[:7]).all()
