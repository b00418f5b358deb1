"""The CPU twin of tests/test_ppo_update_kernels_gpu.py (no GPU, no kernel):

  * pins the gradient restatement (tests/_ppo_update_ref.py) to oracle/ppo.py's PPOOracle / A2COracle formulas run in
    float64 and, with the Adam restatement, to the ppo_update / a2c_update goldens of the reference;
  * pins the Adam restatement to torch.optim.Adam + clip_grad_norm_ in float64;
  * asserts every input condition of tests/_ppo_update_cases.py on exactly the inputs the GPU file runs, and that SEED_BUMP
    is the first seed that meets them;
  * measures RELU_MARGIN and the constants K of the bounds from the restatement's FLOAT32 run, and holds that run to every
    bound of the GPU file at a quarter of the bound (the factor 4 is left to the kernels' other summation order, fp32 MFMA
    accumulation and __expf)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _gauss_ref as gr                                                       # noqa: E402
import _ppo_update_cases as pc                                                # noqa: E402
import _ppo_update_ref as ref                                                 # noqa: E402
from oracle import nets                                                       # noqa: E402
from oracle.ppo import A2COracle, PPOOracle                                   # noqa: E402

MARGIN = 4.0
_RUNS = {}


def runs(c, loss_mode, clipv):
    """(float64 run, float32 run, floors) of the restatement on a case, computed once."""
    key = (pc.case_id(c), loss_mode, clipv)
    if key not in _RUNS:
        x = pc.grad_inputs(c)
        mb = pc.minibatch(x)
        a = (x["pf"], x["logstd"], x["vf"], mb, x["adv_raw"], x["n_global"], loss_mode, clipv, x["tanh"], x["act"])
        w = ref.minibatch_grads(*a, torch.float64, x["clip"], pc.C_ENT)
        g = ref.minibatch_grads(*a, torch.float32, x["clip"], pc.C_ENT)
        _RUNS[key] = (x, w, g, ref.grad_floor(mb, x["pf"], x["vf"], x["act"], x["n_global"]))
    return _RUNS[key]


# ------------------------------------------------------------------ the restatement against the oracle and the goldens
def oracle_grads64(x, loss_mode, clipv):
    """oracle/ppo.py's losses (PPOOracle.update / A2COracle.update, written for float32) on float64 tensors."""
    d = lambda t: t.double()
    cls = A2COracle if loss_mode == gr.LOSS_A2C else PPOOracle
    o = cls([d(p) for p in x["pf"]], d(x["logstd"]), [d(p) for p in x["vf"]], entropy_coeff=pc.C_ENT, clip_para=x["clip"],
            clipped_value_loss=clipv, act=x["act"], tanh_action=x["tanh"])
    mb = pc.minibatch(x)
    obs, acts, advs = d(mb["obs"]), d(mb["acts"]), d(mb["advs"])
    rets, old_v, old_lp = d(mb["rets"]), d(mb["old_values"]), d(mb["old_logp"])
    advs = (advs - advs.mean()) / (advs.std() + 1e-5)
    v = nets.mlp(obs, o.vf, o.act)
    if clipv:
        v_clip = old_v + (v - old_v).clamp(-o.clip_para, o.clip_para)
        vl = 0.5 * torch.max((v - rets) ** 2, (v_clip - rets) ** 2).mean()
    else:
        vl = ((v - rets) ** 2).mean()
    out = nets.policy_update_terms(obs, acts, o.pf, o.logstd, o.act, o.tanh_action)
    lp = out["log_prob"]
    if loss_mode == gr.LOSS_A2C:
        pl = (-lp * advs).mean() - o.entropy_coeff * out["ent"].mean()
    else:
        ratio = torch.exp(lp - old_lp)
        pl = -torch.min(torch.clamp(ratio, 1.0 - o.clip_para, 1.0 + o.clip_para) * advs, ratio * advs).mean() \
            - o.entropy_coeff * out["ent"].mean()
    gp = torch.autograd.grad(pl, o.pf + [o.logstd])
    gv = torch.autograd.grad(vl, o.vf)
    flat = lambda g: torch.cat([t.reshape(-1) for t in g])
    return flat(gp), flat(gv), float(pl), float(vl)


# (the oracle normalises by the local batch, which a shard is not)
ORACLE_CASES = [c for c in pc.GRAD_CASES if c[4] != "shard"]


@pytest.mark.parametrize("c", ORACLE_CASES, ids=pc.case_id)
def test_restatement_is_the_oracle_in_float64(c):
    for loss_mode, clipv in pc.LOSSES:
        x, w, _, _ = runs(c, loss_mode, clipv)
        gp, gv, pl, vl = oracle_grads64(x, loss_mode, clipv)
        B, A = x["rows"] * x["N"], x["A"]
        for name, got, want in (("pf", w["pf"], gp), ("vf", w["vf"], gv)):
            # (log(1 - a^2 + 1e-6) against log((1 - a)(1 + a) + 1e-6): a few ulps of float64 on log pi)
            err, top = float((got - want).abs().max()), float(want.abs().max())
            assert err <= 1e-10 * top, (loss_mode, clipv, name, err, top)
        ent = float(w["loss"]["ent"])
        assert w["info"][0] / B - pc.C_ENT * ent == pytest.approx(pl, rel=1e-10, abs=1e-12)
        assert w["info"][7] / B == pytest.approx(vl, rel=1e-10, abs=1e-12)
        assert np.isnan(w["info"][9]) == (A == 1) and np.isnan(w["info"][17]) == (A == 1)


def _golden_params(g, prefix, with_logstd):
    names = sorted(k for k in g.files if k.startswith(prefix))
    base = [k for k in names if "base__seq_fcs" in k]
    head = [k for k in names if "seq_append_fcs" in k]
    order = sorted(base, key=lambda k: (int(k.split("__")[-2]), "bias" in k)) + sorted(head, key=lambda k: "bias" in k)
    return [torch.tensor(g[k]) for k in order], (torch.tensor(g[prefix + "logstd"]) if with_logstd else None)


def _flat(ps, ls=None):
    return torch.cat([p.reshape(-1) for p in ps] + ([ls.reshape(-1)] if ls is not None else [])).double().numpy()


@pytest.mark.parametrize("name,tag", [("ppo_update", "small"), ("ppo_update", "clipv"), ("ppo_update", "mid"),
                                      ("a2c_update", "small"), ("a2c_update", "mid")])
def test_restatements_reproduce_the_reference_goldens(golden, name, tag):
    """The first update of the fixture: float64 gradients of the restatement, then the Adam restatement's float64 step,
    against the reference's post-step parameters (float32: abs 1e-6, the project's bound) and its info dict."""
    g = golden(name)
    ppo = name == "ppo_update"
    pf, ls = _golden_params(g, f"{tag}_pf0_", True)
    vf, _ = _golden_params(g, f"{tag}_vf0_", False)
    clipv = bool(int(g[f"{tag}_args"][2])) if ppo else False
    t = lambda k: torch.tensor(g[f"{tag}_batch_{k}"])
    mb = dict(obs=t("obs"), acts=t("acts"), advs=t("advs"), rets=t("estimate_returns"))
    B = mb["obs"].shape[0]
    mb["old_values"] = t("values") if ppo else torch.zeros(B, 1)
    if ppo:
        tpf, tls = _golden_params(g, f"{tag}_tpf0_", True)
        mean = ref.layers([p.double() for p in tpf], mb["obs"].double(), "tanh")[0]
        mb["old_logp"] = gr.logp(mean, tls.double(), mb["acts"].double(), True).reshape(-1, 1)
    else:
        mb["old_logp"] = torch.zeros(B, 1, dtype=torch.float64)
    c_ent, plr, vlr = (0.005, 3e-4, 3e-4) if ppo else (0.01, 3e-4, 1e-3)
    w = ref.minibatch_grads(pf, ls, vf, mb, gr.adv_raw_of(mb["advs"]), float(B), gr.LOSS_PPO_CLIP if ppo else gr.LOSS_A2C,
                            clipv, True, "tanh", torch.float64, 0.2, c_ent)
    p0 = np.concatenate([_flat(pf, ls), _flat(vf)])
    opt = ref.AdamRef(p0, np.zeros_like(p0), np.zeros_like(p0), (w["pf"].numel(), w["vf"].numel()))
    r = opt.step(torch.cat([w["pf"], w["vf"]]).numpy(), (plr, vlr), 0.5, 1.0, step_count=1)
    want_pf, want_ls = _golden_params(g, f"{tag}_pf1_", True)
    want_vf, _ = _golden_params(g, f"{tag}_vf1_", False)
    err = np.abs(opt.p - np.concatenate([_flat(want_pf, want_ls), _flat(want_vf)])).max()
    assert err <= 1e-6, err
    info = dict(zip((str(k) for k in g[f"{tag}_info0_keys"]), g[f"{tag}_info0_vals"]))
    i, ent = w["info"], float(w["loss"]["ent"])
    close = lambda a, b: a == pytest.approx(b, rel=1e-4, abs=1e-5)
    assert close(i[0] / B - c_ent * ent, info["Training/policy_loss"]) and close(i[7] / B, info["Training/vf_loss"])
    if ppo:
        assert close(i[1] / B, info["logprob/mean"]) and close(i[3], info["logprob/max"]) and close(-i[4], info["logprob/min"])
        assert close(i[5], info["ratio/max"]) and close(-i[6], info["ratio/min"])
        assert close(i[8], info["log_std/mean"]) and close(i[10], info["log_std/max"]) and close(i[11], info["log_std/min"])
        assert close(r["norms"][0], info["grad_norm/pf"]) and close(r["norms"][1], info["grad_norm/vf"])
    else:
        assert close(i[12] / B, info["v_pred/mean"]) and close(i[14], info["v_pred/max"]) and close(-i[15], info["v_pred/min"])
        sd = np.sqrt(max(i[13] - i[12] * i[12] / B, 0.0) / (B - 1))
        assert close(sd, info["v_pred/std"])
        assert close(i[16], info["std/mean"]) and close(i[17], info["std/std"]) and close(i[18], info["std/max"])
        assert close(i[19], info["std/min"]) and close(i[1] / B, info["log_prob"]) and close(ent, info["ent"])


@pytest.mark.parametrize("sizes", [(7,), (255, 257), (2047, 0, 2049)])
def test_adam_restatement_is_torch_adam_and_clip_grad_norm_in_float64(sizes):
    n = int(sum(sizes))
    off = np.concatenate([[0], np.cumsum(sizes)])
    for kind, max_norm in pc.ADAM_NORMS:
        for gs in pc.ADAM_SCALES:
            x = pc.adam_case(sizes, kind, 11)
            me = ref.AdamRef(x["p"], np.zeros(n), np.zeros(n), sizes)
            ps = [torch.tensor(x["p"][off[k]:off[k + 1]], dtype=torch.float64, requires_grad=True) for k in range(len(sizes))]
            opts = [torch.optim.Adam([p], lr=ref.f32v(pc.ADAM_LRS[k]), betas=(ref.f32v(0.9), ref.f32v(0.999)), eps=ref.f32v(1e-5))
                    for k, p in enumerate(ps)]
            for step, grads in enumerate(pc.chain_grads(n, 4, 3)):
                grads = grads if kind == "big" else grads * np.float32(1e-3)
                r = me.step(grads, pc.ADAM_LRS, max_norm, gs)                # from its own state {steps, beta^steps}
                for k, p in enumerate(ps):
                    p.grad = torch.tensor(grads[off[k]:off[k + 1]], dtype=torch.float64) * ref.f32v(gs)
                    total = float(p.grad.norm()) if p.numel() else 0.0
                    if max_norm > 0:
                        torch.nn.utils.clip_grad_norm_([p], ref.f32v(max_norm))
                    assert r["norms"][k] == pytest.approx(total, rel=1e-13, abs=1e-300)
                    opts[k].step()
                got = torch.cat([p.detach() for p in ps]).numpy()
                assert np.abs(got - me.p).max() <= 1e-14, (kind, max_norm, gs, step)
            assert me.state[0] == 4.0 and me.state[1] == pytest.approx(ref.f32v(0.9) ** 4, rel=1e-15)
            by_count = ref.AdamRef(x["p"], np.zeros(n), np.zeros(n), sizes)
            for step, grads in enumerate(pc.chain_grads(n, 4, 3)):
                grads = grads if kind == "big" else grads * np.float32(1e-3)
                by_count.step(grads, pc.ADAM_LRS, max_norm, gs, step_count=step + 1)
            assert np.abs(by_count.p - me.p).max() <= 1e-15                  # the two sources of the bias corrections agree


# ------------------------------------------------------------------ input conditions
@pytest.mark.parametrize("c", pc.GRAD_CASES, ids=pc.case_id)
def test_input_conditions_and_seed_bumps(c):
    x = pc.grad_inputs(c)
    bad = pc.conditions(x)
    print("%s: seed %d (bump %d), B = %d, conditions violated: %s" % (pc.case_id(c), x["seed"], pc.SEED_BUMP.get(pc.case_id(c), 0),
                                                                       x["rows"] * x["N"], bad))
    assert not bad
    bump = pc.SEED_BUMP.get(pc.case_id(c), 0)
    assert 0 <= bump <= pc.MAX_BUMP
    for b in range(bump):                                                     # a recorded bump skips only seeds that fail
        assert pc.conditions(pc._grad_inputs(c, pc.base_seed(c) + b)), b
    R = x["rows"] + 3
    assert x["obs"].shape == (R, x["N"], x["D"]) and len(set(x["row_idx"].tolist())) == x["rows"]
    assert 1 <= x["row_idx"].min() and x["row_idx"].max() < R               # (row 0 stays outside: see _grad_inputs)
    if x["rows"] > 2:
        assert list(x["row_idx"]) != sorted(x["row_idx"])                     # shuffled
    A = x["A"]
    if x["kind"] == "clamp":
        hi, lo = pc.clamp_columns(A)
        assert float(x["logstd"][hi]) == pc.LS_HIGH and float(x["logstd"][lo]) == pc.LS_LOW and not x["tanh"]
        assert bool((x["pf"][4][lo] == 0).all()) and bool((x["acts"][..., lo] == x["pf"][5][lo]).all())
        assert bool(((x["logstd"][1:A - 1] > -20) & (x["logstd"][1:A - 1] < 2)).all()) and A >= 3
    else:
        assert bool(((x["logstd"] > -20) & (x["logstd"] < 2)).all())
    if x["kind"] == "tie":
        assert bool((x["vf"][4] == 0).all()) and float(x["vf"][5]) == 0.5 and x["clip"] == 0.25
        mb = pc.minibatch(x)
        d = 0.5 - mb["old_values"].reshape(-1)
        assert bool((mb["old_values"] * 8 == (mb["old_values"] * 8).round()).all()) and bool((mb["rets"] * 8 == (mb["rets"] * 8).round()).all())
        kinds = set()
        for dv, R_ in zip(d.tolist(), mb["rets"].reshape(-1).tolist()):
            vc = 0.5 - dv + min(max(dv, -0.25), 0.25)
            l1, l2 = (0.5 - R_) ** 2, (vc - R_) ** 2
            kinds.add(("gate" if abs(dv) == 0.25 else "out" if abs(dv) > 0.25 else "in", "tie" if l1 == l2 else "l1" if l1 > l2 else "l2"))
        assert {("gate", "tie"), ("out", "tie"), ("out", "l1"), ("out", "l2"), ("in", "tie")} <= kinds
    if x["kind"] == "shard":
        assert x["n_global"] == 3 * x["rows"] * x["N"]


def test_layouts_reach_the_tile_walks_they_are_named_for():
    """Arithmetic on the layouts: tiles per row, tile stride, what a wave's walk does."""
    walk = {}
    for name, (N, rows, n_wg, n_pf) in pc.LAYOUTS.items():
        per_net = n_pf if n_pf else n_wg // 2
        tiles, stride = -(-rows * N // 16), 4 * per_net
        walk[name] = dict(contig=N % 16 == 0, tpr=N // 16, tiles=tiles, stride=stride, per_wave=-(-tiles // stride))
    assert walk["contig1"] == dict(contig=True, tpr=1, tiles=6, stride=4, per_wave=2)
    assert walk["cols"] == dict(contig=True, tpr=3, tiles=33, stride=8, per_wave=5)       # row step 2, column step 2: wraps
    assert walk["cols"]["stride"] % walk["cols"]["tpr"] != 0
    assert walk["longrow"] == dict(contig=True, tpr=10, tiles=20, stride=4, per_wave=5)  # stride < tiles per row
    assert not walk["ragged"]["contig"] and (7 * 12) % 16 != 0
    assert not walk["partial"]["contig"] and walk["partial"]["tiles"] == 3
    assert walk["empty"]["tiles"] == 1 and walk["empty"]["stride"] == 4
    assert walk["uneven"]["stride"] == 12 and pc.LAYOUTS["uneven"][2] - pc.LAYOUTS["uneven"][3] == 2
    assert all(rows * N <= 640 for (N, rows, _, _) in pc.LAYOUTS.values())
    rows = sorted({n for n_wg, n_pf in pc.FOLD_SPLITS for n in (n_pf, n_wg - n_pf)})
    assert rows == [1, 2, 8, 9, 109, 128, 129, 147, 192, 193]


# ------------------------------------------------------------------ RELU_MARGIN and the constants K
def test_relu_margin():
    worst = 0.0
    for c in pc.GRAD_CASES:
        if c[2] != "relu":
            continue
        x, w, g, _ = runs(c, *pc.LOSSES[0])
        worst = max(worst, float((g["z"].double() - w["z"]).abs().max()))
    print("largest |z_float32 - z_float64| over the ReLU cases: %.3e; RELU_MARGIN %.3e" % (worst, pc.RELU_MARGIN))
    assert 4.0 * worst <= pc.RELU_MARGIN <= 8.0 * worst


def test_gradient_constants_are_the_measured_ones():
    """K_W / K_LS: the smallest powers of two for which the float32 run stays under a quarter of the element bound on every
    element of every case."""
    need_w, need_ls, at = 0.0, 0.0, None
    for c in pc.GRAD_CASES:
        for loss_mode, clipv in pc.LOSSES:
            x, w, g, fl = runs(c, loss_mode, clipv)
            A = x["A"]
            kw = max(ref.k_needed(g["pf"][:-A], w["pf"][:-A], w["M_pf"][:-A], fl[0][:-A], MARGIN),
                     ref.k_needed(g["vf"], w["vf"], w["M_vf"], fl[1], MARGIN))
            kl = ref.k_needed(g["pf"][-A:], w["pf"][-A:], w["M_pf"][-A:], fl[0][-A:], MARGIN)
            if kw > need_w:
                need_w, at = kw, (pc.case_id(c), loss_mode, clipv)
            need_ls = max(need_ls, kl)
    print("float32 CPU run: K needed %.2f for weights and biases (at %s), %.2f for d_logstd; K_W = %g, K_LS = %g"
          % (need_w, at, need_ls, pc.K_W, pc.K_LS))
    assert pc.K_W == ref.pow2_at_least(need_w) and pc.K_LS == ref.pow2_at_least(need_ls)


@pytest.mark.parametrize("c", pc.GRAD_CASES, ids=pc.case_id)
def test_float32_restatement_holds_the_gpu_bounds_at_a_quarter(c):
    for loss_mode, clipv in pc.LOSSES:
        x, w, g, fl = runs(c, loss_mode, clipv)
        D, A, B = x["D"], x["A"], x["rows"] * x["N"]
        r = ref.grad_error_ratios(g["pf"], g["vf"], w, fl, pc.K_W, pc.K_LS, D, A)
        worst_block = max(r["blocks"], key=r["blocks"].get)
        print("%s mode %d clipv %d: elem %.3f, d_logstd %.3f of the bound; worst block %s at %.3f of 1e-4 max"
              % (pc.case_id(c), loss_mode, clipv, r["elem"], r["elem_ls"], worst_block, r["blocks"][worst_block]))
        assert r["elem"] <= 1.0 / MARGIN and r["elem_ls"] <= 1.0 / MARGIN
        assert all(v <= 1.0 / MARGIN for v in r["blocks"].values()), r["blocks"]
        assert gr.info_error_ratio(g["info"], w["info"], B) <= 1.0 / MARGIN
        for k in (9, 17):
            assert np.isnan(w["info"][k]) == (A == 1)
        assert np.isfinite(np.delete(w["info"], (9, 17))).all() and (w["info"][20:] == ref.SENTINEL).all()
        if x["kind"] == "clamp":
            hi, lo = pc.clamp_columns(A)
            for run_ in (w, g):
                d = run_["pf"][-A:]
                assert float(d[hi]) == 0.0 and float(d[lo]) == 0.0 and bool((d[1:A - 1] != 0).all())
                assert run_["info"][10] == 2.0 and run_["info"][11] == -20.0
        if x["kind"] == "tie" and clipv:
            assert g["info"][7] == pytest.approx(w["info"][7], rel=1e-6)
            sl = ref.block_slices(D, A, False)
            assert bool((w["vf"][sl["W2"]] == 0).all()) and bool((w["vf"][sl["W1"]] == 0).all()) and bool((w["vf"][sl["b3"]] != 0).all())


# ------------------------------------------------------------------ the fold, clip + Adam and Polyak in float32
@pytest.mark.parametrize("n_wg,n_pf", pc.FOLD_SPLITS)
def test_float32_fold_in_the_kernel_order_holds_its_bound(n_wg, n_pf):
    D, A = pc.FOLD_SHAPES[0]
    p_pf, p_vf = pc.p_sizes(D, A)
    part, scal, logstd = pc.fold_case(D, A, n_wg, n_pf, 5760, 100 + n_wg)
    for rows, P in ((part[:n_pf, :p_pf], p_pf), (part[n_pf:n_wg, :p_vf], p_vf)):
        want, S = ref.fold(rows)
        got = torch.from_numpy(ref.fold_kernel_order(rows.numpy())).double()
        assert bool(((got - want).abs() <= ref.fold_bound(rows.shape[0], S)).all())
        assert bool(torch.isfinite(want).all()) and float(rows.abs().max()) > 100 and float(rows.abs().min()) < 1e-2
    assert np.isfinite(np.delete(pc.fold_info(scal, n_wg, n_pf, logstd), (20, 21, 22, 23))).all()


def adam_runs(sizes):
    """[(label, steps)] of every clip + Adam check on a group layout: the single-step combinations and the 5-step chain."""
    n = int(sum(sizes))
    out = []
    for kind, max_norm, gs, count, zero in pc.adam_combos(sizes):
        x = pc.adam_case(sizes, kind, 17, zero)
        out.append(("%s_mn%g_gs%g_t%d_z%s" % (kind, max_norm, gs, count, zero), x, [(x["g"], pc.ADAM_LRS, max_norm, gs, count)]))
    x = pc.adam_case(sizes, "big", 19)
    out.append(("chain", x, pc.chain_steps(n, len(sizes))))
    return out


def adam_needs(sizes):
    need = dict(m=0.0, v=0.0, p=0.0, norm=0.0)
    for label, x, steps in adam_runs(sizes):
        o64, bound, r64 = ref.adam_chain(x, sizes, steps)
        o32, _, r32 = ref.adam_chain(x, sizes, steps, np.float32)
        for k, v in ref.adam_k_needed(o32.p, o32.m, o32.v, o64, bound, pc.K_R, MARGIN).items():
            need[k] = max(need[k], v)
        nz = r64["norms"] > 0
        if nz.any():
            need["norm"] = max(need["norm"], float((np.abs(r32["norms"][nz] - r64["norms"][nz]) / r64["norms"][nz]).max()))
        if label == "chain":
            assert o64.state[0] == 5.0 and o64.state[1] == pytest.approx(ref.f32v(0.9) ** 5, rel=1e-15)
    return need


@pytest.mark.parametrize("sizes", pc.ADAM_LAYOUTS, ids=lambda s: "x".join(str(k) for k in s))
def test_float32_adam_holds_the_gpu_bounds_at_a_quarter(sizes):
    need = adam_needs(sizes)
    print("sizes %s: float32 CPU run needs K_M %.2f, K_V %.2f, K_P %.2f (K_R = %g); norms rel %.2e"
          % (sizes, need["m"], need["v"], need["p"], pc.K_R, need["norm"]))
    assert need["m"] <= pc.K_M and need["v"] <= pc.K_V and need["p"] <= pc.K_P and need["norm"] <= 1e-5 / MARGIN


def test_adam_constants_are_the_measured_ones():
    need = dict(m=0.0, v=0.0, p=0.0)
    for sizes in pc.ADAM_LAYOUTS:
        for k, v in adam_needs(sizes).items():
            if k in need:
                need[k] = max(need[k], v)
    print("float32 CPU run over all layouts: K needed m %.2f, v %.2f, params %.2f" % (need["m"], need["v"], need["p"]))
    assert pc.K_M == ref.pow2_at_least(need["m"]) and pc.K_V == ref.pow2_at_least(need["v"]) and pc.K_P == ref.pow2_at_least(need["p"])


def test_float32_polyak_holds_its_bound():
    rs = np.random.RandomState(4)
    t, s = rs.randn(4099).astype(np.float32), rs.randn(4099).astype(np.float32)
    got, want = ref.polyak(t, s, 0.005, np.float32), ref.polyak(t, s, 0.005)
    assert (np.abs(got.astype(np.float64) - want) <= ref.polyak_bound(t, s)).all()
    assert [ref.ring_row(u, 3) for u in range(5)] == [0, 1, 2, 0, 1]


@pytest.mark.parametrize("c", pc.CHAIN_CASES, ids=pc.case_id)
def test_float32_three_updates_hold_the_parameter_bound_at_a_quarter(c):
    """Three whole updates (gradients, clip, Adam on non-trivial moments) in float32 against float64: the project's bound on
    post-step parameters, abs 1e-6, which the GPU file applies to the kernels' three chained updates."""
    x = pc.grad_inputs(c)
    mb = pc.minibatch(x)
    mv = pc.adam_case(pc.p_sizes(x["D"], x["A"]), "big", 31)
    lrs = (np.float32(3e-4), np.float32(1e-3))
    runs_ = [ref.update_chain(x, mb, mv, lrs, 3, *pc.LOSSES[1], pc.C_ENT, dt) for dt in (np.float64, np.float32)]
    err = float(np.abs(runs_[1].p.astype(np.float64) - runs_[0].p).max())
    print("%s: float32 against float64 after three updates: %.3e" % (pc.case_id(c), err))
    assert err <= 1e-6 / MARGIN and runs_[0].state[0] == 3.0
