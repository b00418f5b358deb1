"""One numpy forward of the `add_ln` two-layer block the persistent rollout's LayerNorm variant carries -- Linear(D, 64), act,
LayerNorm(64), Linear(64, 64), act, act, Linear(64, O) -- in float64 or float32, and the teacher-forced restatement of a
launch's stored cells from it (tests/test_layernorm_rollout_gpu.py).  Bounds are `_rollout_ref.verify`'s per-element forms
(`_gauss_ref.act_bound` / `logp_bound`, `_rollout_ref.sd_logp_terms`, the categorical margin of `_rollout_ref.cat_terms`) with
the head allowance 1e-5 (1 + |element|) widened by the row's LayerNorm amplification max(1, rstd max|gamma|): the factor by
which an error of the first layer's activations grows through the norm."""
import numpy as np
import torch

import _categorical_ref as CR
import _gauss_ref as G
import _rollout_ref as R

U = R.U
CAT_SEED = 0xC011                                                # the collector's key of the categorical draw


def params_of(net):
    """{"lin": [W1, b1, W2, b2, W3, b3], "ln": (gamma, beta) or None} of a two-layer torchrl_amd Net, float64 numpy."""
    from torchrl_amd import ops
    plan = ops.net_plan(net)
    f = lambda t: t.detach().cpu().double().numpy()
    post = plan[0][2]
    return {"lin": [f(t) for w, b, _ in plan for t in (w, b)], "ln": None if post is None else (f(post[1]), f(post[2]))}


def forward(p, x, act, dtype=np.float64):
    """-> (head output (M, O), amplification (M,)) with every intermediate rounded to `dtype`."""
    W1, b1, W2, b2, W3, b3 = (q.astype(dtype) for q in p["lin"])
    fn = R.ACT_FN[act]
    h = fn(np.asarray(x).astype(dtype) @ W1.T + b1).astype(dtype)
    amp = np.ones(len(h))
    if p["ln"] is not None:
        g, be = (q.astype(dtype) for q in p["ln"])
        d = h - h.mean(-1, keepdims=True, dtype=dtype)
        rstd = (dtype(1.0) / np.sqrt((d * d).mean(-1, keepdims=True, dtype=dtype) + dtype(1e-5))).astype(dtype)
        h = (g * (d * rstd) + be).astype(dtype)
        amp = np.maximum(1.0, rstd[:, 0].astype(np.float64) * np.abs(g).max())
        h = fn(fn(h @ W2.T + b2)).astype(dtype)
    else:
        h = fn(h @ W2.T + b2).astype(dtype)
    return (h @ W3.T + b3).astype(dtype), amp


def quantities(c, pf, vf, obs, next_obs, eps, acts, dtype=np.float64):
    """What a launch stores for M cells, restated in `dtype` from the stored observations, the noise and the STORED actions:
    act (Gaussian heads), logp at the stored action, v = V(obs), v2 = V(next_obs).  In float64 also the bounds b_* and, for a
    categorical head, `allowed` (M, A): the indices a float32 implementation may store."""
    A, head, f64 = c["A"], c["head"], dtype == np.float64
    out, amp = forward(pf, obs, c["act"], dtype)
    q = {}
    hb = lambda z: 1e-5 * (1.0 + np.abs(z)) * amp[:, None]
    t = lambda z: torch.from_numpy(np.asarray(z, dtype))
    if head == "cat":
        k = np.asarray(acts).reshape(-1).astype(np.int64)
        rows = np.arange(len(k))
        m = out.max(1, keepdims=True)
        pre = np.cumsum(np.exp(out - m), axis=1, dtype=dtype)
        S = pre[:, -1]
        q["logp"] = (out[rows, k] - m[:, 0]) - np.log(S)
        if f64:                                                   # `_rollout_ref.cat_terms`' margin with the widened allowance
            H = hb(out).max(1)
            thr = (np.asarray(eps, np.float64).reshape(-1) * S)[:, None]
            hit = pre >= thr
            want = np.where(hit.any(1), hit.argmax(1), A - 1)
            close = np.abs(pre - thr) <= (np.expm1(2.0 * H) + (A + 3 + (m - out).max(1)) * U)[:, None] * (pre + thr)
            allowed = np.zeros_like(hit)
            allowed[rows, want] = True
            up, dn = close[rows, want] & (want < A - 1), close[rows, np.maximum(want - 1, 0)] & (want > 0)
            allowed[rows[up], want[up] + 1] = True
            allowed[rows[dn], want[dn] - 1] = True
            q["allowed"] = allowed[rows, k]
            q["b_logp"] = 2.0 * H + U * (np.abs(out[rows, k] - m[:, 0]) + 4.0 * np.abs(np.log(S)) + np.abs(q["logp"]) + 2.0 * A + 2.0)
        q["keep"] = np.ones(len(k), bool)
    else:
        mean = out[:, :A]
        ls = t(out[:, A:]) if head == "sd" else t(c["logstd"])
        q["act"] = G.explore(t(mean), ls, t(eps), c["tanh"])[0].numpy()
        ta = t(acts).clamp(-1 + 1e-12, 1 - 1e-12) if c["tanh"] else t(acts)
        if head == "sd" and f64:
            raw, h, h_ls = out[:, A:], hb(mean), hb(out[:, A:])
            q["b_act"] = h + G.act_bound(t(mean), ls, t(eps), c["tanh"]).numpy() + \
                np.exp(np.clip(raw, -20.0, 2.0)) * np.abs(eps) * np.expm1(h_ls)
            sd = R.sd_logp_terms(c, mean, raw, np.asarray(acts, np.float64), h, h_ls)
            assert not sd["low"].any()                            # (no element on the lower clamp in these cases)
            q.update(logp=sd["logp"], b_logp=sd["b_logp"], keep=sd["keep"])
        else:
            q["logp"] = G.logp(t(mean), ls, ta, c["tanh"]).numpy()
            q["keep"] = G.logp_keep(t(acts), c["tanh"]).numpy()
            if f64:
                p = G.logp_parts(t(mean), ls, ta, c["tanh"])
                h = hb(mean)
                q["b_act"] = h + G.act_bound(t(mean), ls, t(eps), c["tanh"]).numpy()
                q["b_logp"] = (G.logp_bound(t(mean), ls, ta, c["tanh"]) + (p["zc"].abs() / p["var"] * t(h)).sum(-1)).numpy()
    for key, x in (("v", obs), ("v2", next_obs)):
        if vf is None:
            q[key], q["b_" + key] = np.zeros(len(obs)), np.full(len(obs), 1e-30)
        else:
            v, amp_v = forward(vf, x, c["act"], dtype)
            q[key], q["b_" + key] = v[:, 0], 1e-5 * (1.0 + np.abs(v[:, 0])) * amp_v
    return q


def ratios(got, q64):
    """{quantity: worst |got - float64| / bound}; log pi on the rows inside `logp_keep` only, as `_rollout_ref.verify`."""
    out = {}
    for k in ("act", "logp", "v", "v2"):
        if k in got and k in q64:
            sel = q64["keep"] if k == "logp" else slice(None)
            assert np.isfinite(np.asarray(got[k], np.float64)[sel]).all(), k
            out[k] = float((np.abs(np.asarray(got[k], np.float64) - q64[k])[sel] / q64["b_" + k][sel]).max())
    return out


def uniforms(step0, T, N):
    return CR.uniforms(CAT_SEED, step0, T, N, 0).astype(np.float32)
