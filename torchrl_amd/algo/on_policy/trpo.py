"""TRPO on the HIP path (reference: torchrl/algo/on_policy/trpo.py:13-286).

`update(whole_batch)` keeps the reference's procedure -- surrogate gradient, conjugate gradient on the Hessian of the
mean KL, step scaling by max_kl, backtracking line search -- with every pass over the data on the kernels:
  policy forward / backward ............ dense-layer kernels (k_gemm.hip), the tape of the forward is kept
  surrogate loss, its gradients, stats .. trl_trpo_surrogate_f32
  Fisher-vector product F v ............. for a diagonal Gaussian policy the Hessian of mean KL(pi_theta || pi_theta.detach())
      is J^T diag(1 / sigma^2) J / n on the network parameters and 2 on each logstd (trpo.py:62-87 gets the same by
      double backward): one forward-mode pass (trl_linear_fwd_f32 on the v-weights and on the propagated tangents,
      trl_jvp_gate_f32), trl_fisher_scale_f32, one backward pass (trl_linear_bwd_*_f32); + cg_damping * v
  line search objective ................. policy forward with the candidate parameters, trl_gauss_logp_f32, trl_ratio_loss_f32
The CG recurrences themselves are BLAS-1 on ~5 k-element parameter vectors and stay torch tensor expressions on the
device (double-precision dot products as in the reference, :93-106); one scalar read-back per CG iteration and per
line-search trial, as the reference's Python control flow needs.
`update_vf` = 0.5 * MSE, clip_grad_norm_(0.5), Adam(eps 1e-5) on the value net (:228-251).
Works for any MLP shape; policies are used as built (examples/trpo_continuous_vec.py passes no tanh squashing).

The three policy heads (`_GenericPPO.head`) differ in the three element-wise calls only:
  head                 surrogate                     Fisher scaling               line search's log pi
  Gaussian, free logstd  trl_trpo_surrogate_f32      trl_fisher_scale_f32         trl_gauss_logp_f32
  categorical            trl_trpo_surrogate_cat_f32  trl_fisher_scale_cat_f32     trl_cat_logp_f32
  [mean | log_std]       trl_trpo_surrogate_sd_f32   trl_fisher_scale_sd_f32      trl_gauss_sd_logp_f32
The flat policy vector of the last two ends with the head layer (no logstd tail); their Fisher product is all network:
J^T H J / n with H = diag(p) - p p^T in the logits resp. diag(1 / sigma^2 | 2 gate) in the [mean | log_std] head, the
Hessian of the mean KL at the expansion point (the reference's discrete KL has `+ 1e-8` inside its log, which moves that
Hessian by O(1e-8 / p): profiles/NOTES_vmpo_trpo_heads.md).  `acts` of a categorical policy: (B,) or (B, 1) floats.
Refused: LayerNorm nets, the last two heads on several ranks, and either of them with an env whose action space is not of
the head's kind (Discrete for the categorical, Box for the [mean | log_std] one)."""
import numpy as np
import torch

from ... import _C, dist
from .. import utils as atu
from .a2c import A2C
from .ppo import HEAD_CAT, HEAD_GAUSS, HEAD_NAME, HEAD_SD, _GenericPPO, plain_layer_refusals


class TRPO(A2C):
    def __init__(self, max_kl, cg_damping, v_opt_times, cg_iters, residual_tol, **kwargs):
        plain_layer_refusals("TRPO", kwargs.get("pf"), kwargs.get("vf"), kwargs.get("env"))
        if kwargs.get("optimizer_class", torch.optim.Adam) is not torch.optim.Adam:
            raise _C.TrlError("the TRPO value step implements torch.optim.Adam only")
        super().__init__(**kwargs)
        self.max_kl, self.cg_damping, self.cg_iters, self.residual_tol = max_kl, cg_damping, cg_iters, residual_tol
        self.v_opt_times = v_opt_times
        self.vf_sample_key = ["obs", "estimate_returns"]
        self._engine = None

    @property
    def networks(self):
        return [self.pf, self.vf]

    def engine(self):
        if self._engine is None:
            self._engine = _TRPOEngine(self)
        return self._engine

    def update(self, batch):
        self.training_update_num += 1
        return self.engine().update(batch)

    def update_vf(self, batch):
        self.training_update_num += 1
        return self.engine().update_vf(batch)

    def update_per_epoch(self):
        self.process_epoch_samples()
        atu.update_linear_schedule(self.pf_optimizer, self.current_epoch, self.num_epochs, self.plr)
        atu.update_linear_schedule(self.vf_optimizer, self.current_epoch, self.num_epochs, self.vlr)
        buf = self.replay_buffer
        flat = lambda t: t.reshape(t.shape[0] * t.shape[1], -1)
        self.logger.add_update_info(self.update({"obs": flat(buf._obs), "acts": flat(buf._acts), "advs": flat(buf._advs),
                                                 "estimate_returns": flat(buf._estimate_returns)}))
        for _ in range(self.v_opt_times):
            for batch in buf.one_iteration(self.batch_size, self.vf_sample_key, self.shuffle):
                self.logger.add_update_info(self.update_vf(batch))


class _TRPOEngine(_GenericPPO):
    carries_layernorm = False                                          # (its own passes walk the plain layer lists)
    step_kinds = ("adam",)                                             # (`update_vf` launches trl_clip_adam_f32 itself)

    def __init__(self, algo):
        super().__init__(algo)
        self._stat = torch.zeros(4 + 5 + 1 + 1, dtype=torch.float64, device=self.dev)   # adv raw | info | scalar | vf loss
        self._zero_idx = torch.zeros(1, 1, dtype=torch.int64, device=self.dev)
        self._vf_norm = torch.zeros(1, device=self.dev)
        self.vf_steps = 0

    # ---- flat parameter vectors <-> per-layer views ----
    def _views(self, flat):
        """[(W, b), ...] of a flat policy-parameter-shaped vector -- the head layer as wide as the engine's layer list has it
        -- and the logstd slice behind them (None: the vector of a categorical / [mean | log_std] head ends with the head layer)."""
        out, off = [], 0
        for w, b in self.pf_layers:
            out.append((flat[off:off + w.numel()].view(w.shape), flat[off + w.numel():off + w.numel() + b.numel()]))
            off += w.numel() + b.numel()
        return out, (flat[off:off + self.A] if self.head == HEAD_GAUSS else None)

    def _logstd(self):
        return self.algo.pf.logstd.detach() if self.head == HEAD_GAUSS else None

    def _forward(self, layers):
        return self.ops.mlp_forward(layers, self.obs, self.act)

    def _logp_of(self, head, logstd):
        """log pi(acts) from the head layer's output (and the logstd vector, for the head that has one)."""
        if self.head == HEAD_CAT:
            return _C.cat_logp(head, self.acts)[0]
        if self.head == HEAD_SD:
            return _C.gauss_sd_logp(head, self.acts, self.tanh_action)[0]
        return _C.gauss_logp(head, self.acts, logstd.contiguous(), self.tanh_action)

    def _logp(self, layers, logstd):
        return self._logp_of(self._forward(layers)[0], logstd)

    def _fisher_scale(self, t, head):
        """d KL / d head along the tangent t of the head layer's output, at the expansion point."""
        if self.head == HEAD_CAT:
            return _C.fisher_scale_cat(t, head)
        if self.head == HEAD_SD:
            return _C.fisher_scale_sd(t, head)
        return _C.fisher_scale(t, self._logstd())

    def _fvp(self, v):
        """F v + cg_damping * v at the current parameters (tape of the current forward in self.tape)."""
        tape, act = self.tape, self.act
        vl, v_ls = self._views(v)
        n_layers = len(self.pf_layers)
        dh = None
        for k, (w, _b) in enumerate(self.pf_layers):
            inp = tape.x if k == 0 else tape.outs[k - 1]
            a = _C.linear_fwd(inp, vl[k][0].contiguous(), vl[k][1].contiguous(), _C.ACT_NONE)   # x W_v^T + b_v
            b = None if dh is None else _C.linear_fwd(dh, w, None, _C.ACT_NONE)                # dx W^T
            last = k == n_layers - 1
            dh = _C.jvp_gate(a, b, None if last else tape.outs[k], act)
        g_head = self._fisher_scale(dh, tape.outs[-1])                                          # d KL / d head
        out = torch.zeros_like(v)
        ol, o_ls = self._views(out)
        self.ops.mlp_backward(tape, g_head, grads=ol, workspace=self._ws(self.n))
        if o_ls is not None:
            raw = self._logstd()
            o_ls.copy_(2.0 * v_ls * ((raw >= -20.0) & (raw <= 2.0)).to(v.dtype))
        return out + self.algo.cg_damping * v

    def _cg(self, b):
        algo = self.algo
        p, r, x = b.clone(), b.clone(), torch.zeros_like(b)
        rdotr = r.double().dot(r.double())
        for _ in range(algo.cg_iters):
            z = self._fvp(p)
            v = (rdotr / p.double().dot(z.double())).float()
            x += v * p
            r -= v * z
            newrdotr = r.double().dot(r.double())
            p = r + (newrdotr / rdotr).float() * p
            rdotr = newrdotr
            if float(rdotr) < algo.residual_tol:
                break
        return x

    def _surrogate(self, theta):
        layers, ls = self._views(theta)
        lp_new = self._logp([(w.contiguous(), b.contiguous()) for w, b in layers], ls)
        return float(_C.ratio_loss(lp_new, self.lp_old, self.adv_n, self._stat[9:10]).item())

    def _linesearch(self, x, fullstep, expected_improve_rate):
        fval = self._surrogate(x)
        self.search = []                                                 # (actual improvement, acceptance ratio) per trial
        for stepfrac in .5 ** np.arange(10):
            xnew = x + float(stepfrac) * fullstep
            actual = fval - self._surrogate(xnew)
            self.search.append((actual, actual / (expected_improve_rate * float(stepfrac))))
            if self.search[-1][1] > .1 and actual > 0:
                return xnew
        self.search.append(None)                                         # (no trial was accepted)
        return x

    def update(self, batch):
        algo, dev = self.algo, self.dev
        as_t = lambda x: (x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))) \
            .to(device=dev, dtype=torch.float32).contiguous()
        self.obs, self.acts = as_t(batch['obs']), as_t(batch['acts'])
        advs = as_t(batch['advs']).reshape(-1)
        if self.head == HEAD_CAT:
            self.acts = self.acts.reshape(-1)                              # one index per sample, given as (B,) or (B, 1)
        if dist.collectives_active():
            if self.head != HEAD_GAUSS:
                raise _C.TrlError("TRPO with a %s policy runs on one rank" % HEAD_NAME[self.head])
            # The natural-gradient step (CG on Fisher products, line search) is one global solve: gather the env shards
            # and run it replicated on the single-process batch -- identical parameters on every rank, no exchange.
            ne = int(algo.replay_buffer.env_nums)
            self.obs, self.acts = dist.gather_env_shards(self.obs, ne), dist.gather_env_shards(self.acts, ne)
            advs = dist.gather_env_shards(advs.view(-1, 1), ne).view(-1)
        self.n = n = int(self.obs.shape[0])
        self.tanh_action = bool(getattr(algo.pf, "tanh_action", False))
        raw, info = self._stat[:4], self._stat[4:9]
        _C.adv_stats(advs.view(1, n), self._zero_idx, raw.view(1, 4))
        self.adv_n = _C.adv_normalize(advs, raw, n, eps=1e-4)            # trpo.py:168
        logstd = self._logstd()
        head, self.tape = self._forward(self.pf_layers)
        g = torch.zeros(self.P_pf, device=dev)
        gl, g_ls = self._views(g)
        if self.head == HEAD_CAT:
            d_head = _C.trpo_surrogate_cat(head, self.acts, self.adv_n, algo.entropy_coeff, info)
        elif self.head == HEAD_SD:
            d_head = _C.trpo_surrogate_sd(head, self.acts, self.adv_n, self.tanh_action, algo.entropy_coeff, info)
        else:
            d_head = _C.trpo_surrogate(head, logstd, self.acts, self.adv_n, self.tanh_action, algo.entropy_coeff, g_ls, info)
        self.ops.mlp_backward(self.tape, d_head, grads=gl, workspace=self._ws(n))
        self.lp_old = self._logp_of(head, logstd)
        self.search = None                                               # (stays None when the gradient is zero)
        if bool((g != 0).any()):                                          # "ensure gradient is not zero" (:188)
            step = self._cg(-g)
            shs = .5 * step.dot(self._fvp(step))
            lm = torch.sqrt(shs / algo.max_kl)
            theta0 = self.flat[:self.P_pf].clone()
            theta = self._linesearch(theta0, step / lm, float(-g.dot(step) / lm))
            if not bool(torch.isnan(theta).any()):
                self.flat[:self.P_pf].copy_(theta)
        host = self._stat.cpu()
        r, i = host[:4].numpy(), host[4:9].numpy()
        mean_adv = r[0] / n
        return {'advs/mean': mean_adv, 'advs/std': float(np.sqrt(max((r[1] - r[0] * mean_adv) / (n - 1), 0.0))),
                'advs/max': r[2], 'advs/min': -r[3], 'Training/policy_loss': i[0],
                'logprob/mean': i[1], 'logprob/std': i[2], 'logprob/max': i[3], 'logprob/min': i[4]}

    def update_vf(self, batch):
        algo, dev, ops = self.algo, self.dev, self.ops
        as_t = lambda x: (x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))) \
            .to(device=dev, dtype=torch.float32).contiguous()
        obs, rets = as_t(batch['obs']), as_t(batch['estimate_returns']).reshape(-1)
        if dist.collectives_active():
            ne = int(algo.replay_buffer.env_nums)
            obs, rets = dist.gather_env_shards(obs, ne), dist.gather_env_shards(rets.view(-1, 1), ne).view(-1)
        B = int(obs.shape[0])
        v, tape = ops.mlp_forward(self.vf_layers, obs, self.act)
        d_v = _C.mse_value_loss(v.view(-1), rets, 2 * B, self._stat[10:11])       # 0.5 * mean((v - R)^2): d = (v - R) / B
        ops.mlp_backward(tape, d_v, grads=self.gviews[1], workspace=self._ws(B))
        self.vf_steps += 1
        _C.clip_adam(_C.adam_args(self.flat, self.grads, self.m, self.v, [self.P_vf], [algo.vf_optimizer.param_groups[0]['lr']],
                                  offset=self.P_pf, max_norm=0.5, eps=1e-5, step_count=self.vf_steps,
                                  norms_out=self._vf_norm.data_ptr()), dev)
        return {'Training/vf_loss': 0.5 * float(self._stat[10].item()) / B, 'grad_norm/vf': float(self._vf_norm.item())}
