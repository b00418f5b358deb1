"""The numpy restatement of trl_clip_step_f32 (tests/_optim_ref.py) against torch.optim.RMSprop / torch.optim.SGD in
float64, the constants K of the GPU bound from its float32 run, and the host side of the optimiser choice: the descriptor's
layout, `step_spec`, the state binding of the flat homes.  No GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _optim_ref as R                                                  # noqa: E402
from torchrl_amd import _C                                              # noqa: E402
from torchrl_amd.algo import _optim                                     # noqa: E402

CASES = [(R.RMSPROP, o) for o in R.RMSPROP_OPTIONS] + [(R.SGD, o) for o in R.SGD_OPTIONS]
IDS = ["%s-%s" % ("rmsprop" if k == R.RMSPROP else "sgd", ",".join("%s=%s" % kv for kv in o.items()) or "plain")
       for k, o in CASES]
LR = 1e-2


# ------------------------------------------------------------------ the restatement is torch's step
@pytest.mark.parametrize("clip", [0.0, 0.5], ids=["noclip", "clip"])
@pytest.mark.parametrize("kind,opts", CASES, ids=IDS)
def test_restatement_is_torch_optim_in_float64(kind, opts, clip):
    rng = np.random.default_rng(7)
    n = 37
    p0 = rng.standard_normal(n)
    p = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    cls = torch.optim.RMSprop if kind == R.RMSPROP else torch.optim.SGD
    opt = cls([p], lr=LR, **opts)
    ref = R.OptRef(kind, p0, [n], dtype=np.float64, exact_hyper=True, **opts)
    for step in range(5):
        g = rng.standard_normal(n) * (3.0 if step % 2 else 0.05)         # norms above and below the clip
        p.grad = torch.tensor(g, dtype=torch.float64)
        if clip:
            torch.nn.utils.clip_grad_norm_([p], clip)
        opt.step()
        ref.step(g, [LR], max_norm=clip)
        want = {"p": p.detach().numpy()}
        for k, name in enumerate(R.STATE_NAMES[kind]):
            if ref.s[k] is not None:
                want["s%d" % k] = opt.state[p][name].numpy()
        assert set(want) == set(ref.values())
        for name, w in want.items():
            got = ref.values()[name]
            assert np.abs(got - w).max() <= 1e-12 * max(1e-300, np.abs(w).max()), (step, name)
    unused = [name for k, name in enumerate(R.STATE_NAMES[kind]) if ref.s[k] is None]
    assert not any(name in opt.state[p] and opt.state[p][name] is not None for name in unused)


# ------------------------------------------------------------------ the constants of the GPU bound
def k_needed_on_cpu(kind, opts, margin=4.0):
    """margin x the largest err / (u M_x) of the float32 run against the float64 one, per stored quantity, over the clip
    modes, a gradient scale and two group layouts; five chained steps each."""
    need = {}
    for sizes in ([5, 300, 1], [64, 64, 64, 64], [2000]):
        n = int(np.sum(sizes))
        for max_norm, gs in ((0.0, 1.0), (1e3, 1.0), (0.3, 1.0), (0.3, 0.5)):
            rng = np.random.default_rng(11 + n)
            p0 = rng.standard_normal(n).astype(np.float32)
            lo, hi = (R.OptRef(kind, p0, sizes, dtype=dt, **opts) for dt in (np.float32, np.float64))
            for step in range(5):
                g = (rng.standard_normal(n) * (2.0 if step % 2 else 0.1)).astype(np.float32)
                lrs = [LR, 3e-3, 1e-3, 2e-2][:len(sizes)]
                lo.step(g, lrs, max_norm, gs)
                hi.step(g, lrs, max_norm, gs)
                for name, r in R.error_ratios(lo, hi).items():
                    need[name] = max(need.get(name, 0.0), margin * r)
    return need


@pytest.mark.parametrize("kind,opts", CASES, ids=IDS)
def test_bound_constants_cover_the_float32_restatement_with_margin_4(kind, opts):
    need = k_needed_on_cpu(kind, opts)
    print("K needed (margin 4)", IDS[CASES.index((kind, opts))], {k: round(v, 3) for k, v in need.items()})
    for name, v in need.items():
        assert np.isfinite(v) and v <= R.K[kind][name], (name, v, R.K[kind][name])


def test_bound_constants_are_the_cpu_ratios_not_looser():
    """Each K is the power of two at or above the largest margin-4 ratio of any option set (never below 1)."""
    worst = {R.RMSPROP: {}, R.SGD: {}}
    for kind, opts in CASES:
        for name, v in k_needed_on_cpu(kind, opts).items():
            worst[kind][name] = max(worst[kind].get(name, 0.0), v)
    for kind in worst:
        assert {n: R.pow2_at_least(v) for n, v in worst[kind].items()} == R.K[kind], worst[kind]


# ------------------------------------------------------------------ descriptor layout
def test_opt_descriptor_layout_matches_c(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "trl_hip.h"', 'int main(void){',
             'printf("size %zu\\n", sizeof(trl_opt_t));', 'printf("kinds %d\\n", TRL_OPT_RMSPROP * 10 + TRL_OPT_SGD);']
    for fname, _ in _C.OptArgs._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(trl_opt_t, %s));' % (fname, fname))
    lines.append("return 0;}")
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)]).decode().splitlines() if ln.strip())
    assert int(got["size"]) == ctypes.sizeof(_C.OptArgs)
    assert int(got["kinds"]) == _C.OPT_RMSPROP * 10 + _C.OPT_SGD == R.RMSPROP * 10 + R.SGD
    for fname, _ in _C.OptArgs._fields_:
        assert int(got[fname]) == getattr(_C.OptArgs, fname).offset, fname


def test_opt_args_carries_the_spec_and_offsets():
    flat, grads, s0, s2 = (torch.zeros(10) for _ in range(4))
    a = _C.opt_args(("rmsprop", 0.95, 0.01, 0.0, True, 1e-2), flat, grads, [s0, None, s2], [3, 4], [1e-3, 2e-3], offset=2,
                    max_norm=0.5, grad_scale=0.5)
    assert a.kind == _C.OPT_RMSPROP and a.params == flat.data_ptr() + 8 and a.state0 == s0.data_ptr() + 8
    assert a.state1 is None and a.state2 == s2.data_ptr() + 8 and a.n_groups == 2 and list(a.group_sizes)[:2] == [3, 4]
    assert (a.alpha, a.eps, a.centered, a.momentum) == (np.float32(0.95), np.float32(0.01), 1, 0.0)
    assert a.weight_decay == np.float32(1e-2) and a.max_norm == 0.5 and a.grad_scale == 0.5
    b = _C.opt_args(("sgd", 0.9, 0.0, True, 0.0), flat, grads, [s0], [10], [1e-3], first_step=1)
    assert b.kind == _C.OPT_SGD and b.nesterov == 1 and b.momentum == np.float32(0.9) and b.first_step == 1
    assert b.state1 is None and b.state2 is None
    with pytest.raises(_C.TrlError, match="adam_args"):
        _C.opt_args(("adam", 1e-8), flat, grads, [s0], [10], [1e-3])


# ------------------------------------------------------------------ step_spec
def _params():
    return [torch.nn.Parameter(torch.zeros(3))]


def test_step_spec_reads_class_and_first_group():
    assert _optim.step_spec(torch.optim.Adam(_params(), lr=1e-3, eps=1e-5)) == ("adam", 1e-5)
    assert _optim.step_spec(torch.optim.RMSprop(_params(), lr=1e-3)) == ("rmsprop", 0.99, 1e-8, 0.0, False, 0.0)
    assert _optim.step_spec(torch.optim.RMSprop(_params(), lr=1e-3, alpha=0.95, eps=0.01, centered=True, momentum=0.95)) \
        == ("rmsprop", 0.95, 0.01, 0.95, True, 0.0)
    assert _optim.step_spec(torch.optim.SGD(_params(), lr=1e-3)) == ("sgd", 0.0, 0.0, False, 0.0)
    assert _optim.step_spec(torch.optim.SGD(_params(), lr=1e-3, momentum=0.9, nesterov=True, weight_decay=1e-2)) \
        == ("sgd", 0.9, 0.0, True, 1e-2)
    hash(_optim.step_spec(torch.optim.SGD(_params(), lr=1e-3)))          # (joins the graph-cache keys)


@pytest.mark.parametrize("make", [
    lambda: torch.optim.AdamW(_params(), lr=1e-3),
    lambda: torch.optim.Adagrad(_params(), lr=1e-3),
    lambda: torch.optim.RMSprop(_params(), lr=1e-3, maximize=True),
    lambda: torch.optim.SGD(_params(), lr=1e-3, maximize=True),
    lambda: torch.optim.RMSprop(_params(), lr=1e-3, foreach=True),
    lambda: torch.optim.SGD(_params(), lr=1e-3, foreach=False),
    lambda: torch.optim.RMSprop(_params(), lr=1e-3, capturable=True),
    lambda: torch.optim.RMSprop(_params(), lr=1e-3, differentiable=True),
    lambda: torch.optim.SGD(_params(), lr=1e-3, differentiable=True),
], ids=["adamw", "adagrad", "rmsprop-maximize", "sgd-maximize", "rmsprop-foreach", "sgd-foreach", "rmsprop-capturable",
        "rmsprop-differentiable", "sgd-differentiable"])
def test_step_spec_refuses_what_has_no_kernel(make):
    with pytest.raises(_C.TrlError):
        _optim.step_spec(make())


# ------------------------------------------------------------------ flat homes bind torch's state names
def _mlp(*widths):
    return torch.nn.Sequential(*[torch.nn.Linear(a, b) for a, b in zip(widths[:-1], widths[1:])])


@pytest.mark.parametrize("cls,opts,names,third", [
    (torch.optim.RMSprop, {}, {"step": None, "square_avg": "m"}, False),
    (torch.optim.RMSprop, dict(momentum=0.9), {"step": None, "square_avg": "m", "momentum_buffer": "v"}, False),
    (torch.optim.RMSprop, dict(centered=True), {"step": None, "square_avg": "m", "grad_avg": "c"}, True),
    (torch.optim.RMSprop, dict(centered=True, momentum=0.9),
     {"step": None, "square_avg": "m", "momentum_buffer": "v", "grad_avg": "c"}, True),
    (torch.optim.SGD, {}, {}, False),
    (torch.optim.SGD, dict(momentum=0.9), {"momentum_buffer": "m"}, False),
], ids=["rmsprop", "rmsprop-momentum", "rmsprop-centered", "rmsprop-centered-momentum", "sgd", "sgd-momentum"])
def test_flat_home_binds_the_state_under_torchs_names(cls, opts, names, third):
    from torchrl_amd.algo.off_policy._engine import FlatHome
    nets = [_mlp(5, 7, 3), _mlp(8, 4, 1)]
    optimizers = [cls(n.parameters(), lr=1e-3, **opts) for n in nets]
    plists = [list(n.parameters()) for n in nets]
    home = FlatHome(plists, optimizers, list(_mlp(8, 4, 1).parameters()))
    assert (home.c is not None) == third and (home.c is None or home.c.shape == home.flat.shape)
    off = 0
    for opt, pl in zip(optimizers, plists):
        for p in pl:
            state = opt.state[p]
            assert sorted(state) == sorted(names) and "exp_avg" not in state
            for name, buf in names.items():
                if buf is not None:
                    assert state[name].data_ptr() == getattr(home, buf).data_ptr() + 4 * off and state[name].shape == p.shape
            off += p.numel()
        keys = set(k for s in opt.state_dict()["state"].values() for k in s)
        assert keys == set(names)


def test_flat_home_refuses_an_optimiser_without_a_kernel():
    from torchrl_amd.algo.off_policy._engine import FlatHome
    net = _mlp(3, 2)
    with pytest.raises(_C.TrlError, match="Adagrad"):
        FlatHome([list(net.parameters())], [torch.optim.Adagrad(net.parameters(), lr=1e-3)], list(_mlp(3, 2).parameters()))
