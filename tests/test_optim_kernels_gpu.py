"""trl_clip_step_f32 / trl_clip_step_polyak_f32 (csrc/k_optim.hip) called directly, against the float64 restatement of
tests/_optim_ref.py.  Every element is compared against K * 2^-24 * its running magnitude with the K of that file (set on
the CPU, tests/test_optim_kernels_cpu.py); the buffers are bracketed by NaN canaries, and state buffers the options do not
use are canaries throughout."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _optim_ref as R                                                  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 67                                                                # canary elements on both sides = the element offset
CASES = [(R.RMSPROP, o) for o in R.RMSPROP_OPTIONS] + [(R.SGD, o) for o in R.SGD_OPTIONS]
IDS = ["%s-%s" % ("rmsprop" if k == R.RMSPROP else "sgd", ",".join("%s=%s" % kv for kv in o.items()) or "plain")
       for k, o in CASES]
# 1 / 255 / 256 / 257 elements, a group boundary inside a block, four groups, 128 blocks (the last self-ticking grid) and
# 129 blocks (the tick launch)
LAYOUTS = [(1,), (255,), (256,), (257,), (5, 300, 1), (64, 64, 64, 64), (32768,), (32769,)]
MODES = [(0.0, 1.0), (1e3, 1.0), (0.3, 1.0), (0.3, 0.5)]                # (max_norm, grad_scale): none, above, below the norm
LRS = [1e-2, 3e-3, 1e-3, 2e-2]


def spec_of(kind, o):
    if kind == R.RMSPROP:
        return ("rmsprop", o.get("alpha", 0.99), o.get("eps", 1e-8), o.get("momentum", 0.0), o.get("centered", False),
                o.get("weight_decay", 0.0))
    return ("sgd", o.get("momentum", 0.0), o.get("dampening", 0.0), o.get("nesterov", False), o.get("weight_decay", 0.0))


def fresh_state():
    return torch.tensor([0.0, 1.0, 1.0, 0.0], dtype=torch.float64, device=DEV)


def check_state(state, steps):
    s = state.cpu()
    assert s[:3].tolist() == [float(steps), 1.0, 1.0]                    # slot 0 only, exactly +1 per launch
    assert s[3:].view(torch.int32).tolist() == [0, 0]                    # the block counter is back at zero


class Bench:
    """Canary-bracketed device buffers of one case: params, grads and three state buffers of PAD + n + PAD floats."""

    def __init__(self, kind, opts, sizes, seed):
        self.kind, self.opts, self.sizes, self.n = kind, opts, list(sizes), int(sum(sizes))
        self.rng = np.random.default_rng(seed)
        self.p0 = self.rng.standard_normal(self.n).astype(np.float32)
        self.ref = R.OptRef(kind, self.p0, sizes, dtype=np.float64, **opts)
        self.used = [s is not None for s in self.ref.s] + [False] * (3 - len(self.ref.s))
        full = lambda: torch.full((self.n + 2 * PAD,), float("nan"), device=DEV)
        self.p, self.g, self.s = full(), full(), [full(), full(), full()]
        self.p[PAD:PAD + self.n] = torch.from_numpy(self.p0).to(DEV)
        for k in range(3):
            if self.used[k]:
                self.s[k][PAD:PAD + self.n] = 0.0
        self.norms = torch.full((5,), -7.0, device=DEV)
        self.lr_dev = torch.zeros(4, device=DEV)

    def args(self, lrs, max_norm, gs, state=None, device_lr=False, first_step=0):
        from torchrl_amd import _C
        if device_lr:
            self.lr_dev[:len(self.sizes)].copy_(torch.tensor([float(x) for x in lrs]))
        return _C.opt_args(spec_of(self.kind, self.opts), self.p, self.g, self.s, self.sizes,
                           [123.0] * len(self.sizes) if device_lr else lrs, offset=PAD, max_norm=max_norm, grad_scale=gs,
                           norms_out=self.norms.data_ptr(), step_state=None if state is None else state.data_ptr(),
                           device_lr=self.lr_dev.data_ptr() if device_lr else None, first_step=first_step)

    def draw(self, step):
        g = (self.rng.standard_normal(self.n) * (2.0 if step % 2 else 0.1)).astype(np.float32)
        self.g[PAD:PAD + self.n] = torch.from_numpy(g).to(DEV)
        return g

    def values(self):
        out = {"p": self.p[PAD:PAD + self.n].cpu().numpy()}
        for k in range(3):
            if self.used[k]:
                out["s%d" % k] = self.s[k][PAD:PAD + self.n].cpu().numpy()
        return out

    def check_canaries(self):
        for name, t in [("p", self.p), ("g", self.g)] + [("s%d" % k, self.s[k]) for k in range(3) if self.used[k]]:
            assert torch.isnan(t[:PAD]).all() and torch.isnan(t[PAD + self.n:]).all(), name
            assert torch.isfinite(t[PAD:PAD + self.n]).all(), name
        for k in range(3):
            if not self.used[k]:
                assert torch.isnan(self.s[k]).all(), "state%d is unused by these options and was written" % k

    def check(self, label, errlog):
        ratios = {k: v / R.K[self.kind][k] for k, v in R.error_ratios(self.values(), self.ref).items()}
        print("%s: err / bound %s" % (label, {k: round(v, 3) for k, v in ratios.items()}))
        for k, v in ratios.items():
            errlog("%s_%s_over_bound" % (label, k), v, 1.0)
        assert max(ratios.values()) <= 1.0, (label, ratios)
        self.check_canaries()


# ---------------------------------------------------------------- the step against the float64 restatement
@pytest.mark.parametrize("kind,opts", CASES, ids=IDS)
def test_three_chained_launches_vs_float64_restatement(kind, opts, errlog):
    """Every layout x clip mode, three chained launches each (SGD's first-step rule and both momentum forms); the learning
    rates from the device or the descriptor and the step from the device state or the host flag, in turn."""
    from torchrl_amd import _C
    worst = {}
    for li, sizes in enumerate(LAYOUTS):
        for mi, (max_norm, gs) in enumerate(MODES):
            b = Bench(kind, opts, sizes, 100 * li + mi)
            state = fresh_state() if (li + mi) % 2 == 0 else None
            device_lr = mi % 2 == 1
            for step in range(3):
                g = b.draw(step)
                lrs = [lr * (1.0 - 0.1 * step) for lr in LRS[:len(sizes)]]
                first = int(step == 0) if state is None else int(step != 0)      # (ignored where the device state says it)
                _C.clip_step(b.args(lrs, max_norm, gs, state, device_lr, first_step=first), DEV)
                r = b.ref.step(g, lrs, max_norm, gs)
                norms = b.norms.cpu().numpy()
                for k in range(len(sizes)):
                    if max_norm <= 0.0:
                        assert norms[k] == 0.0                           # no clipping: the norm pass is skipped, 0 is written
                    else:
                        assert norms[k] == pytest.approx(r["norms"][k], rel=1e-5)
                assert (norms[len(sizes):] == -7.0).all()                # nothing written behind the groups
            if state is not None:
                check_state(state, 3)
            label = "%s_mn%g_gs%g" % ("x".join(map(str, sizes)), max_norm, gs)
            b.check(label, errlog)
            assert not np.array_equal(b.values()["p"], b.p0)
            for k, v in R.error_ratios(b.values(), b.ref).items():
                worst[k] = max(worst.get(k, 0.0), v / R.K[kind][k])
    for k, v in worst.items():
        errlog("worst_%s_over_bound" % k, v, 1.0)


# ---------------------------------------------------------------- exact checks
@pytest.mark.parametrize("opts", [dict(), dict(centered=True)], ids=["plain", "centered"])
def test_zero_gradient_leaves_rmsprop_parameters_bit_identical(opts):
    from torchrl_amd import _C
    b = Bench(R.RMSPROP, opts, (5, 300, 1), 3)
    b.s[0][PAD:PAD + b.n] = torch.rand(b.n, device=DEV) + 0.5            # a square_avg with history
    b.g[PAD:PAD + b.n] = 0.0
    for max_norm in (0.0, 0.5):
        _C.clip_step(b.args(LRS[:3], max_norm, 1.0), DEV)
    assert np.array_equal(b.values()["p"], b.p0)
    b.check_canaries()


@pytest.mark.parametrize("n", [32768, 32769], ids=["last_block_ticks", "tick_launch"])
@pytest.mark.parametrize("kind,opts", [CASES[0], CASES[6]], ids=["rmsprop", "sgd-momentum"])
def test_step_state_advances_by_exactly_one_in_both_tick_modes(kind, opts, n):
    from torchrl_amd import _C
    b, state = Bench(kind, opts, (n,), 5), fresh_state()
    for step in range(4):
        b.draw(step)
        _C.clip_step(b.args(LRS[:1], 0.5, 1.0, state), DEV)
        check_state(state, step + 1)
    b.check_canaries()


@pytest.mark.parametrize("sizes", LAYOUTS + [(4097, 3, 64, 8192)], ids=lambda s: "x".join(map(str, s)))
def test_norms_carry_the_bits_of_the_adam_launch(sizes):
    from torchrl_amd import _C
    b = Bench(R.SGD, {}, sizes, 9)
    b.draw(1)
    for max_norm, gs in MODES[1:]:
        _C.clip_step(b.args(LRS[:len(sizes)], max_norm, gs), DEV)
        got = b.norms.cpu().numpy().copy()
        p, m, v = (torch.zeros(b.n + 2 * PAD, device=DEV) for _ in range(3))
        norms = torch.full((5,), -7.0, device=DEV)
        a = _C.adam_args(p, b.g, m, v, list(sizes), LRS[:len(sizes)], offset=PAD, max_norm=max_norm, grad_scale=gs,
                         norms_out=norms.data_ptr(), step_count=1)
        _C.clip_adam(a, DEV)
        assert np.array_equal(got, norms.cpu().numpy()) and (got[:len(sizes)] > 0).all()


@pytest.mark.parametrize("kind,opts", [(R.RMSPROP, dict(centered=True, momentum=0.9)), (R.SGD, dict(momentum=0.9, nesterov=True))],
                         ids=["rmsprop-centered-momentum", "sgd-nesterov"])
def test_graph_replay_gives_the_bits_of_eager_launches(kind, opts):
    """One captured launch replayed three times against three eager launches from the same start (one stream, no branches):
    the step state and the learning rates live on the device, so nothing in the launch changes between replays."""
    from torchrl_amd import _C
    results = []
    for captured in (False, True):
        b, state = Bench(kind, opts, (5, 300, 1), 21), fresh_state()
        b.draw(1)
        launch = lambda: _C.clip_step(b.args(LRS[:3], 0.3, 1.0, state, device_lr=False), DEV)
        if captured:
            torch.cuda.synchronize()
            graph, _ = _C.capture_graph(launch)
            for _ in range(3):
                graph.replay()
        else:
            for _ in range(3):
                launch()
        torch.cuda.synchronize()
        check_state(state, 3)
        b.check_canaries()
        results.append(b.values())
    assert results[0].keys() == results[1].keys()
    for name in results[0]:
        assert np.array_equal(results[0][name], results[1][name]), name
    assert not np.array_equal(results[0]["p"], b.p0)


# ---------------------------------------------------------------- the Polyak variant
@pytest.mark.parametrize("n", [300, 32769], ids=["self_tick", "polyak_ticks"])
@pytest.mark.parametrize("kind,opts", [CASES[3], CASES[8]], ids=["rmsprop-all", "sgd-nesterov"])
def test_polyak_variant_files_the_ring_and_steps_the_target(kind, opts, n, errlog):
    from torchrl_amd import _C
    slots, raw_bytes, tau = 3, 52, 0.005
    b, state = Bench(kind, opts, (n,), 31), fresh_state()
    rs = np.random.RandomState(n)
    target = torch.full((n + 2 * PAD,), float("nan"), device=DEV)
    target[PAD:PAD + n] = torch.from_numpy(rs.randn(n).astype(np.float32)).to(DEV)
    ring = torch.full((slots, raw_bytes), 0xAB, dtype=torch.uint8, device=DEV)
    want_ring = ring.cpu().clone()
    worst = 0.0
    for k in range(4):
        g = b.draw(k)
        raw = torch.from_numpy(rs.randint(0, 256, raw_bytes).astype(np.uint8))
        t0 = target[PAD:PAD + n].cpu().numpy()
        _C.clip_step_polyak(b.args(LRS[:1], 0.5, 1.0, state), target[PAD:PAD + n], b.p[PAD:PAD + n], tau, DEV,
                            file=(raw.to(DEV), ring))
        torch.cuda.synchronize()
        b.ref.step(g, LRS[:1], 0.5, 1.0)
        want_ring[k % slots] = raw                                       # row (steps taken before) mod slots, the others untouched
        assert torch.equal(ring.cpu(), want_ring), k
        check_state(state, k + 1)
        want = R.polyak(t0, b.values()["p"], tau)                        # float64 Polyak of the STEPPED parameters
        got = target[PAD:PAD + n].cpu().numpy()
        # an ulp at the magnitude of the two terms, |t| + |s| (`polyak_bound`'s quantity in _ppo_update_ref.py): where t is
        # small beside tau s the sum cancels, and the rounding of tau s alone is many ulps OF THE RESULT in any float32
        # evaluation of the formula
        mag = (np.abs(t0.astype(np.float64)) + np.abs(b.values()["p"].astype(np.float64))).astype(np.float32)
        ulps = np.abs(got.astype(np.float64) - want) / np.spacing(mag).astype(np.float64)
        worst = max(worst, float(ulps.max()))
    errlog("polyak_ulps", worst, 2.0)
    assert worst <= 2.0
    assert torch.isnan(target[:PAD]).all() and torch.isnan(target[PAD + n:]).all()
    b.check("polyak_chain", errlog)


# ---------------------------------------------------------------- refusals
def test_refusals_return_einval():
    from torchrl_amd import _C
    import ctypes as C
    lib, stream = _C.lib(), _C.stream_ptr(torch.device(DEV))
    EINVAL = -1

    def rc(kind, opts, edit=None, polyak=None):
        b = Bench(kind, opts, (8,), 1)
        b.g[PAD:PAD + 8] = 1.0
        a = b.args(LRS[:1], 0.0, 1.0)
        if edit:
            edit(a)
        if polyak is None:
            code = lib.trl_clip_step_f32(C.byref(a), stream)
        else:
            tgt, raw, ring = torch.zeros(8, device=DEV), torch.zeros(8, dtype=torch.uint8, device=DEV), \
                torch.zeros(3, 8, dtype=torch.uint8, device=DEV)
            code = lib.trl_clip_step_polyak_f32(C.byref(a), tgt.data_ptr(), b.p[PAD:].data_ptr(), 8, 0.5, raw.data_ptr(), 8,
                                                ring.data_ptr(), 3, stream)
        torch.cuda.synchronize()
        if code != 0:
            assert np.array_equal(b.values()["p"], b.p0)                 # a refused launch touches nothing
            assert _C.lib().trl_last_error()
        return code

    def null(field):
        return lambda a: setattr(a, field, None)

    assert rc(R.RMSPROP, {}) == 0 and rc(R.SGD, dict(momentum=0.9)) == 0
    assert rc(R.RMSPROP, {}, null("state0")) == EINVAL
    assert rc(R.RMSPROP, dict(momentum=0.9), null("state1")) == EINVAL
    assert rc(R.RMSPROP, dict(centered=True), null("state2")) == EINVAL
    assert rc(R.SGD, dict(momentum=0.9), null("state0")) == EINVAL
    assert rc(R.SGD, {}, null("state0")) == 0                            # (SGD without momentum keeps no state)
    assert rc(R.SGD, {}, null("params")) == EINVAL and rc(R.SGD, {}, null("grads")) == EINVAL
    for n_groups in (0, 5, -1):
        assert rc(R.SGD, {}, lambda a: setattr(a, "n_groups", n_groups)) == EINVAL
    assert rc(R.SGD, {}, lambda a: setattr(a, "nesterov", 1)) == EINVAL                       # zero momentum
    assert rc(R.SGD, dict(momentum=0.9, dampening=0.1), lambda a: setattr(a, "nesterov", 1)) == EINVAL
    assert rc(R.SGD, {}, lambda a: setattr(a, "kind", 3)) == EINVAL
    assert rc(R.RMSPROP, {}, polyak=True) == EINVAL                      # a ring without the step state
