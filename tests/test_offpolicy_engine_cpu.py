"""The host plumbing the fused off-policy engines share (algo/off_policy/_engine.py, _C.adam_args) on CPU tensors: the
eager -> captured -> replayed rule with a stand-in for the capture, the flat-buffer home, the AdamArgs builder against the
field-by-field fills it replaced, and the copy of a sampled batch into the fixed-address inputs.  CPU only."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

from torchrl_amd import _C, dist
from torchrl_amd.algo.off_policy._engine import FlatHome, GraphCache, load_static


# ------------------------------------------------------------------ GraphCache
class _Graph:
    def __init__(self):
        self.replays = 0

    def replay(self):
        self.replays += 1


@pytest.fixture
def captured(monkeypatch):
    """`_C.capture_graph` replaced by a stand-in that runs the launches once; the list of graphs it handed out."""
    graphs = []

    def fake(launches):
        launches()
        graphs.append(_Graph())
        return graphs[-1], None
    monkeypatch.delenv("TRL_NO_GRAPH", raising=False)
    monkeypatch.setattr(dist, "collectives_active", lambda: False)
    monkeypatch.setattr(_C, "capture_graph", fake)
    return graphs


class _Counter:
    def __init__(self):
        self.n = 0

    def __call__(self):
        self.n += 1


def test_graph_cache_runs_eagerly_then_captures_then_replays(captured):
    cache, a, b = GraphCache(8), _Counter(), _Counter()
    key_a, key_b = (96, True, (1e-3, 1e-3)), ("epoch", 3, 96)
    seen = []
    for _ in range(4):
        cache.run(key_a, a)
        seen.append((a.n, captured[0].replays if captured else 0))
    assert seen == [(1, 0), (2, 1), (2, 2), (2, 3)]                      # the capture itself runs the launches once
    assert len(cache) == 1 and key_a in cache and key_b not in cache
    cache.run(key_b, b)                                                  # a second key starts from its own first visit
    assert (b.n, len(captured), len(cache), a.n) == (1, 1, 1, 2)
    cache.run(key_b, b)
    cache.run(key_b, b)
    assert (b.n, captured[1].replays, captured[0].replays) == (2, 2, 3)
    assert len(cache) == 2 and list(cache) == [key_a, key_b] and cache[key_b] is captured[1]
    assert any(k[0] == "epoch" for k in cache if isinstance(k, tuple))


def test_full_graph_cache_stays_eager_and_does_not_remember_the_key(captured):
    cache, fns = GraphCache(2), [_Counter() for _ in range(3)]
    for _ in range(2):
        cache.run(("a",), fns[0])
        cache.run(("b",), fns[1])
    assert len(cache) == 2 and cache.has_room(("a",)) and cache.has_room(("b",)) and not cache.has_room(("c",))
    for n in range(1, 4):
        cache.run(("c",), fns[2])
        assert fns[2].n == n and len(captured) == 2 and ("c",) not in cache
    cache.run(("a",), fns[0])                                            # the held graphs still replay
    assert fns[0].n == 2 and captured[0].replays == 2
    cache.clear()
    assert len(cache) == 0 and list(cache) == [] and cache.has_room(("c",))
    cache.run(("c",), fns[2])                                            # had the full cache marked it seen, this would capture
    assert fns[2].n == 4 and len(captured) == 2 and len(cache) == 0
    cache.run(("c",), fns[2])
    assert fns[2].n == 5 and len(captured) == 3 and list(cache) == [("c",)]


def test_clear_drops_graphs_and_seen_keys_together(captured):
    cache, f = GraphCache(4), _Counter()
    cache.run(("k",), f)                                                 # seen, not captured yet
    cache.clear()
    cache.run(("k",), f)                                                 # a first visit again: eager
    assert f.n == 2 and not captured and len(cache) == 0
    cache.run(("k",), f)
    assert f.n == 3 and len(captured) == 1 and len(cache) == 1
    cache.clear()
    assert len(cache) == 0 and ("k",) not in cache
    cache.run(("k",), f)
    assert f.n == 4 and len(captured) == 1 and captured[0].replays == 1


@pytest.mark.parametrize("switch", ["env", "collectives"])
def test_graph_cache_stays_eager_without_graphs_or_between_ranks(captured, monkeypatch, switch):
    if switch == "env":
        monkeypatch.setenv("TRL_NO_GRAPH", "1")
    else:
        monkeypatch.setattr(dist, "collectives_active", lambda: True)
    cache, f = GraphCache(8), _Counter()
    for n in range(1, 5):
        cache.run(("k",), f)
        assert f.n == n and len(cache) == 0 and not captured
    monkeypatch.delenv("TRL_NO_GRAPH", raising=False)
    monkeypatch.setattr(dist, "collectives_active", lambda: False)
    cache.run(("k",), f)                                                 # nothing was recorded meanwhile: a first visit
    assert f.n == 5 and not captured
    cache.run(("k",), f)
    assert f.n == 6 and len(captured) == 1 and len(cache) == 1


# ------------------------------------------------------------------ FlatHome
def _mlp(*widths):
    return nn.Sequential(*[nn.Linear(a, b) for a, b in zip(widths[:-1], widths[1:])])


def _homed(keep=None, seed=0):
    torch.manual_seed(seed)
    nets = [_mlp(5, 7, 3), _mlp(8, 4, 1), _mlp(8, 4, 1)]
    opts = [torch.optim.Adam(n.parameters(), lr=1e-3) for n in nets]
    plists = [list(n.parameters()) for n in nets]
    before = [p.detach().clone() for pl in plists for p in pl]
    return nets, opts, plists, before, FlatHome(plists, opts, list(_mlp(8, 4, 1).parameters()), keep=keep)


def test_flat_home_parameters_gradients_and_moments_are_views_at_the_cumulative_offsets():
    nets, opts, plists, before, home = _homed()
    sizes = [5 * 7 + 7 + 7 * 3 + 3, 8 * 4 + 4 + 4 + 1, 8 * 4 + 4 + 4 + 1]
    assert home.sizes == sizes and list(home.offsets) == [0, 66, 107, 148] and home.flat.numel() == 148
    assert all(t.shape == home.flat.shape and t.dtype == torch.float32 for t in (home.grads, home.m, home.v))
    assert not home.grads.any() and not home.m.any() and not home.v.any()
    params = [p for pl in plists for p in pl]
    assert len(home.views) == len(params) == 12
    off = 0
    for p, old, g in zip(params, before, home.views):
        assert p.data_ptr() == home.flat.data_ptr() + 4 * off and torch.equal(p.detach(), old)
        assert g.data_ptr() == home.grads.data_ptr() + 4 * off and g.shape == p.shape
        off += p.numel()
    off = 0
    for opt, pl in zip(opts, plists):
        assert len(opt.state) == len(pl)
        for p in pl:
            state = opt.state[p]
            assert sorted(state) == ["exp_avg", "exp_avg_sq", "step"]
            assert state["step"].device.type == "cpu" and state["step"].shape == () and float(state["step"]) == 0.0
            assert state["exp_avg"].data_ptr() == home.m.data_ptr() + 4 * off and state["exp_avg"].shape == p.shape
            assert state["exp_avg_sq"].data_ptr() == home.v.data_ptr() + 4 * off and state["exp_avg_sq"].shape == p.shape
            off += p.numel()
    home.flat.copy_(torch.arange(148.0))                                 # a write through the buffer shows in the modules
    assert torch.equal(nets[0][0].weight.detach(), torch.arange(35.0).view(7, 5))
    assert torch.equal(nets[1][0].bias.detach(), torch.arange(66.0 + 32, 66.0 + 36))
    assert float(nets[2][1].bias.detach()) == 147.0
    home.grads.copy_(torch.arange(148.0))
    pairs = home.pairs()
    assert [len(pr) for pr in pairs] == [2, 2, 2]
    assert [t for pr in pairs for wb in pr for t in wb] == home.views
    gw, gb = pairs[1][1]
    assert gw.shape == (1, 4) and gb.shape == (1,) and gw.flatten().tolist() == [102.0, 103.0, 104.0, 105.0]
    assert float(gb) == 106.0


def test_flat_home_with_one_optimizer_for_one_list_and_its_target():
    torch.manual_seed(1)
    net, target = _mlp(3, 2, 2), _mlp(3, 2, 2)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    want = torch.cat([p.detach().reshape(-1) for p in target.parameters()])
    home = FlatHome([list(net.parameters())], [opt], list(target.parameters()))
    assert torch.equal(home.tflat, want) and home.tflat.data_ptr() != home.flat.data_ptr()
    assert target[1].weight.data_ptr() == home.tflat.data_ptr() + 4 * 8 and len(opt.state) == 4       # targets: no state
    assert home.sizes == [14] and list(home.offsets) == [0, 14] and len(home.pairs()) == 1 and len(home.pairs()[0]) == 2
    assert opt.state[net[1].bias]["exp_avg_sq"].data_ptr() == home.v.data_ptr() + 4 * 12


def test_flat_home_keeps_moments_of_a_matching_size_and_zeroes_others():
    m, v = torch.arange(148.0), -torch.arange(148.0)
    _, opts, plists, _, home = _homed(keep=(m, v))
    assert torch.equal(home.m, torch.arange(148.0)) and torch.equal(home.v, -torch.arange(148.0))
    assert not home.grads.any()
    last = plists[2][-1]
    assert float(opts[2].state[last]["exp_avg"]) == 147.0 and float(opts[2].state[last]["exp_avg_sq"]) == -147.0
    assert opts[2].state[last]["exp_avg"].data_ptr() == home.m.data_ptr() + 4 * 147
    _, opts, plists, _, home = _homed(keep=(torch.ones(147), torch.ones(147)))
    assert home.m.numel() == 148 and not home.m.any() and not home.v.any()
    assert float(opts[0].state[plists[0][0]]["exp_avg"].abs().sum()) == 0.0


# ------------------------------------------------------------------ adam_args
def _fields(a):
    out = {}
    for name, _ in _C.AdamArgs._fields_:
        v = getattr(a, name)
        out[name] = list(v) if isinstance(v, ctypes.Array) else v
    return out


@pytest.fixture
def bufs():
    flat, grads, m, v = (torch.zeros(300) for _ in range(4))
    norms = torch.zeros(3)
    step_state = torch.zeros(3, 4, dtype=torch.float64)
    return flat, grads, m, v, norms, step_state


def test_adam_args_equals_the_sac_fill(bufs):
    flat, grads, m, v, norms, step_state = bufs
    sizes, lrs, clip, world = [100, 120, 80], (3e-4, 1e-3, 1e-3), 0.5, 2
    a = _C.AdamArgs()                                                    # _FusedSAC._tail, field by field
    a.params, a.grads, a.exp_avg, a.exp_avg_sq = flat.data_ptr(), grads.data_ptr(), m.data_ptr(), v.data_ptr()
    a.n_groups = len(sizes)
    for k, size in enumerate(sizes):
        a.group_sizes[k] = size
    for k, lr in enumerate(lrs):
        a.group_lr[k] = lr
    a.max_norm = float(clip)
    a.beta1, a.beta2, a.eps = 0.9, 0.999, 1e-8
    a.grad_scale = 1.0 / world
    a.step_count, a.norms_out = 0, norms.data_ptr()
    a.step_state = step_state.data_ptr()
    got = _C.adam_args(flat, grads, m, v, sizes, lrs, max_norm=float(clip), grad_scale=1.0 / world,
                       norms_out=norms.data_ptr(), step_state=step_state.data_ptr())
    assert _fields(got) == _fields(a)
    assert got.n_groups == 3 and list(got.group_sizes) == [100, 120, 80, 0] and got.device_state == 0 and got.device_lr is None


@pytest.mark.parametrize("k", [1, 2])
def test_adam_args_equals_the_detac_fill_at_an_offset(bufs, k):
    flat, grads, m, v, norms, step_state = bufs
    sizes, offsets, lr = [100, 120, 80], np.array([0, 100, 220, 300]), 1e-3
    a = _C.AdamArgs()                                                    # _FusedDetAC._adam, field by field
    o = int(offsets[k]) * 4
    a.params, a.grads = flat.data_ptr() + o, grads.data_ptr() + o
    a.exp_avg, a.exp_avg_sq = m.data_ptr() + o, v.data_ptr() + o
    a.n_groups = 1
    a.group_sizes[0] = sizes[k]
    a.group_lr[0] = lr
    a.max_norm = 0.0                                                     # grad_clip None
    a.beta1, a.beta2, a.eps, a.grad_scale = 0.9, 0.999, 1e-8, 1.0 / 1
    a.step_count, a.norms_out = 0, norms.data_ptr() + 4 * k
    a.step_state = step_state.data_ptr() + 32 * k
    got = _C.adam_args(flat, grads, m, v, [sizes[k]], [lr], offset=offsets[k], max_norm=0.0, grad_scale=1.0,
                       norms_out=norms.data_ptr() + 4 * k, step_state=step_state.data_ptr() + 32 * k)
    assert _fields(got) == _fields(a)
    assert got.params == flat[offsets[k]:].data_ptr() and got.exp_avg_sq == v[offsets[k]:].data_ptr()
    assert got.step_state == step_state[k].data_ptr() and got.norms_out == norms[k:].data_ptr()


@pytest.mark.parametrize("info,grad_scale", [({"eps": 1.5e-4}, 0.25), ({}, 1.0)])      # DQN on four ranks; Bootstrapped DQN
def test_adam_args_equals_the_dqn_fills(bufs, info, grad_scale):
    flat, grads, m, v, _, step_state = bufs
    lr = 6.25e-5
    a = _C.AdamArgs()                                                    # _FusedDQN._sequence, field by field
    a.params, a.grads, a.exp_avg, a.exp_avg_sq = flat.data_ptr(), grads.data_ptr(), m.data_ptr(), v.data_ptr()
    a.n_groups = 1
    a.group_sizes[0] = flat.numel()
    a.group_lr[0] = lr
    a.max_norm, a.beta1, a.beta2 = 0.0, 0.9, 0.999
    a.eps = float(info.get("eps", 1e-8))
    a.grad_scale, a.norms_out = grad_scale, None
    a.step_count, a.step_state = 0, step_state.data_ptr()
    got = _C.adam_args(flat, grads, m, v, [flat.numel()], [lr], eps=float(info.get("eps", 1e-8)), grad_scale=grad_scale,
                       step_state=step_state.data_ptr())
    assert _fields(got) == _fields(a)
    assert got.norms_out is None and got.eps == np.float32(info.get("eps", 1e-8)) and got.max_norm == 0.0


def test_adam_args_defaults():
    t = torch.zeros(8)
    a = _C.adam_args(t, t, t, t, [8], [1e-3], step_count=7)
    assert (a.beta1, a.beta2, a.eps) == (np.float32(0.9), np.float32(0.999), np.float32(1e-8))
    assert (a.max_norm, a.grad_scale, a.step_count, a.norms_out, a.step_state) == (0.0, 1.0, 7, None, None)


# ------------------------------------------------------------------ load_static
def test_load_static_coerces_dtype_and_shape_and_skips_what_is_in_place():
    B = 6
    st = {"obs": torch.zeros(B, 3), "next_obs": torch.zeros(B, 3), "acts": torch.zeros(B, 1), "rewards": torch.zeros(B, 1),
          "terminals": torch.zeros(B, 1), "eps1": torch.full((B, 2), 7.0)}
    addresses = {k: t.data_ptr() for k, t in st.items()}
    st["next_obs"].fill_(3.0)                                            # what a replay gather wrote there already
    batch = dict(obs=np.arange(B * 3, dtype=np.float64).reshape(B, 3) / 3.0, next_obs=st["next_obs"],
                    acts=torch.arange(B, dtype=torch.int64), rewards=[[0.5]] * B,
                    terminals=torch.ones(B, dtype=torch.float64))
    copies = []
    real = torch.Tensor.copy_

    def spy(self, src, non_blocking=False):
        copies.append((self.data_ptr(), non_blocking))
        return real(self, src, non_blocking=non_blocking)
    with pytest.MonkeyPatch.context() as m:
        m.setattr(torch.Tensor, "copy_", spy)
        load_static(st, batch, ("obs", "next_obs", "acts", "rewards", "terminals"))
    assert [c[0] for c in copies] == [addresses[k] for k in ("obs", "acts", "rewards", "terminals")]     # not next_obs
    assert all(c[1] for c in copies)
    assert {k: t.data_ptr() for k, t in st.items()} == addresses
    assert all(t.dtype == torch.float32 for t in st.values())
    assert torch.equal(st["obs"], torch.from_numpy((np.arange(B * 3, dtype=np.float64).reshape(B, 3) / 3.0).astype(np.float32)))
    assert torch.equal(st["next_obs"], torch.full((B, 3), 3.0))
    assert st["acts"].shape == (B, 1) and st["acts"].view(-1).tolist() == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]       # (B,) -> (B, 1)
    assert st["rewards"].view(-1).tolist() == [0.5] * B and st["terminals"].view(-1).tolist() == [1.0] * B
    assert torch.equal(st["eps1"], torch.full((B, 2), 7.0))              # a key that was not asked for


def test_load_static_keeps_uint8_frames_uint8():
    st = {"obs": torch.zeros(2, 1, 3, 3, dtype=torch.uint8), "acts": torch.zeros(2, 1)}
    frames = torch.arange(18, dtype=torch.uint8).view(2, 1, 3, 3) + 200
    load_static(st, {"obs": frames, "acts": np.array([[2], [0]])}, ("obs", "acts"))
    assert st["obs"].dtype == torch.uint8 and torch.equal(st["obs"], frames) and st["obs"] is not frames
    assert st["acts"].dtype == torch.float32 and st["acts"].view(-1).tolist() == [2.0, 0.0]
    load_static(st, {"obs": frames.to(torch.int64).view(2, 9) - 100}, ("obs",))     # coerced to the static dtype and shape
    assert st["obs"].dtype == torch.uint8 and st["obs"].shape == (2, 1, 3, 3) and int(st["obs"][1, 0, 2, 2]) == 117
