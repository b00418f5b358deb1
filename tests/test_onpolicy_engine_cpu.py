"""The host plumbing of the on-policy update engines (algo/_graphs.py, _C.adam_args, the helpers of algo/on_policy/ppo.py) on
CPU tensors: the AdamArgs builder against the five field-by-field fills it replaced, the caller's say over the eager ->
captured -> replayed rule, the joint sequence's one-slot cache against the state machine it replaced, and the views of a
statistics block.  `_C.capture_graph` is a stand-in that runs the launches once and counts.  CPU only."""
import ctypes
import itertools

import pytest
import torch

from torchrl_amd import _C, dist
from torchrl_amd.algo._graphs import GraphCache, LastGraph
from torchrl_amd.algo.off_policy import _engine as off_engine
from torchrl_amd.algo.on_policy import ppo as ppo_mod


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


def test_the_off_policy_engines_import_the_same_cache():
    assert off_engine.GraphCache is GraphCache and issubclass(LastGraph, GraphCache)


# ------------------------------------------------------------------ GraphCache.run(..., eager=)
def test_eager_false_captures_although_collectives_are_active(captured, monkeypatch):
    monkeypatch.setattr(dist, "collectives_active", lambda: True)
    monkeypatch.setenv("TRL_NO_GRAPH", "1")                              # (the caller has weighed both already)
    cache, f = GraphCache(4), _Counter()
    cache.run(("k",), f)                                                 # today's rule: eager, nothing recorded
    assert f.n == 1 and len(cache) == 0 and not captured
    cache.run(("k",), f, eager=False)                                    # first visit: eager, seen
    cache.run(("k",), f, eager=False)                                    # second: captured (the capture runs the launches)
    cache.run(("k",), f, eager=False)
    assert f.n == 3 and len(captured) == 1 and captured[0].replays == 2 and list(cache) == [("k",)]
    cache.run(("k",), f)                                                 # None again: today's rule, eager
    assert f.n == 4 and captured[0].replays == 2


def test_eager_true_runs_the_launches_and_leaves_the_key_unseen(captured):
    cache, f = GraphCache(4), _Counter()
    for n in range(1, 4):
        cache.run(("k",), f, eager=True)
        assert f.n == n and len(cache) == 0 and not captured
    cache.run(("k",), f)                                                 # had an eager visit marked it seen, this would capture
    assert f.n == 4 and not captured
    cache.run(("k",), f)
    assert f.n == 5 and len(captured) == 1
    cache.run(("k",), f, eager=True)                                     # a held graph is not replayed on a forced-eager visit
    assert f.n == 6 and captured[0].replays == 1 and len(cache) == 1


def test_eager_false_cannot_overfill_the_cache(captured):
    cache, f = GraphCache(1), _Counter()
    for _ in range(2):
        cache.run(("a",), f, eager=False)
    for n in range(3, 6):
        cache.run(("b",), f, eager=False)
        assert f.n == n and list(cache) == [("a",)] and len(captured) == 1


# ------------------------------------------------------------------ the joint sequence's cache
class _JointBefore:
    """The state machine `_FusedPPO.run` carried (graph, graph_key, seen), as it was written there."""

    def __init__(self):
        self._graph = self._graph_key = self._graph_seen = None

    def run(self, key, launch_all, use_graph):
        if not use_graph:
            launch_all()
            return "eager"
        elif self._graph is not None and self._graph_key == key:
            self._graph.replay()
            return "replay"
        elif self._graph_seen != key:
            self._graph_seen = key
            self._graph = None
            launch_all()
            return "eager"
        else:
            graph, _ = _C.capture_graph(launch_all)
            self._graph, self._graph_key = graph, key
            graph.replay()
            return "capture"


def _visit(cache, key, use_graph, captured):
    """What one visit of LastGraph did, read off the launches run, the captures made and the replays counted."""
    f, n_cap, replays = _Counter(), len(captured), sum(g.replays for g in captured)
    cache.run(key, f, eager=not use_graph)
    if len(captured) > n_cap:
        assert f.n == 1 and captured[-1].replays == 1 and cache.graph is captured[-1]
        return "capture"
    if f.n == 1:
        assert sum(g.replays for g in captured) == replays
        return "eager"
    assert f.n == 0 and sum(g.replays for g in captured) == replays + 1
    return "replay"


def test_joint_cache_table_on_the_sequence_A_A_A_B_B_A(captured):
    cache = LastGraph()
    assert cache.graph is None
    did = [_visit(cache, k, True, captured) for k in ("A", "A", "A", "B", "B", "A")]
    assert did == ["eager", "capture", "replay", "eager", "capture", "eager"]
    # row by row: (no graph, key != seen) eager; (no graph, key == seen) capture; (graph, same key) replay;
    # (graph, other key) eager and the graph dropped; then B's own second visit captures; A again finds B's graph: dropped
    assert cache.graph is None and len(captured) == 2 and [g.replays for g in captured] == [2, 1]
    assert _visit(cache, "A", True, captured) == "capture" and cache.graph is captured[2]


def test_joint_cache_drops_the_graph_when_another_key_arrives(captured):
    cache = LastGraph()
    for _ in range(2):
        cache.run("A", _Counter(), eager=False)
    assert cache.graph is captured[0] and list(cache) == ["A"]
    cache.run("B", _Counter(), eager=False)
    assert cache.graph is None and len(cache) == 0                       # graph dropped, seen = B
    assert _visit(cache, "B", True, captured) == "capture"


def test_an_eager_forced_visit_changes_nothing_in_the_joint_cache(captured):
    cache = LastGraph()
    assert _visit(cache, "A", True, captured) == "eager"
    assert _visit(cache, "B", False, captured) == "eager"                # (use_graph false: B is not remembered, A not forgotten)
    assert _visit(cache, "A", True, captured) == "capture"
    graph = cache.graph
    assert _visit(cache, "B", False, captured) == "eager" and cache.graph is graph      # the graph survives
    assert _visit(cache, "A", False, captured) == "eager" and graph.replays == 1         # and is not replayed
    assert _visit(cache, "A", True, captured) == "replay" and graph.replays == 2
    assert _visit(cache, "B", True, captured) == "eager" and cache.graph is None


def test_joint_cache_equals_the_state_machine_it_replaced_on_every_short_sequence(captured):
    visits = [(k, u) for k in ("A", "B", "C") for u in (True, False)]
    for seq in itertools.product(visits, repeat=5):
        before, after = _JointBefore(), LastGraph()
        for n, (key, use_graph) in enumerate(seq):
            want = before.run(key, _Counter(), use_graph)
            assert _visit(after, key, use_graph, captured) == want, (seq, n)
            assert (after.graph is None) == (before._graph is None), (seq, n)
        del captured[:]


def test_clearing_the_joint_cache_costs_one_eager_visit(captured):
    """`_buffers` clears it when (K, rows_mb) changes: the graph goes and so does `seen` (the one accepted difference)."""
    cache = LastGraph()
    assert [_visit(cache, "A", True, captured) for _ in range(3)] == ["eager", "capture", "replay"]
    cache.clear()
    assert cache.graph is None
    assert [_visit(cache, "A", True, captured) for _ in range(3)] == ["eager", "capture", "replay"]


# ------------------------------------------------------------------ adam_args, the on-policy fills
def _fields(a):
    out = {}
    for name, _ in _C.AdamArgs._fields_:
        v = getattr(a, name)
        out[name] = list(v) if isinstance(v, ctypes.Array) else v
    return out


class _Engine(ppo_mod._FusedPPO):
    """The buffers `_adam_args` reads, without a device."""

    def __init__(self):
        self.P_pf, self.P_vf = 180, 120
        self.flat, self.grads, self.m, self.v = (torch.zeros(300) for _ in range(4))
        self.norms = torch.zeros(4, 2)
        self.step_state, self.lr_dev = torch.zeros(4, dtype=torch.float64), torch.zeros(2)


def _fused_fill(self, lr_pf, lr_vf, device_state):
    a = _C.AdamArgs()                                                    # _FusedPPO.run / _run_chains, field by field
    a.params, a.grads, a.exp_avg, a.exp_avg_sq = (self.flat.data_ptr(), self.grads.data_ptr(),
                                                  self.m.data_ptr(), self.v.data_ptr())
    a.n_groups = 2
    a.group_sizes[0], a.group_sizes[1] = self.P_pf, self.P_vf
    a.group_lr[0], a.group_lr[1] = lr_pf, lr_vf
    a.max_norm, a.beta1, a.beta2, a.eps, a.grad_scale = 0.5, 0.9, 0.999, 1e-5, 1.0
    a.device_state = device_state
    return a


@pytest.mark.parametrize("device_state", [1, 0])                        # one process / peer transport; all-reduce calls
def test_adam_args_equals_the_joint_sequences_fill(device_state):
    self = _Engine()
    got = self._adam_args((3e-4, 1e-3), device_state=device_state)
    assert _fields(got) == _fields(_fused_fill(self, 3e-4, 1e-3, device_state))
    assert got.device_state == device_state and got.step_count == 0 and got.norms_out is None and got.device_lr is None
    # what the minibatch loop and the TRL_GRAPH_COLLECTIVES tail then set per step lands in the same fields
    want = _fused_fill(self, 3e-4, 1e-3, device_state)
    for a in (got, want):
        a.step_count, a.norms_out = 7, self.norms[2].data_ptr()
        a.step_count, a.step_state, a.device_lr = 0, self.step_state.data_ptr(), self.lr_dev.data_ptr()
    assert _fields(got) == _fields(want)


def test_adam_args_equals_the_two_chains_fill():
    self = _Engine()
    assert _fields(self._adam_args((2.5e-4, 5e-4), device_state=1)) == _fields(_fused_fill(self, 2.5e-4, 5e-4, 1))


def test_adam_args_equals_the_policy_only_fill():
    self, lr = _Engine(), 3e-3
    self.P_pf, self.P_vf, self.eps = 300, 0, 1e-8                        # a vacant critic: `flat` is the policy's alone
    a = _C.AdamArgs()                                                    # the policy-only engines' fill, field by field
    a.params, a.grads, a.exp_avg, a.exp_avg_sq = (self.flat.data_ptr(), self.grads.data_ptr(),
                                                  self.m.data_ptr(), self.v.data_ptr())
    a.n_groups = 1
    a.group_sizes[0] = self.P_pf
    a.group_lr[0] = lr
    a.max_norm, a.beta1, a.beta2, a.eps, a.grad_scale = 0.5, 0.9, 0.999, 1e-8, 1.0
    a.device_state = 1
    got = self._adam_args((lr,), device_state=1)
    assert _fields(got) == _fields(a)
    assert got.n_groups == 1 and list(got.group_sizes) == [300, 0, 0, 0] and list(got.group_lr)[1:] == [0.0] * 3
    assert _fields(self._adam_args((lr, 0.0), device_state=1)) == _fields(a)             # as the shared `run` calls it
    assert _Engine().eps == 1e-5                                         # (two networks: A2C's)


def test_adam_args_equals_the_generic_engines_fill():
    self, k = _Engine(), 3
    norms = self.norms
    a = _C.AdamArgs()                                                    # _GenericPPO.run, field by field
    a.params, a.grads, a.exp_avg, a.exp_avg_sq = (self.flat.data_ptr(), self.grads.data_ptr(),
                                                  self.m.data_ptr(), self.v.data_ptr())
    a.n_groups = 2
    a.group_sizes[0], a.group_sizes[1] = self.P_pf, self.P_vf
    a.max_norm, a.beta1, a.beta2, a.eps, a.grad_scale = 0.5, 0.9, 0.999, 1e-5, 1.0
    a.step_count, a.norms_out = 0, norms[k].data_ptr()
    a.step_state, a.device_lr = self.step_state.data_ptr(), self.lr_dev.data_ptr()
    got = self._adam_args(norms_out=norms[k].data_ptr(), step_state=self.step_state.data_ptr(),
                          device_lr=self.lr_dev.data_ptr())
    assert _fields(got) == _fields(a)
    assert list(got.group_lr) == [0.0] * 4 and got.device_state == 0 and got.device_lr == self.lr_dev.data_ptr()


def test_adam_args_equals_the_vmpo_fill():
    self = _Engine()
    self.step_count, norms = 41, self.norms[0]
    lr_pf, lr_vf = 1e-4, 7e-4
    a = _C.AdamArgs()                                                    # _VMPOEngine.update, field by field
    a.params, a.grads, a.exp_avg, a.exp_avg_sq = (self.flat.data_ptr(), self.grads.data_ptr(),
                                                  self.m.data_ptr(), self.v.data_ptr())
    a.n_groups = 2
    a.group_sizes[0], a.group_sizes[1] = self.P_pf, self.P_vf
    a.group_lr[0] = lr_pf
    a.group_lr[1] = lr_vf
    a.max_norm, a.beta1, a.beta2, a.eps, a.grad_scale = 0.5, 0.9, 0.999, 1e-5, 1.0
    a.step_count, a.norms_out = self.step_count + 1, norms.data_ptr()
    got = self._adam_args((lr_pf, lr_vf), step_count=self.step_count + 1, norms_out=norms.data_ptr())
    assert _fields(got) == _fields(a) and got.step_count == 42 and got.step_state is None


def test_adam_args_equals_the_trpo_value_fill_at_its_offset():
    self = _Engine()
    vf_steps, vf_norm, lr = 5, torch.zeros(1), 3e-4
    a = _C.AdamArgs()                                                    # _TRPOEngine.update_vf, field by field
    o = 4 * self.P_pf
    a.params, a.grads = self.flat.data_ptr() + o, self.grads.data_ptr() + o
    a.exp_avg, a.exp_avg_sq = self.m.data_ptr() + o, self.v.data_ptr() + o
    a.n_groups = 1
    a.group_sizes[0] = self.P_vf
    a.group_lr[0] = lr
    a.max_norm, a.beta1, a.beta2, a.eps, a.grad_scale = 0.5, 0.9, 0.999, 1e-5, 1.0
    a.step_count, a.norms_out = vf_steps, vf_norm.data_ptr()
    got = _C.adam_args(self.flat, self.grads, self.m, self.v, [self.P_vf], [lr], offset=self.P_pf, max_norm=0.5, eps=1e-5,
                       step_count=vf_steps, norms_out=vf_norm.data_ptr())
    assert _fields(got) == _fields(a)
    assert got.params == self.flat[self.P_pf:].data_ptr() and got.exp_avg_sq == self.v[self.P_pf:].data_ptr()
    assert list(got.group_sizes) == [120, 0, 0, 0] and got.device_state == 0


# ------------------------------------------------------------------ statistics block, hyper, bookkeeping
@pytest.mark.parametrize("K", [1, 3, 8])
def test_stat_views_are_the_three_slices_of_the_block(K):
    block = torch.arange(29.0 * K, dtype=torch.float64)
    raw, info, norms = ppo_mod._stat_views(block, K)
    assert torch.equal(raw, block[:4 * K].view(K, 4)) and raw.data_ptr() == block.data_ptr()
    assert torch.equal(info, block[4 * K:28 * K].view(K, 24)) and info.data_ptr() == block.data_ptr() + 32 * K
    assert norms.dtype == torch.float32 and norms.shape == (K, 2) and norms.data_ptr() == block.data_ptr() + 224 * K
    assert torch.equal(norms, block[28 * K:].view(torch.float32).view(K, 2))
    norms[K - 1, 1] = 2.5                                                # views, not copies: a row of one chain's block too
    assert block[29 * K - 1:].view(torch.float32)[1] == 2.5
    both = torch.zeros(2, 29 * K, dtype=torch.float64)
    assert ppo_mod._stat_views(both[1], K)[2].data_ptr() == both.data_ptr() + 8 * (29 * K + 28 * K)


def test_hyper_and_the_end_of_run_bookkeeping():
    class _Pf:
        tanh_action = True

    class _Algo:
        pf, entropy_coeff, clip_para, clipped_value_loss = _Pf(), 0.005, 0.2, False
    assert ppo_mod._hyper(_Algo) == (0.2, 0.005, 0, 1) and [type(x) for x in ppo_mod._hyper(_Algo)] == [float, float, int, int]
    del _Algo.clip_para, _Algo.clipped_value_loss                        # A2C has neither
    _Pf.tanh_action = 0
    assert ppo_mod._hyper(_Algo) == (0.0, 0.005, 0, 0)
    self = _Engine()
    self.step_count, self._opt_steps = 10, [torch.tensor(10.0), torch.tensor(10.0)]
    self._stepped(4)
    assert self.step_count == 14 and [float(s) for s in self._opt_steps] == [14.0, 14.0]
