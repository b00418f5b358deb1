"""The host-side plumbing every fused off-policy engine shares (none of it is kernel code, all of it runs on CPU tensors):
the eager -> captured -> replayed rule (`GraphCache`, algo/_graphs.py, shared with the on-policy engines), the networks'
home in one flat buffer, the copy of a sampled batch into the fixed-address inputs, the whole-epoch builder, and what an
algorithm forwards to its engine."""
import os

import numpy as np
import torch

from ... import _C, dist, ops
from ...networks import flatten_into
from .. import _optim
from .._graphs import GraphCache  # noqa: F401  (the engines and tests import it from here)


class FlatHome:
    """`plists` (one parameter list per network: per layer W, b and, behind a LayerNorm layer, gamma, beta --
    `ops.plan_params`) back to back in one buffer `flat`, the parameters views of it; `grads`, `m`, `v` beside it, with `views` the per-parameter gradient views and every
    `optimizer.state[p]` bound to its slices of the moments.  `targets`: the target networks' parameters, homed in `tflat`
    (allocated right behind `flat`, where it has always been).  `keep=(m, v)`: moments of an earlier home, reused when
    the size still matches."""

    def __init__(self, plists, optimizers, targets, keep=None):
        self.sizes = [sum(p.numel() for p in pl) for pl in plists]
        self.offsets = np.concatenate([[0], np.cumsum(self.sizes)]).astype(int)
        self.flat, self.tflat = flatten_into([p for pl in plists for p in pl]), flatten_into(targets)
        self.grads = torch.zeros_like(self.flat)
        if keep is not None and keep[0].numel() == self.flat.numel():
            self.m, self.v = keep[0].to(self.flat.device), keep[1].to(self.flat.device)
        else:
            self.m, self.v = torch.zeros_like(self.flat), torch.zeros_like(self.flat)
        # Adam: m = exp_avg, v = exp_avg_sq.  RMSprop: m = square_avg, v = momentum_buffer, c = grad_avg (allocated for a
        # centered RMSprop only).  SGD: m = momentum_buffer.  The state is bound under torch's names for the class.
        self.specs = [_optim.step_spec(opt) for opt in optimizers]
        self.c = torch.zeros_like(self.flat) if _optim.needs_third(self.specs) else None
        self.views, self._counts, off = [], [len(pl) for pl in plists], 0
        for opt, spec, pl in zip(optimizers, self.specs, plists):
            _optim.bind_state(opt, spec, pl, off, (self.m, self.v, self.c))
            for p in pl:
                n = p.numel()
                self.views.append(self.grads[off:off + n].view(p.shape))
                off += n

    def pairs(self):
        """The gradient views as (gW, gb) pairs: one list per parameter list."""
        firsts = np.concatenate([[0], np.cumsum(self._counts)])
        return [[(self.views[i], self.views[i + 1]) for i in range(f, f + n, 2)] for f, n in zip(firsts, self._counts)]

    def layer_views(self, layers_list):
        """`pairs()` for layer lists that may carry LayerNorms (`ops.net_layers`): per network one tuple per layer,
        (gW, gb) or (gW, gb, ggamma, gbeta), cut from the views in `ops.plan_params` order."""
        firsts, out = np.concatenate([[0], np.cumsum(self._counts)]), []
        for f, n, layers in zip(firsts, self._counts, layers_list):
            i, views = int(f), []
            for l in layers:
                k = len(ops.plan_params([l]))
                views.append(tuple(self.views[i:i + k]))
                i += k
            if i != f + n:
                raise _C.TrlError("FlatHome.layer_views: the layer lists do not match the homed parameter lists")
            out.append(views)
        return out


def post_kinds(layers):
    """What follows each layer's activation: None, "ln" or "act" (`ops.net_plan`)."""
    return [None if len(l) < 3 or l[2] is None else l[2][0] for l in layers]


def net_home(named_nets, named_targets, optimizers, same=(), keep=None):
    """The layer lists (`ops.net_layers`: plain (W, b) lists, or plans with post-ops for `add_ln` nets), the one activation
    code and the `FlatHome` of an engine's trained networks and targets -- parameters per layer in the order W, b, gamma,
    beta for both, so the Polyak step and the hard copy cover the norms.  named_nets / named_targets: [(name, net)], the
    targets tracking the LAST len(named_targets) trained networks.  `add_ln` nets need TRL_OFFPOLICY_LN=1
    (`ops.offpolicy_layers`).  `same`: groups of names that run in one grouped launch
    and must agree on `add_ln` (twin critics); a network and its target always must."""
    got = [ops.offpolicy_layers(n) for _, n in named_nets]
    tgot = [ops.offpolicy_layers(n) for _, n in named_targets]
    names = [n for n, _ in named_nets]
    if any(a != got[0][1] for _, a in got + tgot):
        raise _C.TrlError("%s must use the same activation" % ", ".join(names))
    layers, tlayers = [ls for ls, _ in got], [ls for ls, _ in tgot]
    kinds = dict(zip(names, (post_kinds(ls) for ls in layers)))
    for group in same:
        for other in group[1:]:
            if kinds[other] != kinds[group[0]]:
                raise _C.TrlError("%s and %s run as one grouped launch per layer and must agree on add_ln (LayerNorm on both or "
                                  "on neither, over the same layers)" % (group[0], other))
    off = len(named_nets) - len(named_targets)
    for (tname, _), tl, (name, _), sl in zip(named_targets, tlayers, named_nets[off:], layers[off:]):
        if post_kinds(tl) != post_kinds(sl) or [tuple(l[0].shape) for l in tl] != [tuple(l[0].shape) for l in sl]:
            raise _C.TrlError("%s and its target %s differ in structure (add_ln / layer shapes)" % (name, tname))
    home = FlatHome([ops.plan_params(ls) for ls in layers], optimizers, [p for ls in tlayers for p in ops.plan_params(ls)], keep)
    return layers, tlayers, got[0][1], home


def ln_slab_floats(layers, B, G=1):
    """Floats of gradient slabs the LayerNorms of one network leave in a fold plan's workspace per backward pass of B rows
    that runs as one of G problems."""
    lib = _C.lib()
    return sum(max(0, lib.trl_layernorm_bwd_group_workspace(G, B, int(l[0].shape[0]))) for l, k in zip(layers, post_kinds(layers))
               if k == "ln")


def load_static(st, batch, keys):
    """Copy the sampled `batch` into the fixed-address inputs `st` (a replay gather that wrote there already is skipped)."""
    for k in keys:
        src = batch[k]
        if src is st[k]:
            continue
        src = src if isinstance(src, torch.Tensor) else torch.as_tensor(np.asarray(src))
        st[k].copy_(src.to(dtype=st[k].dtype).reshape(st[k].shape), non_blocking=True)


class _FusedOffPolicy:
    """What the engines with a whole-epoch path share.  Theirs: `_graphs`, `_ring`, `_slab`, `step_count`, `step_state`,
    `static_batch(B)`, `_sequence(st, soft)`, `_handles(count, B)`, `_epoch_declined(count)`, `_epoch_key(soft)`."""
    KEYS = ("obs", "next_obs", "acts", "rewards", "terminals")           # the sampled keys = the static input tensors

    def update(self, batch):
        return self.resolve([self.enqueue(batch)])[0]

    def enqueue_epoch(self, count):
        """`count` x {uniform replay sample -> update} as ONE graph launch: the index sets are drawn on the host in the
        order `count` random_batch calls would draw them and uploaded once; every update of the graph gathers the set the
        device-resident update count selects (trl_gather_rows_multi with its update counter) and files its statistics
        into its ring slot.  Returns the handles, or None when this path does not apply: TRL_NO_GRAPH=1, several ranks, a
        replay buffer that does not store the sampled keys plainly, a full graph cache, the engine's own conditions."""
        algo = self.algo
        buf, B = getattr(algo, "replay_buffer", None), int(algo.batch_size)
        if buf is None or count < 1 or count > self._ring.slots or dist.collectives_active() or \
                os.environ.get("TRL_NO_GRAPH") == "1" or not hasattr(buf, "gather_sources") or self._epoch_declined(count):
            return None
        keys, soft = self.KEYS, bool(algo.use_soft_update)
        srcs = buf.gather_sources(keys)
        if srcs is None:
            return None
        st, nrows = self.static_batch(B), buf._rows_per_batch(B)
        if any(s.dtype != st[k].dtype or s[0].numel() * nrows != st[k].numel() for s, k in zip(srcs, keys)):
            return None
        key = ("epoch", count, B, nrows, tuple(s.data_ptr() for s in srcs)) + self._epoch_key(soft)
        if not self._graphs.has_room(key):                               # before anything below consumes the host's
            return None                                                  # random stream or touches the ring
        self._ring.make_room(count)
        slab = self._slab.upload(self.step_count, buf.draw_indices(B, count))
        dsts = [st[k] for k in keys]

        def launches():
            for _ in range(count):
                _C.gather_rows_multi(srcs, slab, dsts, slab_counter=self.step_state, n_rows=nrows)
                self._sequence(st, soft)
        self._graphs.run(key, launches)
        self.step_count += count
        return self._handles(count, B)


class _EngineSurface:
    """What an algorithm offers over its fused engine (`engine()`): `update` and its deferred forms, `static_batch`."""

    def static_batch(self):
        return self.engine().static_batch(self.batch_size)

    def update(self, batch):
        self.training_update_num += 1
        return self.engine().update(batch)

    def update_deferred(self, batch):
        """`update` without its read-back: OffRLAlgo.update_per_epoch enqueues all `opt_times` updates of an epoch and
        resolves their info dicts with one D2H (`resolve_updates`)."""
        self.training_update_num += 1
        return self.engine().enqueue(batch)

    def update_epoch_deferred(self, count):
        """All `count` {uniform sample -> update} pairs of an epoch as one replayed graph (None when the engine's
        conditions for it do not hold: the caller then samples and enqueues one by one)."""
        handles = self.engine().enqueue_epoch(count)
        if handles is not None:
            self.training_update_num += count
        return handles

    def resolve_updates(self, handles):
        return self.engine().resolve(handles)
