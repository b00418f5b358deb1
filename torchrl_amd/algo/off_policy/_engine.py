"""The host-side plumbing every fused off-policy engine shares (none of it is kernel code, all of it runs on CPU tensors):
the eager -> captured -> replayed rule (`GraphCache`, algo/_graphs.py, shared with the on-policy engines), the networks'
home in one flat buffer, the copy of a sampled batch into the fixed-address inputs, the whole-epoch builder, and what an
algorithm forwards to its engine."""
import os

import numpy as np
import torch

from ... import _C, dist
from ...networks import flatten_into
from .. import _optim
from .._graphs import GraphCache  # noqa: F401  (the engines and tests import it from here)


class FlatHome:
    """`plists` (one parameter list per network, W and b alternating) back to back in one buffer `flat`, the parameters
    views of it; `grads`, `m`, `v` beside it, with `views` the per-parameter gradient views and every
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
