"""The eager -> captured -> replayed rule every update engine shares, on and off policy (host code, no kernel)."""
import os
from collections.abc import Mapping

from .. import _C, dist


def _eager_by_default():
    return os.environ.get("TRL_NO_GRAPH") == "1" or dist.collectives_active()


class GraphCache(Mapping):
    """Captured HIP graphs by key, at most `cap` of them and none ever evicted (a learning-rate schedule would mint a key
    per value).  A launch sequence runs eagerly on the first visit of its key, is captured on the second and replayed
    afterwards: the host then issues one call per update instead of ~45-90 and stays ahead of the device."""

    def __init__(self, cap):
        self.cap, self._graphs, self._seen = cap, {}, set()

    def __getitem__(self, key):
        return self._graphs[key]

    def __iter__(self):
        return iter(self._graphs)

    def __len__(self):
        return len(self._graphs)

    def clear(self):
        self._graphs.clear()
        self._seen.clear()

    def has_room(self, key):
        return key in self._graphs or len(self._graphs) < self.cap

    def run(self, key, launches, eager=None):
        """`eager`: the caller's decision; None = eager when TRL_NO_GRAPH=1 or while collectives are active.  An eager
        visit leaves the key unseen, and so does a new key that finds the cache full."""
        eager = _eager_by_default() if eager is None else eager
        graph = self._graphs.get(key)
        if eager or (graph is None and len(self._graphs) >= self.cap):
            launches()
        elif graph is not None:
            graph.replay()
        elif key not in self._seen:
            self._seen.add(key)
            launches()
        else:
            self._graphs[key], _ = _C.capture_graph(launches)
            self._graphs[key].replay()


class LastGraph(GraphCache):
    """One slot that a key other than the last one empties: the graph of a sequence whose key changes rarely, and then for
    good.  (A visit the caller forces eager changes nothing here.)"""

    def __init__(self):
        super().__init__(1)
        self._last = None

    @property
    def graph(self):
        return next(iter(self._graphs.values()), None)

    def run(self, key, launches, eager=None):
        eager = _eager_by_default() if eager is None else eager
        if not eager and key != self._last:
            self.clear()
            self._last = key
        super().run(key, launches, eager)
