"""Owner — the one place that keeps a raw C handle alive and destroys it: for the ten classes that hold one (ObsPipeline,
NativeHostRunner, NativeStepLoop, FrameHistory, ReplaySampler, StepLog, PrioritizedSampler, RandomShift, Minibatcher, Chunker).

An object that was built from the raw handles of others names them as its parents and must be gone before any of them is.  The
tree is

    pipeline -> {history, loop}      runner -> {loop}      history -> {samplers, step logs, shift sources, minibatchers, chunkers}

and ``close()`` of any node closes its children first (in the order they were made), then destroys its own handle, then takes
itself off its parents' lists; it does so once, however often and from wherever it is called - by the user, by a parent, or by
the one ``__del__`` when the garbage collector runs the finalizers of an abandoned env in an order of its own.

It needs no library: a handle is anything with a ``value`` that is true while the handle is (a ``ctypes.c_void_p``), destroy any
callable that takes it."""
from __future__ import annotations


class Owner:
    _handle = None           # (class defaults: close() / __del__ of an object whose constructor raised early find nothing to do)
    _children = ()
    _parents = ()
    _closed_what = "the handle"

    def _own(self, handle, destroy, parents=()):
        """handle: the created handle; destroy(handle) frees it; parents: the Owners whose raw handles this object holds."""
        self._handle, self._destroy, self._parents = handle, destroy, tuple(parents)
        self._children, self._links = [], []
        for p in self._parents:
            p._children.append(self)

    @property
    def alive(self) -> bool:
        return self._handle is not None and bool(self._handle.value)

    def _live(self):
        """RuntimeError once this object is closed - by itself, or by a parent that closed (a parent closes its children first,
        so an open child has open parents: one test, on the hot path of sample() and gather())."""
        if not self._handle.value:
            raise RuntimeError(f"{self._closed_what} is closed")

    def _while_both_alive(self, peer: "Owner", undo):
        """``undo()`` runs when this object closes - after its children, before its destroy - if ``peer`` is then still alive
        (a peer that closed first needs nothing undone: it simply forgets)."""
        self._links.append((peer, undo))

    def close(self):
        if not self.alive:
            return
        for child in list(self._children):
            child.close()
        for peer, undo in self._links:
            if peer.alive:
                undo()
        self._links = []
        self._destroy(self._handle)
        self._handle.value = None               # in place: every name of the handle (pipe._ctx, history.handle, ...) reads null
        for p in self._parents:
            p._children.remove(self)

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass
