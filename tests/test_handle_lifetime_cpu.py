"""active_gym.lifetime.Owner without the library: handles are plain objects with a ``value``, destroy / detach are recording
callables.  The tree is the env's: pipeline -> {history, loop}, runner -> {loop}, history -> {sampler, step log}."""
import itertools

import pytest

from active_gym import lifetime


class _Handle:
    def __init__(self):
        self.value = 1


class _Node(lifetime.Owner):
    def __init__(self, name, events, parents=()):
        self.name = name
        self._own(_Handle(), lambda h: events.append(("destroy", name)), parents)


def _tree(events, attach=True):
    pipe, runner = _Node("pipe", events), _Node("runner", events)
    hist = _Node("hist", events, (pipe,))
    loop = _Node("loop", events, (pipe, runner))
    smp, log = _Node("smp", events, (hist,)), _Node("log", events, (hist,))
    if attach:
        hist._while_both_alive(loop, lambda: events.append(("detach", "loop")))
    return dict(pipe=pipe, runner=runner, hist=hist, loop=loop, smp=smp, log=log)


def _destroyed(events):
    return [name for what, name in events if what == "destroy"]


def test_closing_the_root_goes_leaves_first():
    events = []
    t = _tree(events)
    t["pipe"].close()
    assert _destroyed(events) == ["smp", "log", "hist", "loop", "pipe"]
    assert t["runner"].alive and not any(t[k].alive for k in ("pipe", "hist", "loop", "smp", "log"))
    assert t["runner"]._children == [] and t["pipe"]._children == []


def test_a_live_loop_is_detached_before_the_history_is_destroyed():
    events = []
    t = _tree(events)
    t["pipe"].close()
    assert events.index(("detach", "loop")) < events.index(("destroy", "hist")) < events.index(("destroy", "loop"))
    assert events.count(("detach", "loop")) == 1
    assert events.index(("destroy", "log")) < events.index(("detach", "loop"))          # after the children


def test_a_loop_closed_first_is_not_detached_afterwards():
    events = []
    t = _tree(events)
    t["loop"].close()
    t["hist"].close()
    t["pipe"].close()
    assert ("detach", "loop") not in events
    assert _destroyed(events) == ["loop", "smp", "log", "hist", "pipe"]


def test_closing_the_history_alone_leaves_pipeline_and_loop_open():
    events = []
    t = _tree(events)
    t["hist"].close()
    assert events == [("destroy", "smp"), ("destroy", "log"), ("detach", "loop"), ("destroy", "hist")]
    assert t["pipe"].alive and t["loop"].alive and t["runner"].alive
    assert t["pipe"]._children == [t["loop"]]
    for k in ("smp", "log"):
        with pytest.raises(RuntimeError, match="closed"):
            t[k]._live()
    t["pipe"]._live()


def test_destroy_runs_exactly_once():
    events = []
    t = _tree(events)
    t["smp"].close()
    t["smp"].close()
    t["smp"].__del__()
    t["pipe"].close()
    t["pipe"].close()
    for node in t.values():
        node.__del__()
    assert sorted(_destroyed(events)) == sorted(t)          # the runner by its __del__


def test_the_closed_error_names_what_was_closed():
    events = []
    hist = _Node("hist", events)
    smp = _Node("smp", events, (hist,))
    smp._closed_what = "the sampler or its history"
    smp._live()
    hist.close()
    with pytest.raises(RuntimeError, match="^the sampler or its history is closed$"):
        smp._live()


def test_every_closing_order_of_a_five_node_tree():
    names = ("pipe", "hist", "loop", "smp", "log")
    parents = {"hist": "pipe", "loop": "pipe", "smp": "hist", "log": "hist"}
    for order in itertools.permutations(names):
        events = []
        pipe = _Node("pipe", events)
        hist, loop = _Node("hist", events, (pipe,)), _Node("loop", events, (pipe,))
        nodes = dict(pipe=pipe, hist=hist, loop=loop, smp=_Node("smp", events, (hist,)), log=_Node("log", events, (hist,)))
        hist._while_both_alive(loop, lambda: events.append(("detach", "loop")))
        for name in order:
            nodes[name].close()
        gone = _destroyed(events)
        assert sorted(gone) == sorted(names), order
        for child, parent in parents.items():
            assert gone.index(child) < gone.index(parent), (order, gone)
        if ("detach", "loop") in events:
            assert events.index(("detach", "loop")) < events.index(("destroy", "hist")) < events.index(("destroy", "loop")), order
        else:
            assert gone.index("loop") < gone.index("hist"), order
