"""The forward schedule, edge for edge: which stream every stage of SIU3RModel._run_stages is enqueued on, and every wait_stream() edge
between the streams, in enqueue order (CPU; no stage body runs).

_run_stages touches the device only through torch.cuda.current_stream(), torch.cuda.stream(s), Stream.wait_stream and
ctx.side_stream(i).  The test puts named stubs behind those four and logs ["run", stage, stream], ["after_seg", stream],
["wait", waiter, waited] and, last, ["return", stream of the tail].  A missing or misplaced wait is a race that the parity tests catch
only sometimes; here it is a one-line difference.

tests/golden/forward_schedule.json was recorded with this harness (python tests/test_forward_schedule.py --record) at the commit before
_run_stages became a table, and is the schedule that commit enqueued.  It changes only by a deliberate, reviewed edit of the schedule:
never re-record it to make a refactor pass."""
import contextlib
import itertools
import json
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from siu3r_amd import model as M  # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forward_schedule.json")
CONFIGS = list(itertools.product((1, 2), (2, 3), (True, False), (True, False), (False, True)))  # B, V, concurrent, fold, pipelined


def _key(B, V, concurrent, fold, pipelined):
    return f"B{B}-V{V}-concurrent{int(concurrent)}-fold{int(fold)}-pipelined{int(pipelined)}"


class _Stream:
    def __init__(self, name, log):
        self.name, self._log = name, log

    def wait_stream(self, other):
        self._log.append(["wait", self.name, other.name])


def _trace(mp, B, V, concurrent, fold, pipelined):
    """(the logged sequence, the stage names of _stages(st)) of one _run_stages call"""
    log = []
    side = {}
    cur = [_Stream("main", log)]

    @contextlib.contextmanager
    def on_stream(s):
        cur.append(s)
        try:
            yield
        finally:
            cur.pop()

    mp.setattr(torch.cuda, "current_stream", lambda *a, **k: cur[-1])
    mp.setattr(torch.cuda, "stream", on_stream)
    m = object.__new__(M.SIU3RModel)
    m._ctx = types.SimpleNamespace(concurrent=concurrent, fold=fold, dev="cpu",
                                   side_stream=lambda i: side.setdefault(i, _Stream(f"side{i}", log)))
    m.adapter, m.raw_gs_dim = None, 83
    m.backbone = types.SimpleNamespace(dec_depth=12, enc_depth=24, enc_embed_dim=1024)
    st = M._Run(torch.empty(B, V, 3, 32, 32), None)
    tail = m._run_stages(st, lambda name, fn: log.append(["run", name, cur[-1].name]), lambda: log.append(["after_seg", cur[-1].name]), pipelined)
    assert len(cur) == 1, "a torch.cuda.stream() context was left open"
    log.append(["return", tail.name])
    return log, [name for name, _ in m._stages(st)]


def _golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("B,V,concurrent,fold,pipelined", CONFIGS, ids=[_key(*c) for c in CONFIGS])
def test_schedule_is_the_recorded_one(monkeypatch, B, V, concurrent, fold, pipelined):
    got, _ = _trace(monkeypatch, B, V, concurrent, fold, pipelined)
    want = _golden()[_key(B, V, concurrent, fold, pipelined)]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"step {i}: enqueues {g}, the recorded schedule has {w}"
    assert len(got) == len(want), (len(got), len(want))


def test_fixture_tells_the_configurations_apart():
    """(a harness that collapses the configurations -- every stream 'main', one shape for all -- must not pass)"""
    gold = _golden()
    assert sorted(gold) == sorted(_key(*c) for c in CONFIGS)
    assert len({json.dumps(seq) for seq in gold.values()}) >= 12


@pytest.mark.parametrize("B,V,concurrent,fold,pipelined", CONFIGS, ids=[_key(*c) for c in CONFIGS])
def test_every_stage_runs_once(monkeypatch, B, V, concurrent, fold, pipelined):
    got, names = _trace(monkeypatch, B, V, concurrent, fold, pipelined)
    ran = [step[1] for step in got if step[0] == "run"]
    assert sorted(ran) == sorted(names) and len(set(ran)) == len(ran), (ran, names)
    assert sum(step[0] == "after_seg" for step in got) == 1


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], "usage: python tests/test_forward_schedule.py --record   (see the docstring first)"
    out = {}
    for c in CONFIGS:
        with pytest.MonkeyPatch.context() as mp:
            out[_key(*c)] = _trace(mp, *c)[0]
    with open(FIXTURE, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in out.items()) + "\n}\n")
    print(f"{FIXTURE}: {len(out)} configurations, {sum(map(len, out.values()))} steps, {len({json.dumps(v) for v in out.values()})} distinct")
