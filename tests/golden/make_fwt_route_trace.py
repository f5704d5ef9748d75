"""Records which calls the multi-level drivers and autograd ops of ``_fwt.py`` make into the level engine, WITHOUT a GPU, and writes
them to ``fwt_route_trace.json``.

The engine is the numpy stand-in of tests/_oracle_engine.py, which also serves the multi-level calls (``pyramid_levels``,
``analysis_pyramid``, ``synthesis_pyramid``, ``analysis_tail``, ``synthesis_long`` …) that CPU tensors never reach on the real engine;
every public method is wrapped so that a call from the host layer appends ``[method, shapes of its tensor arguments]`` (calls the
stand-in makes into itself are not recorded).  The table: the six multi-level transforms, graph-free / gradient w.r.t. the input /
the same with ``create_graph=True``, zero and symmetric mode.

    python tests/golden/make_fwt_route_trace.py            # rewrite the fixture from the modules of this tree
    python tests/golden/make_fwt_route_trace.py --check    # compare instead of writing

tests/test_host_logic.py runs the same table and compares exactly.
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "fwt_route_trace.json")

TABLE = (("wavedec2", "waverec2", (2, 40, 44), 3), ("wavedec", "waverec", (3, 60), 3), ("fswavedec2", "fswaverec2", (2, 33, 41), 2))


def _shapes(o):
    if isinstance(o, torch.Tensor):
        return [list(o.shape)]
    if isinstance(o, (list, tuple)):
        return [s for e in o for s in _shapes(e)]
    return []


def tracing(engine, trace: list):
    """``engine`` with every public method wrapped to append ``[name, shapes of the tensor arguments]`` to ``trace``."""
    depth = [0]

    def wrap(name, fn):
        def call(*args, **kw):
            if depth[0] == 0:
                trace.append([name, _shapes(args) + _shapes(list(kw.values()))])
            depth[0] += 1
            try:
                return fn(*args, **kw)
            finally:
                depth[0] -= 1

        return call

    for name in dir(type(engine)):
        if not name.startswith("_") and callable(getattr(engine, name)):
            setattr(engine, name, wrap(name, getattr(engine, name)))
    return engine


def _tensors(o):
    if isinstance(o, torch.Tensor):
        return [o]
    return [t for e in (o.values() if isinstance(o, dict) else o) for t in _tensors(e)]


def _rebuild(c, ts):
    it = iter(ts)
    out = [({k: next(it) for k in lv} if isinstance(lv, dict) else type(lv)(*[next(it) for _ in lv]) if isinstance(lv, tuple) else next(it)) for lv in c]
    return out if isinstance(c, list) else tuple(out)


def record() -> dict:
    """Runs the table with ``ptwt_amd._engine.ENGINE`` replaced by the traced stand-in (restored afterwards)."""
    import ptwt_amd
    from ptwt_amd import _engine
    from tests._oracle_engine import OracleLevelEngine

    trace: list = []
    keep = _engine.ENGINE
    _engine.ENGINE = tracing(OracleLevelEngine(), trace)
    out = {}

    def run(key, fn):
        for memo in _engine._routing_caches:  # (a case does not depend on the ones before it)
            memo.clear()
        del trace[:]
        fn()
        first = list(trace)
        del trace[:]
        fn()  # (the same geometry again: what the routing memos replay)
        out[key] = {"first": first, "again": list(trace)}

    try:
        for dec, rec, shape, level in TABLE:
            for mode in ("zero", "symmetric"):
                x = torch.sin(torch.arange(float(torch.Size(shape).numel())) * 0.37).reshape(shape)
                with torch.no_grad():
                    c = getattr(ptwt_amd, dec)(x, "db2", level=level, mode=mode)
                flat = _tensors(c)
                for how in ("graph-free", "grad", "create-graph"):
                    gkw = dict(create_graph=True) if how == "create-graph" else {}

                    def fwd():
                        if how == "graph-free":
                            with torch.no_grad():
                                return getattr(ptwt_amd, dec)(x, "db2", level=level, mode=mode)
                        xg = x.clone().requires_grad_(True)
                        got = _tensors(getattr(ptwt_amd, dec)(xg, "db2", level=level, mode=mode))
                        return torch.autograd.grad(sum((t * t).sum() for t in got), xg, **gkw)

                    def inv():
                        if how == "graph-free":
                            with torch.no_grad():
                                return getattr(ptwt_amd, rec)(c, "db2")
                        leaves = [t.clone().requires_grad_(True) for t in flat]
                        y = getattr(ptwt_amd, rec)(_rebuild(c, leaves), "db2")
                        return torch.autograd.grad((y * y).sum(), leaves, **gkw)

                    run("%s-%s-%s" % (dec, mode, how), fwd)
                    run("%s-%s-%s" % (rec, mode, how), inv)
    finally:
        _engine.ENGINE = keep
        for memo in _engine._routing_caches:
            memo.clear()
    return json.loads(json.dumps(out))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    got = record()
    if "--check" in sys.argv:
        with open(FIXTURE) as f:
            want = json.load(f)
        bad = [k for k in want if got.get(k) != want[k]] + [k for k in got if k not in want]
        assert not bad, bad
        print("fwt_route_trace.json: %d cases match" % len(want))
    else:
        if "--list" in sys.argv:
            for k, v in got.items():
                print("%-36s %s" % (k, " | ".join(",".join(n for n, _ in v[w]) for w in ("first", "again"))))
        with open(FIXTURE, "w") as f:
            json.dump(got, f, separators=(",", ":"), sort_keys=True)
            f.write("\n")
        print("wrote %s: %d cases, %d bytes" % (FIXTURE, len(got), os.path.getsize(FIXTURE)))
