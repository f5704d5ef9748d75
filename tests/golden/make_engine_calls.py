"""Records every call the host layer (``_engine.py``, ``_bwt.py``, ``stationary_transform.py``) makes into ``libmifwt.so`` for a table
of small geometries, WITHOUT a GPU, and writes them to ``engine_calls.json``.

The real library is loaded; a :class:`RecordingLib` stands in its place.  Host-only queries (``*_supported``, ``*kernel_id*``,
``*workspace_bytes*``, ...) pass through to the real library, so the routes are the ones the library really picks; every launch
entry point is recorded and answers 0.  ``_require_gpu``, the stream lookup and ``torch.cuda.device`` / ``current_device`` are
stubbed, so CPU tensors reach the launch.  Per launch the record holds the entry name, the bytes of every descriptor, every scalar,
the contents of every tap / integer array and every pointer as (which tensor, byte offset); per call the shapes, strides and dtypes of
what it returned and the names of the host queries it made (none on a cache hit).

    python tests/golden/make_engine_calls.py            # rewrite the fixture from the modules of this tree
    python tests/golden/make_engine_calls.py --check    # compare instead of writing

tests/test_engine_calls_host.py runs the same cases and compares exactly; tools/host_cpu_profile.py uses the same stand-in.
"""
import contextlib
import ctypes
import fnmatch
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "engine_calls.json")
STREAM = 0x5EED00

QUERIES = ("*_supported", "*kernel_id*", "*workspace_bytes*", "*_levels", "*_max_n", "*_plan", "*_schedule", "mifwt_set_option",
           "mifwt_strerror", "mifwt_abi_version", "mifwt_launch_count")
EXEMPT: tuple = ()  # launch entry points that only tools/ reach


def is_query(name: str) -> bool:
    return any(fnmatch.fnmatch(name, p) for p in QUERIES)


_INTS = (ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t, ctypes.c_uint64)


def _struct(arg):
    return arg._obj if hasattr(arg, "_obj") else arg.contents


class RecordingLib:
    """Stands in for the loaded library: queries go to the real one, launches are handed to ``sink(name, encoded args)`` (or dropped
    when there is no sink) and answer 0 — or what ``answers[name](args)`` says, for an entry that refuses some requests."""

    def __init__(self, real, sink=None, on_query=None, answers=None):
        self.__dict__.update(_real=real, _sink=sink, _on_query=on_query, _answers=answers or {})

    def __getattr__(self, name):
        fn = getattr(self._real, name)  # (AttributeError for a missing symbol, as from the library itself)
        if is_query(name):
            if self._on_query is None or name == "mifwt_strerror":
                return fn
            on_query = self._on_query

            def query(*args):
                on_query(name)
                return fn(*args)

            return query
        sink, answer = self._sink, self._answers.get(name)
        if sink is None:
            stub = (lambda *args: 0) if answer is None else (lambda *args: answer(args))  # noqa: E731
        else:
            def stub(*args):
                argtypes = fn.argtypes
                assert len(args) == len(argtypes), (name, len(args), len(argtypes))
                sink(name, [_encode(t, a) for t, a in zip(argtypes, args)])
                return 0 if answer is None else answer(args)

        self.__dict__[name] = stub
        return stub


def _encode(t, a):
    if t in _INTS:
        return int(a)
    if t is ctypes.c_double:
        return float(a)
    if t is ctypes.c_void_p:
        return ("ptr", a)
    if a is None:
        return None
    target = t._type_
    if target in _INTS or target is ctypes.c_double:
        return [v for v in a]
    if target is ctypes.c_void_p:
        return [("ptr", v) for v in a]
    if issubclass(target, ctypes.Structure):
        s = _struct(a)
        if [f[0] for f in target._fields_] == ["rows", "n_top", "n_bot"]:
            return {"rows": ("ptr", s.rows), "n_top": s.n_top, "n_bot": s.n_bot}
        return bytes(s).hex()
    inner = target._type_  # pointer to pointer: an array of descriptor pointers, or of pointers to three band pointers each
    if inner is ctypes.c_void_p:
        return [[("ptr", q[j]) for j in range(3)] for q in a]
    return [bytes(q.contents).hex() for q in a]


def _span(t):
    st = t.untyped_storage()
    return st.data_ptr(), st.nbytes()


class Recorder:
    """Runs calls under the stubs and collects their records."""

    def __init__(self):
        import ptwt_amd  # noqa: F401
        from ptwt_amd import _bwt, _engine, stationary_transform

        self.engine = _engine
        self.real = _engine.load_library()
        for mod in (_bwt, stationary_transform):  # (modules that bind entries of their own do it on the real library, before the stand-in)
            if hasattr(mod, "_lib"):
                mod._lib()
        self.records = {}
        self.entries = set()
        self._launches, self._queries, self._tracked = [], [], []
        # the two 1-D tail entries refuse odd filter lengths before they launch anything (MIFWT_ERR_UNSUPPORTED, csrc/mifwt_dwt1_tail.hip)
        self.answers = {"mifwt_dwt1_fwd_tail": lambda a: -2 if a[1] % 2 else 0, "mifwt_dwt1_inv_tail": lambda a: -2 if a[1] % 2 else 0}

    @contextlib.contextmanager
    def stubs(self):
        E = self.engine
        keep = (E._lib, E._require_gpu, torch.cuda.device, torch.cuda.current_device, torch._C._cuda_getCurrentRawStream, torch.empty)
        real_empty = torch.empty

        def empty(*a, **k):
            t = real_empty(*a, **k)
            if t.device.type == "cpu":
                self._tracked.append(t)  # (kept alive until the call ends: no address is used twice within a call)
            return t

        E._lib = RecordingLib(self.real, self._on_launch, self._queries.append, self.answers)
        E._require_gpu = lambda t: None
        torch.cuda.device = lambda dev: contextlib.nullcontext()
        torch.cuda.current_device = lambda: 0
        torch._C._cuda_getCurrentRawStream = lambda index: STREAM
        torch.empty = empty
        try:
            yield self
        finally:
            E._lib, E._require_gpu, torch.cuda.device, torch.cuda.current_device, torch._C._cuda_getCurrentRawStream, torch.empty = keep

    def _on_launch(self, name, args):
        self.entries.add(name)
        others = {}

        def resolve(v):
            if isinstance(v, tuple) and len(v) == 2 and v[0] == "ptr":
                p = v[1]
                if p is None:
                    return None
                if p == STREAM:
                    return "stream"
                for i, t in enumerate(self._inputs):
                    base, size = _span(t)
                    if base <= p < base + size:
                        return ["in%d" % i, p - base]
                for i, t in enumerate(self._tracked):
                    base, size = _span(t)
                    if base <= p < base + max(size, 1):
                        return ["trk", i, p - base]
                return "other%d" % others.setdefault(p, len(others))
            if isinstance(v, list):
                return [resolve(e) for e in v]
            if isinstance(v, dict):
                return {k: resolve(e) for k, e in v.items()}
            return v

        self._launches.append({"entry": name, "args": resolve(args)})

    def call(self, case, fn, inputs):
        """Run ``fn(*inputs)`` once under the stubs and append its record to the case."""
        self._inputs = [t for t in inputs if isinstance(t, torch.Tensor)]
        self._launches, self._tracked = [], []
        del self._queries[:]
        out = err = None
        try:
            out = fn(*inputs)
        except (ValueError, RuntimeError, AssertionError) as e:  # (a case that pins an error: the launches made before it, its type and text)
            err = e
        flat = []

        def walk(o):
            if isinstance(o, torch.Tensor):
                flat.append(o)
            elif isinstance(o, dict):
                for k in o:
                    walk(o[k])
            elif isinstance(o, (list, tuple)):
                for e in o:
                    walk(e)

        walk(out)
        names, tmp = {}, {}
        for i, t in enumerate(self._tracked):
            base = _span(t)[0]
            for j, r in enumerate(flat):
                if r.device.type == "cpu" and _span(r)[0] == base and _span(r)[1]:
                    names[i] = "out%d" % j
                    break

        def finish(v):
            if isinstance(v, list):
                if len(v) == 3 and v[0] == "trk":
                    return [names.get(v[1]) or "tmp%d" % tmp.setdefault(v[1], len(tmp)), v[2]]
                return [finish(e) for e in v]
            if isinstance(v, dict):
                return {k: finish(e) for k, e in v.items()}
            return v

        rec = {"launches": finish(self._launches), "queries": list(self._queries),
               "returns": [None if out is None else "no tensor"] if not flat else
               [[list(r.shape), list(r.stride()), str(r.dtype).replace("torch.", "")] for r in flat]}
        if err is not None:
            rec["raises"] = [type(err).__name__, str(err)]
        self.records.setdefault(case, []).append(rec)
        self._tracked = []
        return out


# ---- the cases -------------------------------------------------------------------------------------------------------------------
def _z(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype)


def run_cases(r: Recorder) -> None:
    import ptwt_amd as P
    from ptwt_amd import _bwt, _engine as E, _wavelets, stationary_transform as S  # noqa: F401

    eng = E.ENGINE

    def case(name, fn, *inputs, times=1):
        E.set_option(E.OPT_FORCE_GENERIC, 0)  # (the default; drops every plan and routing memo: a case does not depend on the ones before it)
        out = None
        for _ in range(times):
            out = r.call(name, fn, inputs)
        return out

    def flat2(c):
        return [c[0]] + [t for lv in c[1:] for t in lv]

    def unflat2(ts):
        return (ts[0], *[tuple(ts[1 + 3 * k: 4 + 3 * k]) for k in range((len(ts) - 1) // 3)])

    # -- the ten public transforms: every multi-level route and its inverse
    def dec_rec(tag, dec, rec, x, flatten, rebuild, **kw):
        c = case(tag + "-dec", lambda t: dec(t, **kw), x)
        ts = flatten(c)
        kw2 = {k: v for k, v in kw.items() if k in ("wavelet", "axes", "axis")}
        case(tag + "-rec", lambda *a: rec(rebuild(list(a)), **kw2), *ts)

    two = dict(flatten=flat2, rebuild=unflat2)
    dec_rec("wavedec2-streaming", P.wavedec2, P.waverec2, _z(2, 72, 512), wavelet="db4", level=3, mode="reflect", **two)
    dec_rec("wavedec2-small-planes", P.wavedec2, P.waverec2, _z(5, 40, 36), wavelet="db2", level=3, mode="symmetric", **two)
    dec_rec("wavedec2-per-level", P.wavedec2, P.waverec2, _z(2, 70, 530), wavelet="db5", level=2, mode="periodic", **two)
    dec_rec("wavedec2-tile-level", P.wavedec2, P.waverec2, _z(2, 70, 530), wavelet="db4", level=1, mode="zero", **two)
    dec_rec("wavedec2-f64", P.wavedec2, P.waverec2, _z(2, 37, 61, dtype=torch.float64), wavelet="db3", level=2, mode="constant", **two)
    one = dict(flatten=list, rebuild=list)
    dec_rec("wavedec-tail", P.wavedec, P.waverec, _z(3, 1001), wavelet="db5", level=3, mode="reflect", **one)
    dec_rec("wavedec-long", P.wavedec, P.waverec, _z(2, 300000), wavelet="db5", level=6, mode="symmetric", **one)
    dec_rec("wavedec-single", P.wavedec, P.waverec, _z(3, 101), wavelet="db2", level=1, mode="zero", **one)

    def flatd(c):
        return [c[0]] + [lv[k] for lv in c[1:] for k in lv]

    def unflatd(keys):
        n = len(keys)
        return lambda ts: (ts[0], *[dict(zip(keys, ts[1 + n * k: 1 + n * (k + 1)])) for k in range((len(ts) - 1) // n)])

    keys3 = ["aad", "ada", "add", "daa", "dad", "dda", "ddd"]
    dec_rec("wavedec3", P.wavedec3, P.waverec3, _z(2, 20, 22, 70), wavelet="db2", level=2, mode="reflect", flatten=flatd, rebuild=unflatd(keys3))
    dec_rec("fswavedec2", P.fswavedec2, P.fswaverec2, _z(2, 40, 300), wavelet="db3", level=2, mode="reflect", flatten=flatd,
            rebuild=unflatd(["ad", "da", "dd"]))
    dec_rec("fswavedec3", P.fswavedec3, P.fswaverec3, _z(2, 12, 14, 40), wavelet="db2", level=1, mode="zero", flatten=flatd, rebuild=unflatd(keys3))
    # -- an f16 2-D level with 18 taps or more: the 128-byte pitch and view_last
    with P.half_storage():
        dec_rec("fswavedec2-f16-20taps", P.fswavedec2, P.fswaverec2, _z(2, 50, 271, dtype=torch.float16), wavelet="db10", level=1, mode="symmetric",
                flatten=flatd, rebuild=unflatd(["ad", "da", "dd"]))

    # -- direct engine calls, host taps and device-resident taps
    lo4, hi4, rlo4, rhi4 = _wavelets.host_taps("db2")
    refl = E.MODE_IDS["reflect"]
    for form in ("host", "dtaps"):
        if form == "host":
            taps, extra = (lo4, hi4, rlo4, rhi4), []
        else:
            extra = [torch.tensor(t, dtype=torch.float64) for t in (lo4, hi4, rlo4, rhi4)]
            taps = tuple(E.DevTaps(t) for t in extra)
            extra = [d.t for d in taps]
        dl, dh, rl, rh = taps
        x = _z(2, 24, 70)
        buf = case("engine-analysis-" + form, lambda t, *e: eng.analysis(t, dl, dh, refl), x, *extra)
        bands = [buf[:, s] for s in range(4)]
        case("engine-synthesis-" + form, lambda a, b, c, d, *e: eng.synthesis(a, [b, c, d], rl, rh, [24, 70]), *bands, *extra)
        case("engine-analysis_adjoint-" + form, lambda g, *e: eng.analysis_adjoint(g, (24, 70), dl, dh, refl), torch.zeros_like(buf), *extra)
        case("engine-analysis_adjoint_bands-" + form, lambda a, b, c, d, *e: eng.analysis_adjoint_bands(a, [b, c, d], (24, 70), dl, dh, refl),
             *[_z(2, 13, 36) for _ in range(4)], *extra)
        case("engine-synthesis_adjoint-" + form, lambda g, *e: eng.synthesis_adjoint(g, (13, 36), rl, rh), x, *extra)
        x3 = _z(2, 24, 70)
        lo_hi = case("engine-analysis_outer-" + form, lambda t, *e: eng.analysis_outer(t, dl, dh, refl), x3, *extra)
        case("engine-synthesis_outer-" + form, lambda a, b, *e: eng.synthesis_outer(a, b, rl, rh, 24), lo_hi[0].contiguous(), lo_hi[1].contiguous(), *extra)
    # -- the three tap-correlate calls
    acc = _z(4, dtype=torch.float64)
    case("tap_correlate", lambda a, b, o: eng.tap_correlate(a, b, 4, 1, -1, refl, o), _z(6, 36), _z(6, 70), acc)
    case("tap_correlate-strided", lambda a, b, o: eng.tap_correlate(a, b, 4, 1, -1, refl, o), _z(6, 36, 2)[:, :, 0], _z(6, 70), acc)
    for along in (0, 1):
        a = _z(2, 13, 70) if along == 0 else _z(2, 24, 36)
        case("tap_correlate_planes-%d" % along, lambda a, b, o: eng.tap_correlate_planes(along, a, b, 4, 1, -1, refl, o), a, _z(2, 24, 70), acc)
    case("tap_correlate_dilated", lambda a, b, o: eng.tap_correlate_dilated(a, b, 4, 4, -2, o), _z(3, 64), _z(3, 64), acc)
    # -- stationary transform
    c = case("swt", lambda t: P.swt(t, "db3", level=2), _z(3, 64))
    case("iswt", lambda *ts: P.iswt(list(ts), "db3"), *c)
    case("swt-strided-f64", lambda t: P.swt(t, "db2", level=1), _z(3, 64, 2, dtype=torch.float64)[:, :, 0])

    # -- boundary-wavelet level maps: fused 1-D / 2-D / 3-D, the composed axis passes, the packet subtrees
    zero = E.MODE_IDS["zero"]
    for wav, shapes in (("db2", ((3, 41), (2, 20, 31), (2, 12, 14, 17))), ("db12", ((2, 100), (2, 50, 61)))):
        tp = _wavelets.host_taps(wav)
        fwd, inv = _bwt.bank(tp, "qr", "analysis"), _bwt.bank(tp, "qr", "synthesis")
        for shp in shapes:
            tag = "bwt-%s-%dd" % (wav, len(shp) - 1)
            buf = case(tag + "-rows", lambda t: _bwt.rows_level(t, fwd, refl), _z(*shp))
            case(tag + "-transposed", lambda *b: _bwt.transposed_level(list(b), inv, shp[1:]), *[buf[:, s] for s in range(buf.shape[1])])
    tp = _wavelets.host_taps("db2")
    fwd, inv = _bwt.bank(tp, "qr", "analysis"), _bwt.bank(tp, "qr", "synthesis")
    keep = _bwt.FORCE_COMPOSED3
    _bwt.FORCE_COMPOSED3 = True
    try:
        buf = case("bwt-composed3-rows", lambda t: _bwt.rows_level(t, fwd, zero), _z(2, 12, 14, 16))
        case("bwt-composed3-transposed", lambda *b: _bwt.transposed_level(list(b), inv, (12, 14, 16)), *[buf[:, s] for s in range(8)])
    finally:
        _bwt.FORCE_COMPOSED3 = keep
    case("bwt-unequal-detail-strides", lambda a, b, c, d: _bwt.transposed_level([a, b, c, d], inv, (20, 30)),
         _z(2, 10, 15), _z(2, 10, 15), _z(2, 10, 30)[:, :, :15], _z(2, 10, 15))
    lv = case("bwt-tree-rows", lambda t: _bwt.rows_tree(t, fwd, 3), _z(5, 64))
    case("bwt-tree-rows-strided", lambda t: _bwt.rows_tree(t, fwd, 2), _z(5, 2, 64)[:, 0])
    case("bwt-tree-transposed", lambda t: _bwt.transposed_tree(t, inv, 3), lv[-1])

    # -- views, copies, refusals, caches
    case("wavedec2-strided-view", lambda t: P.wavedec2(t, "db4", level=3, mode="reflect"), _z(3, 75, 521)[:, 3:, 5:])
    case("synthesis-unequal-detail-strides", lambda a, b, c, d: eng.synthesis(a, [b, c, d], rlo4, rhi4, [24, 70]),
         _z(2, 13, 36), _z(2, 13, 36), _z(2, 13, 72)[:, :, :36], _z(2, 13, 36))
    case("synthesis_pair-unequal-detail-strides",
         lambda a, b, c, d, e, f, g: eng.synthesis_pair(a, [b, c, d], [e, f, g], rlo4, rhi4, [140, 528]),
         _z(2, 37, 134), _z(2, 37, 134), _z(2, 37, 268)[:, :, :134], _z(2, 37, 134), _z(2, 71, 265), _z(2, 71, 265, 2)[..., 0], _z(2, 71, 265))
    case("wavedec2-empty-batch", lambda t: P.wavedec2(t, "db2", level=2, mode="zero"), _z(0, 24, 70))
    case("engine-synthesis-empty-batch", lambda a, b, c, d: eng.synthesis(a, [b, c, d], rlo4, rhi4, [24, 70]), *[_z(0, 13, 36) for _ in range(4)])
    s3 = 0.5 ** 0.5
    bank3 = (torch.tensor([s3, s3, 0.0]), torch.tensor([-s3, s3, 0.0]), torch.tensor([0.0, s3, s3]), torch.tensor([0.0, s3, -s3]))
    case("wavedec-3tap-refused-tail", lambda t: P.wavedec(t, bank3, level=3, mode="zero"), _z(3, 200))
    case("synthesis_tail-3tap-refused", lambda a, b, c: eng.synthesis_tail(a, [b, c], [0.0, s3, s3], [0.0, s3, -s3], [50, 98]), _z(3, 26), _z(3, 26), _z(3, 50))
    c = case("wavedec2-twice", lambda t: P.wavedec2(t, "db4", level=3, mode="reflect"), _z(2, 72, 512), times=2)
    case("waverec2-twice", lambda *ts: P.waverec2(unflat2(list(ts)), "db4"), *flat2(c), times=2)
    x = _z(2, 72, 512)
    case("force-generic-before", lambda t: P.wavedec2(t, "db4", level=2, mode="reflect"), x)
    E.set_option(E.OPT_FORCE_GENERIC, 0)
    try:
        E.set_option(E.OPT_FORCE_GENERIC, 1)
        r.call("force-generic-after", lambda t: P.wavedec2(t, "db4", level=2, mode="reflect"), [x])
        r.call("force-generic-after", lambda t: P.wavedec2(t, "db4", level=2, mode="reflect"), [x])
    finally:
        E.set_option(E.OPT_FORCE_GENERIC, 0)
    grad_cases(case, P, _wavelets)


def grad_cases(case, P, _wavelets) -> None:
    """Gradient-mode calls: the autograd routes of ``_fwt.py``.  Each case is one function that runs the forward and one
    ``torch.autograd.grad`` of the sum of its outputs; the record holds the launches of both."""

    def tensors(o):
        if isinstance(o, torch.Tensor):
            return [o]
        return [t for e in (o.values() if isinstance(o, dict) else o) for t in tensors(e)]

    def leaf(t):
        return torch.zeros_like(t).requires_grad_(True)

    def grad_of(forward, wrt=None, **gkw):
        def fn(*ts):
            out = forward(*ts)
            leaves = [t for t in ts if t.requires_grad] if wrt is None else [ts[i] for i in wrt]
            return out, torch.autograd.grad(sum(t.sum() for t in tensors(out) if t.requires_grad), leaves, **gkw)

        return fn

    def coeffs(dec, x, *a, **kw):  # (shapes of a decomposition, for the reconstruction cases: not part of any record)
        with torch.no_grad():
            return dec(x, *a, **kw)

    def rebuild_like(c):
        """flat tensors -> the container ``c`` has"""
        def build(ts):
            it = iter(ts)
            out = [({k: next(it) for k in lv} if isinstance(lv, dict) else type(lv)(*[next(it) for _ in lv]) if isinstance(lv, tuple) else next(it))
                   for lv in c]
            return out if isinstance(c, list) else tuple(out)

        return build

    def rec_case(name, rec, c, wavelet, needs=None, **gkw):
        flat = tensors(c)
        ins = [leaf(t) if needs is None or i in needs else torch.zeros_like(t) for i, t in enumerate(flat)]
        build = rebuild_like(c)
        case(name, grad_of(lambda *ts: rec(build(ts), wavelet), **gkw), *ins)

    # 1-D: the tail launch, the long launches, forward and fused chain backward
    x = _z(3, 1001).requires_grad_(True)
    case("grad-wavedec-tail", grad_of(lambda t: P.wavedec(t, "db5", level=3, mode="reflect")), x)
    rec_case("grad-waverec-tail", P.waverec, coeffs(P.wavedec, x, "db5", level=3, mode="reflect"), "db5")
    x = _z(2, 300000).requires_grad_(True)
    case("grad-wavedec-long", grad_of(lambda t: P.wavedec(t, "db5", level=6, mode="symmetric")), x)
    rec_case("grad-waverec-long", P.waverec, coeffs(P.wavedec, x, "db5", level=6, mode="symmetric"), "db5")
    # 2-D: the whole reconstruction of a small plane in one launch (with and without a graph of the backward), the per-level route
    c = coeffs(P.wavedec2, _z(5, 40, 36), "db2", level=3, mode="symmetric")
    rec_case("grad-waverec2-small-planes", P.waverec2, c, "db2")
    rec_case("grad-waverec2-small-planes-create-graph", P.waverec2, c, "db2", create_graph=True)
    x = _z(2, 40, 300).requires_grad_(True)
    case("grad-wavedec2-per-level", grad_of(lambda t: P.wavedec2(t, "db3", level=2, mode="reflect")), x)
    c = coeffs(P.wavedec2, x, "db3", level=2, mode="reflect")
    rec_case("grad-waverec2-per-level", P.waverec2, c, "db3")
    # only the finest level's details ask for a gradient: the coarse level is a plain call, the fine one the differentiable op
    rec_case("grad-waverec2-finest-details-only", P.waverec2, c, "db3", needs=(4, 5, 6))
    # a learnable filter bank: the per-level ops and the tap correlations
    bank = [torch.tensor(t, dtype=torch.float32, requires_grad=True) for t in _wavelets.host_taps("db2")]
    case("grad-wavedec2-learnable-bank", grad_of(lambda t, *b: P.wavedec2(t, tuple(b), level=2, mode="symmetric"), wrt=(0, 1, 2)),
         _z(2, 40, 36).requires_grad_(True), *bank)
    # the separable crop (an odd extent: the running approximation is one sample larger than the next level's details), and 3-D
    rec_case("grad-fswaverec2-odd-extent", P.fswaverec2, coeffs(P.fswavedec2, _z(2, 33, 41), "db2", level=2, mode="zero"), "db2")
    case("grad-wavedec3", grad_of(lambda t: P.wavedec3(t, "db2", level=2, mode="reflect")), _z(2, 12, 14, 20).requires_grad_(True))
    # coefficients that fail a check of the reference at the second level: the launches made before the error, its type and text
    c = coeffs(P.wavedec, _z(3, 1001), "db5", level=3, mode="reflect")
    case("error-waverec-second-level", lambda *ts: P.waverec(list(ts), "db5"), c[0], c[1], c[2], _z(3, c[3].shape[1] + 5))
    c = coeffs(P.wavedec2, _z(2, 40, 300), "db3", level=3, mode="reflect")
    bad = (c[0], c[1], type(c[2])(c[2][0], c[2][1], _z(2, c[2][2].shape[1], c[2][2].shape[2] + 1)), c[3])
    case("error-waverec2-second-level", lambda *ts: P.waverec2(rebuild_like(bad)(ts), "db3"), *tensors(bad))
    c = coeffs(P.wavedec2, _z(2, 40, 300), "db3", level=2, mode="reflect")  # (two levels go as a pair: its look-ahead raises before the launch)
    bad = (c[0], c[1], type(c[2])(c[2][0], c[2][1], _z(2, c[2][2].shape[1], c[2][2].shape[2] + 1)))
    case("error-waverec2-pair-look-ahead", lambda *ts: P.waverec2(rebuild_like(bad)(ts), "db3"), *tensors(bad))


def bound_launch_entries(real) -> set:
    """The launch entry points the three modules have bound (given argument types) on the loaded library."""
    return {n for n, f in vars(real).items() if n.startswith("mifwt_") and getattr(f, "argtypes", None) is not None and not is_query(n)}


def record() -> dict:
    r = Recorder()
    with r.stubs():
        run_cases(r)
    bound = bound_launch_entries(r.real)
    assert r.entries == bound - set(EXEMPT), ("launch entry points never reached", sorted(bound - r.entries), "unbound", sorted(r.entries - bound))
    def plan_queries(rec):  # (what only building a plan asks; the per-call envelope queries of the 1-D routes are not cached)
        return [q for q in rec["queries"] if "workspace_bytes" in q or "kernel_id" in q or q.endswith("_supported")]

    for name in ("wavedec2-twice", "waverec2-twice"):
        first, second = r.records[name]
        assert plan_queries(first) and not plan_queries(second), name  # the cache hit
        assert first["launches"] == second["launches"] and first["returns"] == second["returns"], name
    before, after = r.records["force-generic-before"][0], r.records["force-generic-after"]
    assert plan_queries(after[0]) and not plan_queries(after[1])  # plans dropped, then cached again
    assert plan_queries(before)
    refused = r.records["wavedec-3tap-refused-tail"][0]
    tail, level = "mifwt_dwt1_fwd_tail", "mifwt_dwt_fwd"  # (asked again while two levels or more remain; every level runs on its own)
    assert [l["entry"] for l in refused["launches"]] == [tail, level, tail, level, level]
    assert r.records["synthesis_tail-3tap-refused"][0]["returns"] == [None]
    signatures = {n: [getattr(f.restype, "__name__", str(f.restype))] + [t.__name__ for t in f.argtypes]
                  for n, f in sorted(vars(r.real).items()) if n.startswith("mifwt_") and getattr(f, "argtypes", None) is not None}
    return json.loads(json.dumps({"signatures": signatures, "cases": r.records}))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    got = record()
    if "--check" in sys.argv:
        with open(FIXTURE) as f:
            want = json.load(f)
        bad = [k for k in want["cases"] if got["cases"].get(k) != want["cases"][k]] + [k for k in got["cases"] if k not in want["cases"]]
        assert not bad and got["signatures"] == want["signatures"], bad
        print("engine_calls.json: %d cases match" % len(want["cases"]))
    else:
        if "--list" in sys.argv:
            for k, recs in got["cases"].items():
                print("%-42s %s" % (k, " | ".join(",".join(l["entry"][6:] for l in c["launches"]) or "-" for c in recs)))
        with open(FIXTURE, "w") as f:
            json.dump(got, f, separators=(",", ":"), sort_keys=True)
            f.write("\n")
        print("wrote %s: %d cases, %d bytes" % (FIXTURE, len(got["cases"]), os.path.getsize(FIXTURE)))
