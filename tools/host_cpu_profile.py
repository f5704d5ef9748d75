"""Host-side cost of a transform call WITHOUT a GPU: the library is replaced by the recording stand-in of tests/golden/make_engine_calls.py
(host queries answered by the real library, every launch entry point a stub that answers 0: no kernel runs, outputs stay uninitialised);
every other line of the Python path — checks, folding, plan lookup, allocations, ctypes marshalling, the launch path itself — runs as
in production.  Per case: microseconds per call (wall time, noisy on a shared CPU) and the Python-level calls per transform call
(cProfile's total call count over N calls / N: deterministic), next to the launches of the call.
usage: host_cpu_profile.py [profile]      (run from the root of the tree whose modules are to be measured)"""
import contextlib, cProfile, importlib.util, os, pstats, sys, time
sys.path.insert(0, '.')
import torch, ptwt_amd
from ptwt_amd import _bwt, _engine, stationary_transform
_spec = importlib.util.spec_from_file_location("make_engine_calls", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "make_engine_calls.py"))
M = importlib.util.module_from_spec(_spec); _spec.loader.exec_module(M)
real = _engine.load_library()
for mod in (_bwt, stationary_transform):  # (entries a module binds itself are bound on the real library first)
    if hasattr(mod, "_lib"): mod._lib()
launches = []
_engine._require_gpu = lambda t: None
torch.cuda.device = lambda dev: contextlib.nullcontext()
torch.cuda.current_device = lambda: 0
torch._C._cuda_getCurrentRawStream = lambda index: M.STREAM
_real_empty = torch.empty
_cache = {}
def _fake_empty(*a, **k):  # (allocation cost of big CPU tensors is not what a CUDA caching allocator costs: reuse one tensor per shape)
    key = (a, tuple(sorted((kk, str(v)) for kk, v in k.items())))
    t = _cache.get(key)
    if t is None:
        t = _cache[key] = _real_empty(*a, **k)
    return t
torch.empty = _fake_empty
CASES = [((4096, 64, 64), 'db2', 3, 'wavedec2'), ((4096, 64, 64), 'db2', 3, 'waverec2'), ((64, 1024, 1024), 'db4', 3, 'wavedec2'), ((64, 1024, 1024), 'db4', 3, 'waverec2'),
         ((32, 1000, 1000), 'db5', 5, 'wavedec2'), ((32, 1000, 1000), 'db5', 5, 'waverec2'), ((8, 64, 64, 64), 'db2', 3, 'wavedec3'), ((32, 100000), 'db5', 10, 'wavedec')]
N = 200
for shape, wav, lev, fn in CASES:
    x = torch.empty(*shape)
    _engine._lib = M.RecordingLib(real)
    if 'rec' in fn:
        c = getattr(ptwt_amd, fn.replace('rec', 'dec'))(x, wav, level=lev)
        call = lambda: getattr(ptwt_amd, fn)(c, wav)
    else:
        f = getattr(ptwt_amd, fn)
        call = lambda: f(x, wav, level=lev)
    for _ in range(20): call()
    t0 = time.perf_counter()
    for _ in range(500): call()
    us = 1e6 * (time.perf_counter() - t0) / 500
    pr = cProfile.Profile(); pr.enable()
    for _ in range(N): call()
    pr.disable()
    st = pstats.Stats(pr)
    _engine._lib = M.RecordingLib(real, lambda name, args: launches.append(name))  # (one more call, counting its launches)
    del launches[:]; call()
    print(f"{fn:9s} {str(shape):20s} {wav} L{lev}: host {us:6.1f} us/call, {st.total_calls / N:6.1f} Python-level calls/call, {len(launches)} launches")
    if len(sys.argv) > 1 and sys.argv[1] == fn + str(shape[0]):
        st.sort_stats("tottime").print_stats(22)
