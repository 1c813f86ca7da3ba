"""CPU-only checks: libbgs.so loads and exports every symbol include/bgs.h declares; host-side logic of the
drop-in package (JSON, value semantics, argument validation); loud failure without a GPU."""

import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    with open(os.path.join(ROOT, "include", "bgs.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    return sorted(set(re.findall(r"\b(bgs_[a-z_]+)\s*\(", text)))


LIBS = [os.path.join(ROOT, "board-game-simulator-python_amd", name) for name in ("libbgs.so", "libbgs_test.so")]


def test_library_exports_every_declared_symbol():
    from simulator.game import _abi

    names = declared_symbols()
    assert len(names) >= 30
    for path in LIBS:
        handle = ctypes.CDLL(path)
        for name in names:
            assert hasattr(handle, name), f"{os.path.basename(path)} does not export {name}"
    # the Python binding table covers exactly the header
    assert sorted(_abi.SIGNATURES) == names
    assert _abi.lib().bgs_version() >= 100


def test_dynamic_symbol_table_is_the_header():
    """libbgs.so is built with -fvisibility=hidden and a version script: `nm -D --defined-only` shows the functions
    include/bgs.h declares and nothing else -- no bgs::* helpers, no STL instantiations, no compiler markers."""
    import subprocess

    from simulator.game import _abi

    for path in LIBS:   # the product library and the test build alike
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        exported = sorted(line.split()[-1] for line in out.splitlines() if line.strip())
        assert exported == declared_symbols(), path
    with open(os.path.join(ROOT, "include", "bgs.h")) as fh:
        header = fh.read()
    # the one number the documents quote is derived from the header (DESIGN.md says "see include/bgs.h", not a count)
    assert len(exported) == len(re.findall(r"^BGS_API ", header, flags=re.M))


def test_product_library_is_lean():
    """Round-5 review: the A/B switches and the fault injection do not ship.  The product library has no BGS_EXPERIMENT parser
    (the variable's name, the switches' names and the injection messages are not in the binary), the test build has; both
    are linked from the SAME kernel objects: the kernel unit ids agree."""
    import subprocess

    product, test = (subprocess.check_output(["strings", path], text=True) for path in LIBS)
    for word in ("inject", "bounce_plan", "BGS_EXPERIMENT", "rollout_opening", "bounce_memo_policy", "gather_comm_alone", "drain_serial_sync"):
        assert word.lower() not in product.lower(), word
        assert word.lower() in test.lower(), word
    ids = []
    for path in LIBS:
        code = ("import ctypes, sys; l = ctypes.CDLL(sys.argv[1]); l.bgs_kernel_unit_id.restype = ctypes.c_char_p; "
                "l.bgs_build_id.restype = ctypes.c_char_p; print(l.bgs_build_id().decode(), *[l.bgs_kernel_unit_id(u).decode() for u in range(3)])")
        ids.append(subprocess.check_output([sys.executable, "-c", code, path], text=True).split())
    assert ids[0] == ids[1] and len(ids[0]) == 4


def test_header_is_plain_c():
    import subprocess, tempfile

    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "t.c")
        with open(src, "w") as fh:
            fh.write('#include "bgs.h"\nint main(void) { return BGS_OK; }\n')
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", src, "-o", os.path.join(tmp, "t.o")])


def test_geometry_limits_are_checked_on_the_host():
    from simulator.game import _abi

    nbytes = ctypes.c_size_t()
    lib = _abi.lib()
    assert lib.bgs_connect_arena_bytes(6, 7, 4, 1 << 20, ctypes.byref(nbytes)) == 0
    assert nbytes.value >= (1 << 20) * (16 + 1 + 2 + 42)
    # beyond the bit-packed limits the generic kernels serve the board (int8 grid in the arena) ...
    assert lib.bgs_connect_arena_bytes(16, 7, 4, 8, ctypes.byref(nbytes)) == 0 and nbytes.value >= 8 * 16 * 7
    assert lib.bgs_connect_arena_bytes(15, 13, 4, 8, ctypes.byref(nbytes)) == 0
    assert lib.bgs_connect_arena_bytes(20, 20, 5, 1000, ctypes.byref(nbytes)) == 0 and nbytes.value >= 1000 * 400
    assert lib.bgs_connect_arena_bytes(64, 64, 5, 8, ctypes.byref(nbytes)) == 0
    # ... up to the generic path's own limits
    assert lib.bgs_connect_arena_bytes(65, 7, 4, 8, ctypes.byref(nbytes)) == _abi.BGS_ERR_ARG
    assert b"height" in lib.bgs_last_error()
    assert lib.bgs_connect_arena_bytes(6, 65, 4, 8, ctypes.byref(nbytes)) == _abi.BGS_ERR_ARG
    assert lib.bgs_connect_arena_bytes(6, 7, 0, 8, ctypes.byref(nbytes)) == _abi.BGS_ERR_ARG
    assert lib.bgs_bounce_arena_bytes(9, 6, 1 << 18, ctypes.byref(nbytes)) == 0
    assert lib.bgs_bounce_arena_bytes(9, 8, 8, ctypes.byref(nbytes)) == 0 and nbytes.value >= 8 * 72
    assert lib.bgs_bounce_arena_bytes(32, 32, 8, ctypes.byref(nbytes)) == 0
    assert lib.bgs_bounce_arena_bytes(2, 6, 8, ctypes.byref(nbytes)) == _abi.BGS_ERR_ARG
    assert lib.bgs_bounce_arena_bytes(33, 32, 8, ctypes.byref(nbytes)) == _abi.BGS_ERR_ARG  # more than 1024 cells
    assert lib.bgs_bounce_arena_bytes(3, 65, 8, ctypes.byref(nbytes)) == _abi.BGS_ERR_ARG


def test_connect_host_objects():
    from simulator.game.connect import Config

    c = Config(2, 3, 2)
    assert c.to_json() == {"height": 2, "width": 3, "count": 2}
    assert Config.from_json(c.to_json()) == c and hash(Config(2, 3, 2)) == hash(c)
    assert Config(2, 3, 2) < Config(2, 3, 3) < Config(2, 4, 1) and Config(2, 3, 2) >= c
    assert Config.num_players == 2
    with pytest.raises(TypeError):
        Config(2.0, 3, 2)
    assert Config(40, 40, 4).to_json() == {"height": 40, "width": 40, "count": 4}  # served by the generic kernels
    with pytest.raises(ValueError):
        Config(65, 40, 4)
    with pytest.raises(RuntimeError):
        Config.from_json({"height": 2})
    with pytest.raises(AttributeError):
        c.height = 3


def test_bounce_host_objects():
    from simulator.game.bounce import Config

    grid = np.zeros((9, 6), dtype=np.int64)
    grid[1] = grid[7] = [1, 2, 3, 3, 2, 1]
    c = Config(grid)
    assert c.grid.dtype == np.int8 and c.to_json() == {"grid": grid.tolist()}
    assert Config.from_json(c.to_json()) == c and hash(Config(grid.astype(np.int8))) == hash(c)
    grid[0, 0] = 1
    with pytest.raises(RuntimeError):
        Config(grid)  # piece in a goal row
    with pytest.raises(TypeError):
        Config(np.zeros((9, 6), dtype=np.float32))
    with pytest.raises(TypeError):
        Config(np.zeros((2, 3, 4), dtype=np.int8))


def test_no_gpu_means_loud_failure_not_a_fallback():
    from simulator.game import _abi

    if _abi.device_count() > 0:
        pytest.skip("a GPU is visible here")
    from simulator.batch import ConnectBatch
    from simulator.game.connect import Config

    with pytest.raises(_abi.BgsError) as err:
        ConnectBatch(6, 7, 4, 16)
    assert err.value.code == _abi.BGS_ERR_NO_DEVICE
    with pytest.raises(RuntimeError):
        Config(6, 7, 4).sample_initial_state()


def test_product_package_never_touches_the_oracle():
    pkg = os.path.join(ROOT, "board-game-simulator-python_amd")
    for base, _, files in os.walk(pkg):
        for name in files:
            if name.endswith((".py", ".hip", ".h", ".cpp", "Makefile")):
                with open(os.path.join(base, name)) as fh:
                    text = fh.read()
                assert "liboracle" not in text and "import oracle" not in text and "from oracle" not in text, name


def test_progress_words_wake_sleepers_and_never_move_backwards():
    """bgs_progress_store / bgs_progress_wait (the futex-backed counters the shared reward array and the sinks use): a
    sleeper wakes when every word has reached the target, a lower store does not lower a word, a wait times out with the
    laggard's index."""
    import ctypes
    import threading
    import time

    import numpy as np

    from simulator.game import _abi

    lib = _abi.lib()
    words = np.zeros((3, 8), dtype=np.int64)  # one word per cache line, as in SharedRewardRing
    base = words.ctypes.data
    woke = []

    def sleeper():
        rc = lib.bgs_progress_wait(ctypes.c_void_p(base), 3, 8, 5, 10000, None)
        woke.append((rc, time.monotonic()))

    t = threading.Thread(target=sleeper)
    t.start()
    time.sleep(0.1)
    assert not woke
    for r in (2, 0):
        _abi.check(lib.bgs_progress_store(ctypes.c_void_p(base + 64 * r), 7))
    time.sleep(0.1)
    assert not woke  # word 1 is still behind
    t_store = time.monotonic()
    _abi.check(lib.bgs_progress_store(ctypes.c_void_p(base + 64), 5))
    t.join(timeout=5)
    assert woke and woke[0][0] == 0 and woke[0][1] - t_store < 0.5
    _abi.check(lib.bgs_progress_store(ctypes.c_void_p(base), 3))
    assert words[0, 0] == 7  # never lowered
    laggard = ctypes.c_int64(-1)
    t0 = time.monotonic()
    rc = lib.bgs_progress_wait(ctypes.c_void_p(base), 3, 8, 6, 150, ctypes.byref(laggard))
    assert rc == _abi.BGS_ERR_RUNTIME and laggard.value == 1 and 0.1 < time.monotonic() - t0 < 2.0
    assert "timed out" in _abi.last_error()
    assert lib.bgs_progress_wait(ctypes.c_void_p(base + 4), 1, 1, 0, 0, None) == _abi.BGS_ERR_ARG  # misaligned


def test_engine_cache_evicts_least_recently_used_per_thread():
    """simulator.game._engine.EngineCache (host logic, no GPU): bounded per thread, least recently used out first and
    closed, threads do not see each other's engines."""
    import threading

    from simulator.game import _engine

    class Fake:
        closed = 0

        def __init__(self, key):
            self.key = key

        def close(self):
            Fake.closed += 1

    cache = _engine.EngineCache()
    cap = _engine.MAX_ENGINES_PER_THREAD
    first = cache.get(0, lambda: Fake(0))
    for k in range(1, cap):
        cache.get(k, lambda k=k: Fake(k))
    assert cache.get(0, lambda: Fake("again")) is first and Fake.closed == 0   # 0 is now the most recently used
    cache.get(cap, lambda: Fake(cap))                                          # one too many: key 1 goes, not key 0
    assert Fake.closed == 1 and cache.get(0, lambda: Fake("again")) is first
    assert cache.get(1, lambda: Fake("new 1")).key == "new 1"
    seen = []
    t = threading.Thread(target=lambda: seen.append(cache.get(0, lambda: Fake("other thread")).key))
    t.start(); t.join()
    assert seen == ["other thread"]


def test_progress_barrier_between_threads():
    """bgs_progress_barrier on words in this process's memory: four threads, ten barriers, some arriving late (spinning
    and sleeping waiters), nobody through before the last arrival; bad arguments and a missing participant are reported."""
    import ctypes
    import threading
    import time

    import numpy as np

    from simulator.game import _abi

    lib = _abi.lib()
    parties, rounds = 4, 10
    words = np.zeros((parties, 8), dtype=np.int64)
    base = words.ctypes.data
    arrived = np.zeros((rounds, parties))
    passed = np.zeros((rounds, parties))
    errors = []

    def party(me):
        for epoch in range(1, rounds + 1):
            time.sleep(0.002 * ((me + epoch) % parties))
            arrived[epoch - 1, me] = time.monotonic()
            rc = lib.bgs_progress_barrier(ctypes.c_void_p(base), parties, 8, me, epoch, 100 if epoch % 2 else 0, 5000)
            passed[epoch - 1, me] = time.monotonic()
            if rc != 0:
                errors.append((me, epoch, rc))

    threads = [threading.Thread(target=party, args=(k,)) for k in range(parties)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    assert (passed.min(axis=1) >= arrived.max(axis=1) - 1e-4).all()
    assert (words[:, 0] == rounds).all()
    # a participant that never comes: timeout; nonsense arguments: BGS_ERR_ARG
    assert lib.bgs_progress_barrier(ctypes.c_void_p(base), parties, 8, 0, rounds + 1, 50, 100) != 0
    assert "timed out" in _abi.last_error()
    assert lib.bgs_progress_barrier(ctypes.c_void_p(base), parties, 8, parties, 1, 0, 100) == _abi.BGS_ERR_ARG
    assert lib.bgs_progress_barrier(None, 1, 8, 0, 1, 0, 100) == _abi.BGS_ERR_ARG
