"""The surface of simulator/batch.py that needs no device: the signatures of the two batch classes and the four
tree-object classes, the library call every host form of an analysis method makes -- entry point, scalars in ABI order,
the returned arrays as the pointer arguments, the trailing workspace / on_device values --, the forests' size query,
restart rule, `advance` and refusals, the size queries, and the refusals that are made before the library is reached.

Everything below was written down from batch.py as it was before the host and tensor forms of a call were given one
body and the forest and guided classes one base each, and this file passed against that batch.py unedited: it is the
record that the surface did not move.

`_abi.lib` is replaced by a stand-in whose every attribute is a function that records (name, args) and returns 0 (a
`*_bytes` query also answers BYTES through its last argument).  Batches are made with `object.__new__` and
`_Batch.__init__`, so no library and no device is touched.  The forests allocate through `batch._torch`; it is a stand-in
too, as small as they need: `zeros` that drops `device`, on numpy memory.  The guided searches' calls and every tensor
form need device tensors: they stay with the GPU tests.
"""

import ctypes
import inspect
from types import SimpleNamespace

import numpy as np
import pytest

from simulator import batch as bm
from simulator.game import _abi

BYTES = 4096                                    # what every size query of the stand-in answers
UNIFORM, DECISIVE = _abi.POLICY_UNIFORM, _abi.POLICY_DECISIVE


class Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            if name.endswith("_bytes"):
                args[-1]._obj.value = BYTES     # (the size_t behind ctypes.byref)
            self.calls.append((name, args))
            return 0
        return call

    def take(self):
        """the one call recorded since the last look: (name, [the handle, the other args with ctypes scalars as their values])"""
        (name, args), = self.calls
        self.calls = []
        return name, [args[0]] + [a.value if isinstance(a, ctypes._SimpleCData) else a for a in args[1:]]


@pytest.fixture
def lib(monkeypatch):
    recorder = Recorder()
    monkeypatch.setattr(_abi, "lib", lambda: recorder)
    return recorder


class HostTensor:
    """what a forest asks of its buffer: an address and a length"""

    def __init__(self, array):
        self.array = array

    def data_ptr(self):
        return self.array.ctypes.data

    def numel(self):
        return self.array.size


TORCH = SimpleNamespace(uint8=np.uint8, zeros=lambda n, dtype, device: HostTensor(np.zeros(n, dtype=dtype)))


def connect_batch(height, width, torch=None):
    b = object.__new__(bm.ConnectBatch)
    bm._Batch.__init__(b, 3, height, width, 0, False)
    b._torch = torch
    return b


def bounce_batch(torch=None):
    b = object.__new__(bm.BounceBatch)
    bm._Batch.__init__(b, 2, 5, 4, 0, False)
    b._torch = torch
    return b


# ---- signatures
SEED = "seed: 'int' = 81985529216486895"
CAP = "max_plies: 'int' = 2147483647"
POLICY = "policy: 'str' = 'uniform'"
EVALUATE = f"{SEED}, playouts: 'int' = 256, {CAP}, {POLICY}"
HALVING = f"{SEED}, budget: 'int' = 1024, {CAP}, {POLICY}"
SEARCH = f"{SEED}, iterations: 'int' = 256, leaf_playouts: 'int' = 64, explore: 'int' = 65536, {CAP}, {POLICY}"
EDGES = "edges: 'Optional[int]' = None"
SOLVE = "max_nodes: 'int' = 1048576, with_plies: 'bool' = True"
ROLLOUT = f"{SEED}, {CAP}, from_initial: 'bool' = False"
EVENT = "event: 'Optional[HostEvent]' = None"
SELF, OUT, STUB = "(self)", "(self, out=None)", "(self, *args, **kwargs)"
COMMON = {
    "action_count_tensor": OUT,
    "buffer": "(self, buffer_id: 'int')",
    "close": SELF,
    "device_view": "(self, what: 'str' = 'reward')",
    "env_step": "(self, actions, observation=None, ended=None, reward=None, status=None, auto_reset: 'bool' = True)",
    "from_json_states": "(self, states)",
    "grid_tensor": OUT,
    "one_board_call": SELF,
    "outcomes_tensor": OUT,
    "read_outcomes_async": f"(self, host_dst, {EVENT})",
    "read_reward_async": f"(self, host_dst, {EVENT})",
    "reset": SELF,
    "reset_steps": SELF,
    "reward_copy_tensor": OUT,
    "reward_tensor": SELF,
    "rollout": f"(self, {ROLLOUT})",
    "rollout_outcomes_tensor": f"(self, out, {ROLLOUT})",
    "rollout_to_host": f"(self, host_dst, {ROLLOUT}, codes: 'bool' = False, {EVENT})",
    "set_first_game": "(self, first_game: 'int')",
    "set_launches_in_flight": "(self, launches: 'int')",
    "set_rng_contract": "(self, contract: 'str')",
    "set_stream": "(self, hip_stream: 'int')",
    "status_tensor": SELF,
    "step_actions_observe": "(self, actions, observation=None, ended=None, status=None)",
    "step_random": f"(self, {SEED}, plies: 'int' = 1)",
    "steps_tensor": SELF,
    "synchronize": SELF,
    "to_json_states": SELF,
    "transition": "(self, grid=None, player=None, winner=None, plies=None, actions=None)",
    "write_state": "(self, grid, player=None, winner=None, plies=None)",
}
CONNECT = {
    "__init__": "(self, height: 'int', width: 'int', count: 'int', n: 'int', device: 'int' = 0, use_torch: 'Optional[bool]' = None)",
    "evaluate_actions": f"(self, {EVALUATE})",
    "evaluate_actions_halving": f"(self, {HALVING})",
    "evaluate_actions_halving_tensor": f"(self, counts=None, given=None, best=None, {HALVING})",
    "evaluate_actions_tensor": f"(self, out=None, {EVALUATE})",
    "evaluate_moves_halving": STUB,
    "evaluate_moves_halving_tensor": STUB,
    "forest_bytes": "(self, capacity: 'int')",
    "guided_bytes": "(self, capacity: 'int')",
    "guided_search": "(self, capacity: 'int', cpuct: 'int' = 320)",
    "halving_min_budget": SELF,
    "legal_tensor": OUT,
    "search_actions": f"(self, {SEARCH})",
    "search_actions_proving": f"(self, {SEARCH})",
    "search_actions_proving_tensor": f"(self, counts=None, visits=None, best=None, nodes=None, proved=None, done=None, {SEARCH}, workspace=None)",
    "search_actions_tensor": f"(self, counts=None, visits=None, best=None, nodes=None, {SEARCH}, workspace=None)",
    "search_forest": "(self, capacity: 'int')",
    "search_moves": STUB,
    "search_moves_proving": STUB,
    "search_moves_proving_tensor": STUB,
    "search_moves_tensor": STUB,
    "search_moves_workspace_bytes": STUB,
    "search_workspace_bytes": "(self, iterations: 'int' = 256)",
    "solve_actions": f"(self, depth: 'Optional[int]' = None, {SOLVE})",
    "solve_actions_tensor": f"(self, codes=None, plies=None, depth: 'Optional[int]' = None, {SOLVE})",
    "solve_moves": STUB,
    "solve_moves_tensor": STUB,
    "step_actions": "(self, columns, want_status: 'bool' = True)",
}
BOUNCE = {
    "__init__": "(self, grid, n: 'int', device: 'int' = 0, use_torch: 'Optional[bool]' = None)",
    "decode_moves": "(self, legal_row, winner: 'int')",
    "evaluate_actions": STUB,
    "evaluate_actions_halving": STUB,
    "evaluate_actions_halving_tensor": STUB,
    "evaluate_actions_tensor": STUB,
    "evaluate_moves": f"(self, {EVALUATE})",
    "evaluate_moves_halving": f"(self, {HALVING})",
    "evaluate_moves_halving_tensor": f"(self, counts=None, given=None, best=None, {HALVING})",
    "evaluate_moves_tensor": f"(self, out=None, {EVALUATE})",
    "forest_bytes": STUB,
    "guided_bytes": STUB,
    "guided_default_edges": "(self, nodes: 'int')",
    "guided_moves_bytes": f"(self, nodes: 'int', {EDGES})",
    "guided_moves_search": f"(self, nodes: 'int', {EDGES}, cpuct: 'int' = 320, max_plies: 'int' = 65535)",
    "guided_search": STUB,
    "halving_min_budget": "(moves: 'int')",
    "moves_forest_bytes": f"(self, nodes: 'int', {EDGES})",
    "search_actions": STUB,
    "search_actions_proving": STUB,
    "search_actions_proving_tensor": STUB,
    "search_actions_tensor": STUB,
    "search_default_edges": "(self, iterations: 'int')",
    "search_forest": STUB,
    "search_min_edges": SELF,
    "search_moves": f"(self, {SEARCH}, {EDGES})",
    "search_moves_forest": f"(self, nodes: 'int', {EDGES})",
    "search_moves_proving": f"(self, {SEARCH}, {EDGES})",
    "search_moves_proving_tensor": f"(self, counts=None, visits=None, best=None, nodes=None, used=None, proved=None, done=None, {SEARCH}, {EDGES}, workspace=None)",
    "search_moves_tensor": f"(self, counts=None, visits=None, best=None, nodes=None, used=None, {SEARCH}, {EDGES}, workspace=None)",
    "search_moves_workspace_bytes": f"(self, iterations: 'int' = 256, {EDGES})",
    "search_workspace_bytes": STUB,
    "slots_to_moves": "(self, slots)",
    "slots_to_moves_tensor": "(self, slots, targets=None)",
    "solve_actions": STUB,
    "solve_actions_tensor": STUB,
    "solve_moves": f"(self, depth: 'int' = 3, {SOLVE})",
    "solve_moves_tensor": f"(self, codes=None, plies=None, depth: 'int' = 3, {SOLVE})",
    "step_actions": "(self, moves, want_status: 'bool' = True)",
    "targets_tensor": OUT,
}
GUIDED = {"begin": SELF, "close": SELF, "finish": "(self, priors, values)", "run": "(self, evaluate, simulations: 'int')",
          "step": "(self, priors, values)"}
SIGNATURES = {
    "ConnectBatch": {**COMMON, **CONNECT},
    "BounceBatch": {**COMMON, **BOUNCE},
    "SearchForest": {
        "__init__": "(self, batch: 'ConnectBatch', capacity: 'int')",
        "advance": "(self, columns)",
        "advance_tensor": "(self, columns, kept=None)",
        "close": SELF,
        "search": f"(self, {SEARCH}, restart: 'bool' = False)",
        "search_tensor": f"(self, counts=None, visits=None, best=None, nodes=None, carried=None, {SEARCH}, restart: 'bool' = False)",
    },
    "MovesForest": {
        "__init__": f"(self, batch: 'BounceBatch', nodes: 'int', {EDGES})",
        "advance": "(self, slots)",
        "advance_tensor": "(self, slots, kept=None)",
        "close": SELF,
        "search": f"(self, {SEARCH}, restart: 'bool' = False)",
        "search_tensor": f"(self, counts=None, visits=None, best=None, nodes=None, used=None, carried=None, {SEARCH}, restart: 'bool' = False)",
    },
    # (the two guided constructors quote the batch's class inside an annotation that is a string already)
    "GuidedSearch": {"__init__": "(self, batch: \"'ConnectBatch'\", capacity: 'int', cpuct: 'int' = 320)", **GUIDED},
    "GuidedMovesSearch": {"__init__": f"(self, batch: \"'BounceBatch'\", nodes: 'int', {EDGES}, cpuct: 'int' = 320, "
                                      "max_plies: 'int' = 65535)", **GUIDED},
}
# every public method has a docstring, but for the constructors and these one-liners of the lifetime and rollout part
UNDOCUMENTED = {"__init__", "close", "legal_tensor", "one_board_call", "reset", "reset_steps", "rollout", "set_stream",
                "status_tensor", "synchronize"}


@pytest.mark.parametrize("name", list(SIGNATURES))
def test_signatures_are_the_table(name):
    cls = getattr(bm, name)
    methods = sorted(n for n, value in inspect.getmembers(cls) if callable(value) and (n == "__init__" or not n.startswith("_")))
    assert methods == sorted(SIGNATURES[name])
    for method in methods:
        signature = inspect.signature(getattr(cls, method)).replace(return_annotation=inspect.Signature.empty)
        assert str(signature) == SIGNATURES[name][method], method
        documented = bool(getattr(cls, method).__doc__ and getattr(cls, method).__doc__.strip())
        assert documented == (method not in UNDOCUMENTED), method
    assert cls.__doc__ and cls.__doc__.strip()


# ---- host forms: (method, keywords, entry point, scalars behind the handle, outputs, what follows the outputs)
# outputs are (a shape with "n" and "row" to be filled in, dtype), or None for an output that is not returned and goes
# to the library as NULL; every scalar has a value of its own that is not the default
I8, I16, I32 = np.int8, np.int16, np.int32
ROW, ROW3 = ("row",), ("row", 3)                # an entry a column (Connect) or a move slot (Bounce), and three counts each
SEARCHED = dict(seed=11, iterations=15, leaf_playouts=16, explore=17, max_plies=13, policy="decisive")
SEARCH_OUT = [(ROW3, I32), (ROW, I32), ((), I32), ((), I32)]
PROVING_OUT = [(ROW, I8), ((), I32)]
SOLVE_OUT = [(ROW, I8), (ROW, I16)]
CONNECT_CALLS = [
    ("evaluate_actions", dict(seed=11, playouts=12, max_plies=13), "bgs_connect_evaluate_actions", [11, 12, 13], [(ROW3, I32)], [0]),
    ("evaluate_actions", dict(seed=11, playouts=12, max_plies=13, policy="decisive"), "bgs_connect_evaluate_actions_policy",
     [11, 12, 13, DECISIVE], [(ROW3, I32)], [0]),
    ("evaluate_actions_halving", dict(seed=11, budget=14, max_plies=13, policy="decisive"), "bgs_connect_evaluate_actions_halving",
     [11, 14, 13, DECISIVE], [(ROW3, I32), (ROW, I32), ((), I32)], [0]),
    ("evaluate_actions_halving", dict(seed=11, budget=14, max_plies=13), "bgs_connect_evaluate_actions_halving",
     [11, 14, 13, UNIFORM], [(ROW3, I32), (ROW, I32), ((), I32)], [0]),
    ("search_actions", SEARCHED, "bgs_connect_search_actions", [11, 15, 16, 17, 13, DECISIVE], SEARCH_OUT, [None, 0, 0]),
    ("search_actions_proving", SEARCHED, "bgs_connect_search_actions_proving", [11, 15, 16, 17, 13, DECISIVE],
     SEARCH_OUT + PROVING_OUT, [None, 0, 0]),
    ("solve_actions", dict(depth=5, max_nodes=18), "bgs_connect_solve_actions", [5, 18], SOLVE_OUT, [None, 0]),
    ("solve_actions", dict(depth=5, max_nodes=18, with_plies=False), "bgs_connect_solve_actions", [5, 18], [(ROW, I8), None], [None, 0]),
]
BOUNCE_CALLS = [
    ("evaluate_moves", dict(seed=11, playouts=12, max_plies=13), "bgs_bounce_evaluate_moves", [11, 12, 13], [(ROW3, I32)], [0]),
    ("evaluate_moves", dict(seed=11, playouts=12, max_plies=13, policy="decisive"), "bgs_bounce_evaluate_moves_policy",
     [11, 12, 13, DECISIVE], [(ROW3, I32)], [0]),
    ("evaluate_moves_halving", dict(seed=11, budget=14, max_plies=13, policy="decisive"), "bgs_bounce_evaluate_moves_halving",
     [11, 14, 13, DECISIVE], [(ROW3, I32), (ROW, I32), ((), I32)], [0]),
    ("search_moves", dict(SEARCHED, edges=190), "bgs_bounce_search_moves", [11, 15, 16, 17, 13, DECISIVE, 190],
     SEARCH_OUT + [((), I32)], [None, 0, 0]),
    ("search_moves_proving", dict(SEARCHED, edges=190), "bgs_bounce_search_moves_proving", [11, 15, 16, 17, 13, DECISIVE, 190],
     SEARCH_OUT + [((), I32)] + PROVING_OUT, [None, 0, 0]),
    # edges=None: min((T + 1) * MIN, MIN + 32 * T) with MIN = 4 * 4 * (5 - 2) = 48 and T = 3 iterations
    ("search_moves", dict(seed=11, iterations=3), "bgs_bounce_search_moves", [11, 3, 64, 65536, 2**31 - 1, UNIFORM, 144],
     SEARCH_OUT + [((), I32)], [None, 0, 0]),
    ("search_moves_proving", dict(seed=11, iterations=3), "bgs_bounce_search_moves_proving", [11, 3, 64, 65536, 2**31 - 1, UNIFORM, 144],
     SEARCH_OUT + [((), I32)] + PROVING_OUT, [None, 0, 0]),
    ("solve_moves", dict(depth=5, max_nodes=18), "bgs_bounce_solve_moves", [5, 18], SOLVE_OUT, [None, 0]),
    ("solve_moves", dict(depth=5, max_nodes=18, with_plies=False), "bgs_bounce_solve_moves", [5, 18], [(ROW, I8), None], [None, 0]),
]


def check_call(lib, b, row, got, entry, scalars, outputs, tail):
    """the one recorded call is `entry`(handle, *scalars, the arrays of `got` (or NULL), *tail); `got` has the shapes"""
    got = got if isinstance(got, tuple) else (got,)
    name, args = lib.take()
    assert name == entry
    assert args[0] is b._handle
    assert args[1:1 + len(scalars)] == scalars
    assert len(got) == len(outputs)
    for array, output in zip(got, outputs):
        if output is None:
            assert array is None
            continue
        shape, dtype = output
        assert isinstance(array, np.ndarray) and array.dtype == dtype and array.flags.c_contiguous
        assert array.shape == (b.n,) + tuple(x for part in shape for x in (row if part == "row" else (part,)))
    assert args[1 + len(scalars):-len(tail)] == [None if array is None else array.ctypes.data for array in got]
    assert args[-len(tail):] == tail
    assert len({array.ctypes.data for array in got if array is not None}) == sum(array is not None for array in got)


@pytest.mark.parametrize("shape", [(6, 7), (3, 4)], ids=["6x7", "3x4"])
@pytest.mark.parametrize("case", CONNECT_CALLS, ids=[f"{c[0]}-{c[2]}-{len(c[4])}{'' if all(c[4]) else '-no-plies'}" for c in CONNECT_CALLS])
def test_connect_host_forms_make_their_call(lib, shape, case):
    method, keywords, entry, scalars, outputs, tail = case
    b = connect_batch(*shape)
    check_call(lib, b, (b.width,), getattr(b, method)(**keywords), entry, scalars, outputs, tail)


@pytest.mark.parametrize("case", BOUNCE_CALLS, ids=[f"{c[0]}-{c[2]}-{c[3][-1]}{'' if all(c[4]) else '-no-plies'}" for c in BOUNCE_CALLS])
def test_bounce_host_forms_make_their_call(lib, case):
    method, keywords, entry, scalars, outputs, tail = case
    b = bounce_batch()
    check_call(lib, b, (4, 20), getattr(b, method)(**keywords), entry, scalars, outputs, tail)


def test_a_full_connect_solve_takes_the_cells_as_its_depth(lib):
    b = connect_batch(3, 4)
    check_call(lib, b, (4,), b.solve_actions(), "bgs_connect_solve_actions", [12, bm.DEFAULT_SOLVE_NODES], SOLVE_OUT, [None, 0])


def test_the_proving_search_passes_sixteen_arguments(lib):
    connect_batch(6, 7).search_actions_proving()
    assert len(lib.calls[0][1]) == 16


# ---- size queries
def test_size_queries(lib):
    c, b = connect_batch(6, 7), bounce_batch()
    for query, entry, scalars in [
        (lambda: c.search_workspace_bytes(15), "bgs_connect_search_workspace_bytes", [15]),
        (lambda: c.search_workspace_bytes(), "bgs_connect_search_workspace_bytes", [256]),
        (lambda: c.forest_bytes(9), "bgs_connect_forest_bytes", [9]),
        (lambda: c.guided_bytes(10), "bgs_connect_guided_bytes", [10]),
        (lambda: b.search_moves_workspace_bytes(15, 190), "bgs_bounce_search_workspace_bytes", [15, 190]),
        (lambda: b.search_moves_workspace_bytes(3), "bgs_bounce_search_workspace_bytes", [3, 144]),
        (lambda: b.moves_forest_bytes(6, 190), "bgs_bounce_forest_bytes", [6, 190]),
        (lambda: b.moves_forest_bytes(6), "bgs_bounce_forest_bytes", [6, 208]),         # search_default_edges(5): 48 + 32 * 5
        (lambda: b.guided_moves_bytes(5, 190), "bgs_bounce_guided_bytes", [5, 190]),
        (lambda: b.guided_moves_bytes(5), "bgs_bounce_guided_bytes", [5, 176]),         # guided_default_edges(5): 48 + 32 * 4
    ]:
        got = query()
        name, args = lib.take()
        assert (got, name, args[1:-1]) == (BYTES, entry, scalars) and type(got) is int
        assert args[0] is (c if "connect" in entry else b)._handle and type(args[-1]).__name__ == "CArgObject"


# ---- forests
def forest_search(lib, forest, sizes, restart, want, **keywords):
    b = forest.batch
    row = (b.width,) if isinstance(b, bm.ConnectBatch) else (b.width, b.height * b.width)
    game = "connect" if isinstance(b, bm.ConnectBatch) else "bounce"
    used = [] if game == "connect" else [((), I32)]
    check_call(lib, b, row, forest.search(restart=restart, **keywords), f"bgs_{game}_forest_search",
               [11, 15, 16, 17, 13, DECISIVE] + sizes + [want], SEARCH_OUT + used + [((), I32)],
               [forest._buffer.data_ptr(), BYTES, 0])


@pytest.mark.parametrize("game", ["connect", "bounce"])
def test_forests(lib, game):
    if game == "connect":
        b = connect_batch(6, 7, TORCH)
        forest, sizes, entry, what = b.search_forest(9), [9], "bgs_connect_forest_bytes", "columns"
        assert type(forest) is bm.SearchForest and forest.capacity == 9
    else:
        b = bounce_batch(TORCH)
        forest, sizes, entry, what = b.search_moves_forest(6), [6, 208], "bgs_bounce_forest_bytes", "slots"
        assert type(forest) is bm.MovesForest and (forest.nodes, forest.edges) == (6, 208)
        assert bm.MovesForest(b, 6, 190).edges == 190
        lib.calls.pop()
    assert forest.batch is b
    name, args = lib.take()
    assert (name, args[1:-1]) == (entry, sizes) and args[0] is b._handle
    assert forest._buffer.numel() == BYTES and not forest._buffer.array.any()
    # the first search restarts every tree, whatever `restart` says; later ones do as they are told
    forest_search(lib, forest, sizes, False, 1, **SEARCHED)
    forest_search(lib, forest, sizes, False, 0, **SEARCHED)
    forest_search(lib, forest, sizes, True, 1, **SEARCHED)
    # advance: the caller's int32 array and the returned one are the pointers
    moves = np.arange(b.n, dtype=np.int32)
    kept = forest.advance(moves)
    name, args = lib.take()
    assert name == f"bgs_{game}_forest_advance"
    assert args == [b._handle, moves.ctypes.data] + sizes + [kept.ctypes.data, forest._buffer.data_ptr(), BYTES, 0]
    assert kept.shape == (b.n,) and kept.dtype == np.int32
    assert forest.advance(list(range(b.n))).shape == (b.n,)             # (anything numpy makes int32[n] of)
    lib.take()
    for wrong in (np.zeros(b.n + 1, dtype=np.int32), np.zeros((b.n, 1), dtype=np.int32), 0):
        with pytest.raises(TypeError) as refusal:
            forest.advance(wrong)
        assert str(refusal.value) == f"{what} must be int32[{b.n}]"
    with pytest.raises(ValueError, match="unknown playout policy 'greedy'"):
        forest.search(policy="greedy")
    assert lib.calls == []
    forest.close()
    assert forest._buffer is None
    for call in (forest.search, lambda: forest.advance(moves)):
        with pytest.raises(RuntimeError) as refusal:
            call()
        assert str(refusal.value) == "the forest is closed"
    forest.close()                                                      # (twice is fine)
    assert lib.calls == []


def test_a_forest_without_torch_names_the_method_that_makes_it(lib):
    for b, make, who in ((connect_batch(6, 7), lambda b: b.search_forest(9), "search_forest"),
                         (bounce_batch(), lambda b: b.search_moves_forest(6), "search_moves_forest")):
        with pytest.raises(RuntimeError) as refusal:
            make(b)
        assert str(refusal.value) == f"{who} needs torch with a GPU"
        assert [name for name, _ in lib.calls] == [f"bgs_{'connect' if who == 'search_forest' else 'bounce'}_forest_bytes"]
        lib.calls = []


# ---- refusals that reach neither an allocation nor the library
UNKNOWN = "unknown playout policy 'greedy': one of ['decisive', 'uniform']"
CONNECT_POLICY = ["evaluate_actions", "evaluate_actions_tensor", "evaluate_actions_halving", "evaluate_actions_halving_tensor",
                  "search_actions", "search_actions_tensor", "search_actions_proving", "search_actions_proving_tensor"]
BOUNCE_POLICY = ["evaluate_moves", "evaluate_moves_tensor", "evaluate_moves_halving", "evaluate_moves_halving_tensor",
                 "search_moves", "search_moves_tensor", "search_moves_proving", "search_moves_proving_tensor"]


def test_an_unknown_policy_is_refused_before_anything_else(lib, monkeypatch):
    monkeypatch.setattr(np, "empty", None)                              # (nothing is allocated either)
    for b, methods in ((connect_batch(6, 7), CONNECT_POLICY), (bounce_batch(), BOUNCE_POLICY)):
        for method in methods:                                          # (no torch: the tensor forms would say so next)
            for policy in ("greedy", None):
                with pytest.raises(ValueError) as refusal:
                    getattr(b, method)(policy=policy)
                assert str(refusal.value) == UNKNOWN.replace("'greedy'", repr(policy))
    assert lib.calls == []


def test_a_tensor_form_without_torch_names_itself(lib):
    for b, methods in ((connect_batch(6, 7), CONNECT_POLICY + ["solve_actions_tensor"]), (bounce_batch(), BOUNCE_POLICY + ["solve_moves_tensor"])):
        for method in methods:
            if method.endswith("_tensor"):
                with pytest.raises(RuntimeError) as refusal:
                    getattr(b, method)()
                assert str(refusal.value) == f"{method} needs torch with a GPU"
    assert lib.calls == []


OTHER_GAME = {
    "ConnectBatch": {
        "solve_moves": "solve_moves: Bounce batches only (Connect boards: solve_actions)",
        "solve_moves_tensor": "solve_moves: Bounce batches only (Connect boards: solve_actions)",
        "evaluate_moves_halving": "evaluate_moves_halving: Bounce batches only (Connect boards: evaluate_actions_halving)",
        "evaluate_moves_halving_tensor": "evaluate_moves_halving: Bounce batches only (Connect boards: evaluate_actions_halving)",
        "search_moves": "search_moves: Bounce batches only (Connect boards: search_actions)",
        "search_moves_tensor": "search_moves: Bounce batches only (Connect boards: search_actions)",
        "search_moves_workspace_bytes": "search_moves: Bounce batches only (Connect boards: search_actions)",
        "search_moves_proving": "search_moves_proving: Bounce batches only (Connect boards: search_actions_proving)",
        "search_moves_proving_tensor": "search_moves_proving: Bounce batches only (Connect boards: search_actions_proving)",
    },
    "BounceBatch": {
        "evaluate_actions": "evaluate_actions: Connect batches only (Bounce boards: evaluate_moves)",
        "evaluate_actions_tensor": "evaluate_actions: Connect batches only (Bounce boards: evaluate_moves)",
        "evaluate_actions_halving": "evaluate_actions_halving: Connect batches only (Bounce boards: evaluate_moves)",
        "evaluate_actions_halving_tensor": "evaluate_actions_halving: Connect batches only (Bounce boards: evaluate_moves)",
        "search_actions": "search_actions: Connect batches only (Bounce boards: evaluate_moves_halving)",
        "search_actions_tensor": "search_actions: Connect batches only (Bounce boards: evaluate_moves_halving)",
        "search_workspace_bytes": "search_actions: Connect batches only (Bounce boards: evaluate_moves_halving)",
        "search_actions_proving": "search_actions_proving: Connect batches only (Bounce boards: search_moves_proving)",
        "search_actions_proving_tensor": "search_actions_proving: Connect batches only (Bounce boards: search_moves_proving)",
        "search_forest": "search_forest: Connect batches only (Bounce boards: search_moves)",
        "forest_bytes": "search_forest: Connect batches only (Bounce boards: search_moves)",
        "guided_search": "guided_search: Connect batches only",
        "guided_bytes": "guided_search: Connect batches only",
        "solve_actions": "solve_actions: Connect batches only",
        "solve_actions_tensor": "solve_actions: Connect batches only",
    },
}


def test_the_other_games_calls_say_where_to_go(lib):
    for b in (connect_batch(6, 7), bounce_batch()):
        stubs = OTHER_GAME[type(b).__name__]
        assert sorted(stubs) == sorted(m for m, s in SIGNATURES[type(b).__name__].items() if s == STUB)
        for method, text in stubs.items():
            for arguments in ((), (1, 2)):
                with pytest.raises(ValueError) as refusal:
                    getattr(b, method)(*arguments, seed=3)
                assert str(refusal.value) == text
    assert lib.calls == []


def test_guided_constructors_refuse_their_ranges_first(lib):
    c, b = connect_batch(6, 7), bounce_batch()
    for cpuct in (-1, 4097):
        text = f"cpuct must be 0 .. 4096, c_puct in Q8 (got {cpuct})"
        for make in (lambda: bm.GuidedSearch(c, 9, cpuct), lambda: c.guided_search(9, cpuct=cpuct),
                     lambda: bm.GuidedMovesSearch(b, 6, None, cpuct), lambda: b.guided_moves_search(6, cpuct=cpuct, max_plies=0)):
            with pytest.raises(ValueError) as refusal:
                make()
            assert str(refusal.value) == text
    for max_plies in (0, -5):
        for make in (lambda: bm.GuidedMovesSearch(b, 6, max_plies=max_plies), lambda: b.guided_moves_search(6, 190, 320, max_plies)):
            with pytest.raises(ValueError) as refusal:
                make()
            assert str(refusal.value) == f"max_plies must be >= 1 (got {max_plies})"
    assert lib.calls == []
    # in range, and no torch: the size query is made, then the method that makes the object is named
    for make, entry, scalars, who in ((lambda: c.guided_search(9, 0), "bgs_connect_guided_bytes", [9], "guided_search"),
                                      (lambda: b.guided_moves_search(6, cpuct=4096, max_plies=1), "bgs_bounce_guided_bytes", [6, 208],
                                       "guided_moves_search")):
        with pytest.raises(RuntimeError) as refusal:
            make()
        assert str(refusal.value) == f"{who} needs torch with a GPU"
        name, args = lib.take()
        assert (name, args[1:-1]) == (entry, scalars)
