"""Batched boards on one MI355X: the host-side mirror of the reference's Config/State/Action loop, N boards a call.

The reference loop (README.md:45-72)::

    state = config.sample_initial_state()
    while not state.has_ended:
        action = random.choice(state.actions)
        state = action.sample_next_state()
    reward = state.reward

becomes ``batch = ConnectBatch(6, 7, 4, n); batch.rollout(seed); batch.reward`` -- one HIP launch.  Every method is
a thin call into libbgs.so (include/bgs.h); arrays come back in the reference layout (``grid`` int8[n, H, W], row 0 =
bottom row).  PyTorch, when present with a GPU, only provides the device arena and the stream (plumbing).
"""

from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from .game import _abi

DEFAULT_SEED = 0x0123456789ABCDEF
# bgs_connect_solve_actions: the codes (include/bgs.h) and the default node budget of one (board, column) search
SOLVE_NONE, SOLVE_LOSS, SOLVE_DRAW, SOLVE_WIN, SOLVE_UNKNOWN, SOLVE_BUDGET = -2, -1, 0, 1, 2, 3
DEFAULT_SOLVE_NODES = 1 << 20
# bgs_connect_search_actions: `explore` for a UCB1 constant of about 1.2 on rewards in [0, 1] (45426 * C * C)
DEFAULT_EXPLORE = 65536
# bgs_connect_guided_step: `cpuct` for c_puct = 1.25 (Q8), and the values of leaf_kind
DEFAULT_CPUCT = 320
GUIDED_EVALUATE, GUIDED_TERMINAL, GUIDED_IDLE = _abi.GUIDED_EVALUATE, _abi.GUIDED_TERMINAL, _abi.GUIDED_IDLE
# bgs_bounce_solve_moves: the deepest horizon (BGS_BOUNCE_SOLVE_MAX_DEPTH) and the default one
BOUNCE_SOLVE_MAX_DEPTH = 16
DEFAULT_BOUNCE_SOLVE_DEPTH = 3
# bgs_bounce_evaluate_moves_halving: `best` of a running board whose legal moves need a larger budget (BGS_HALVING_SHORT)
HALVING_SHORT = _abi.HALVING_SHORT


PLAYOUT_POLICIES = {"uniform": _abi.POLICY_UNIFORM, "decisive": _abi.POLICY_DECISIVE}


def playout_policy(name) -> int:
    """the BGS_POLICY_* code of a playout policy's name ("uniform", "decisive"); ValueError for anything else"""
    if not isinstance(name, str) or name not in PLAYOUT_POLICIES:
        raise ValueError(f"unknown playout policy {name!r}: one of {sorted(PLAYOUT_POLICIES)}")
    return PLAYOUT_POLICIES[name]


def _playout_args(seed: int, policy, *int32s) -> list:
    """(seed, *int32s, the code of `policy`): the scalars every entry point that plays playouts begins with.  An unknown
    policy is refused here, before its caller allocates anything or reaches the library."""
    code = playout_policy(policy)
    return [ctypes.c_uint64(seed), *(ctypes.c_int32(x) for x in int32s), code]


def _ptr(a: np.ndarray, ctype):
    return a.ctypes.data_as(ctypes.POINTER(ctype))


def _torch_cuda():
    try:
        import torch
    except ImportError:  # torch is optional: the library then owns its device memory
        return None
    return torch if torch.cuda.is_available() else None


class PinnedArray:
    """A page-locked host array (bgs_host_alloc) viewed as a numpy array: the destination of asynchronous device ->
    host copies.  Keep the object alive while copies into it may be in flight."""

    def __init__(self, shape, dtype):
        self.shape = tuple(int(x) for x in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.dtype = np.dtype(dtype)
        nbytes = max(int(np.prod(self.shape)) * self.dtype.itemsize, 1)
        p = ctypes.c_void_p()
        _abi.check(_abi.lib().bgs_host_alloc(nbytes, ctypes.byref(p)))
        self._ptr = p
        buf = (ctypes.c_uint8 * nbytes).from_address(p.value)
        self.array = np.frombuffer(buf, dtype=self.dtype, count=int(np.prod(self.shape))).reshape(self.shape)

    @property
    def ptr(self) -> int:
        return self._ptr.value

    def close(self) -> None:
        if self._ptr:
            self.array = None
            _abi.lib().bgs_host_free(self._ptr)
            self._ptr = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HostEvent:
    """A device event the asynchronous hand-over records behind its copy (bgs_event)."""

    def __init__(self, device: int = 0):
        self._handle = _abi.c_handle()
        _abi.check(_abi.lib().bgs_event_create(int(device), ctypes.byref(self._handle)))

    def synchronize(self) -> None:
        _abi.check(_abi.lib().bgs_event_synchronize(self._handle))

    def done(self) -> bool:
        flag = ctypes.c_int(0)
        _abi.check(_abi.lib().bgs_event_query(self._handle, ctypes.byref(flag)))
        return bool(flag.value)

    def close(self) -> None:
        if self._handle:
            _abi.lib().bgs_event_destroy(self._handle)
            self._handle = _abi.c_handle()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _host_ptr(dst) -> int:
    """Address of a host destination: PinnedArray, numpy array or (pinned) CPU torch tensor."""
    if isinstance(dst, PinnedArray):
        return dst.ptr
    if isinstance(dst, np.ndarray):
        if not dst.flags.c_contiguous:
            raise TypeError("host destination must be C-contiguous")
        return dst.ctypes.data
    if hasattr(dst, "data_ptr") and not getattr(dst, "is_cuda", False):
        return dst.data_ptr()
    raise TypeError("host destination must be a PinnedArray, a numpy array or a CPU torch tensor")


def expand_outcomes_host(packed, n: int, out=None, first: int = 0, count: Optional[int] = None) -> np.ndarray:
    """Packed 2-bit outcome codes on the HOST (uint8[(n + 3) // 4]) -> reward int8[n, 2] (bgs_expand_outcomes_host)."""
    if out is None:
        out = np.empty((n, 2), dtype=np.int8)
    cnt = n - first if count is None else count
    _abi.check(_abi.lib().bgs_expand_outcomes_host(ctypes.c_void_p(_host_ptr(packed)), first, cnt, ctypes.c_void_p(_host_ptr(out))))
    return out


def _reward_destination(dst, n_games: int, per_game: int = 2) -> int:
    """Address of a host array the library's worker threads will fill with int8[n_games, per_game] LATER (rewards: 2
    bytes per game; grids: height * width): it must be large enough, of 1-byte items and writeable -- the C side cannot
    check any of that from a bare pointer."""
    if per_game != 2:
        return _reward_destination(dst, (n_games * per_game + 1) // 2)
    if isinstance(dst, PinnedArray):
        arr = dst.array
    elif isinstance(dst, np.ndarray):
        arr = dst
    elif hasattr(dst, "data_ptr") and not getattr(dst, "is_cuda", False):
        if dst.element_size() != 1 or dst.numel() < 2 * n_games or not dst.is_contiguous():
            raise TypeError(f"host reward destination must be a contiguous 1-byte-item tensor of at least {2 * n_games} elements")
        return dst.data_ptr()
    else:
        raise TypeError("host reward destination must be a PinnedArray, a numpy array or a CPU torch tensor")
    if arr is None:
        raise ValueError("host reward destination has been closed")
    if arr.dtype.itemsize != 1:
        raise TypeError(f"host reward destination must have 1-byte items (int8), got {arr.dtype}")
    if not arr.flags.c_contiguous:
        raise TypeError("host reward destination must be C-contiguous")
    if not arr.flags.writeable:
        raise ValueError("host reward destination is read-only")
    if arr.nbytes < 2 * n_games:
        raise ValueError(f"host reward destination holds {arr.nbytes} bytes, int8[{n_games}, 2] needs {2 * n_games}")
    return arr.ctypes.data


class RewardSink:
    """Delivers the rewards of successive batch steps into host arrays int8[n, 2] while the GPU goes on playing
    (bgs_sink_*): outcome codes cross PCIe into pinned slots, worker threads expand them on arrival.

    The destination of a submission is written by the library's worker threads after the call has returned: the sink
    checks its size / item size / writeability up front and keeps a reference to it until the submission has been
    waited for (or the sink is closed), so dropping the array early cannot turn into a write to freed memory."""

    def __init__(self, max_games: int, slots: int = 4, threads: int = 4, device: int = 0):
        self._handle = _abi.c_handle()
        self._alive = {}  # ticket -> destination (and anything else that must outlive the delivery)
        self.max_games = int(max_games)
        _abi.check(_abi.lib().bgs_sink_create(int(device), int(max_games), int(slots), int(threads), ctypes.byref(self._handle)))

    def _destination(self, host_reward, n_games: int) -> int:
        return _reward_destination(host_reward, n_games)

    def _keep(self, ticket: int, *objects) -> int:
        if len(self._alive) >= 64:  # (callers that never wait: forget what has been delivered, now and then)
            done = self.completed
            for t in [t for t in self._alive if t < done]:
                del self._alive[t]
        self._alive[ticket] = objects
        return ticket

    def submit(self, batch: "_Batch", host_reward) -> int:
        ticket = ctypes.c_int64(-1)
        ptr = self._destination(host_reward, batch.n)
        try:
            _abi.check(_abi.lib().bgs_sink_submit(self._handle, batch._handle, ctypes.c_void_p(ptr), ctypes.byref(ticket)))
        finally:
            if ticket.value >= 0:  # the ticket exists even when the enqueue failed
                self._keep(ticket.value, host_reward, batch)
        return ticket.value

    def rollout(self, batch: "_Batch", host_reward, seed: int = DEFAULT_SEED, max_plies: int = 2**31 - 1,
                from_initial: bool = False) -> int:
        """`batch.rollout(...)` + `submit(batch, host_reward)` in one library call (bgs_sink_rollout)."""
        flags = _abi.ROLLOUT_FROM_INITIAL if from_initial else 0
        ticket = ctypes.c_int64(-1)
        ptr = self._destination(host_reward, batch.n)
        try:
            _abi.check(
                _abi.lib().bgs_sink_rollout(
                    self._handle, batch._handle, ctypes.c_uint64(seed), ctypes.c_int32(max_plies), ctypes.c_uint32(flags),
                    ctypes.c_void_p(ptr), ctypes.byref(ticket),
                )
            )
        finally:
            if ticket.value >= 0:
                self._keep(ticket.value, host_reward, batch)
        return ticket.value

    def submit_packed(self, device_packed, n_games: int, host_reward, stream: int = 0) -> int:
        """`device_packed`: CUDA uint8 tensor (or device address) of the codes of n_games games, e.g. the RCCL-gathered
        codes of all ranks; copied on HIP stream `stream`."""
        ptr = device_packed.data_ptr() if hasattr(device_packed, "data_ptr") else int(device_packed)
        if hasattr(device_packed, "numel") and device_packed.numel() * device_packed.element_size() < (int(n_games) + 3) // 4:
            raise ValueError("device_packed is smaller than the codes of n_games games")
        ticket = ctypes.c_int64(-1)
        dst = _reward_destination(host_reward, int(n_games))
        try:
            _abi.check(
                _abi.lib().bgs_sink_submit_packed(
                    self._handle, ctypes.c_void_p(stream), ctypes.c_void_p(ptr), int(n_games), ctypes.c_void_p(dst), ctypes.byref(ticket)
                )
            )
        finally:
            if ticket.value >= 0:
                self._keep(ticket.value, host_reward, device_packed)
        return ticket.value

    def wait(self, ticket: int) -> None:
        _abi.check(_abi.lib().bgs_sink_wait(self._handle, int(ticket)))
        self._alive.pop(int(ticket), None)

    @property
    def completed(self) -> int:
        """Number of submissions whose rewards are in their host arrays (they complete in ticket order)."""
        if not self._handle:
            return 0
        v = ctypes.c_int64(0)
        _abi.check(_abi.lib().bgs_sink_completed(self._handle, ctypes.byref(v)))
        return v.value

    def set_progress(self, word_address: Optional[int], keepalive=None) -> None:
        """Announce `completed` in the int64 at `word_address` (host memory, e.g. a SharedRewardRing progress word) after
        every delivery; sleepers use `bgs_progress_wait`.  None stops it."""
        _abi.check(_abi.lib().bgs_sink_set_progress(self._handle, ctypes.c_void_p(word_address) if word_address else None))
        self._progress_keepalive = keepalive

    def close(self) -> None:
        if self._handle:
            _abi.lib().bgs_sink_destroy(self._handle)  # waits for every claimed submission before the workers stop
            self._handle = _abi.c_handle()
        self._alive.clear()
        self._progress_keepalive = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GridSink(RewardSink):
    """Delivers the BOARDS of successive batch steps -- `state.grid` of every game, int8[n, H, W] in the reference layout --
    into host arrays while the GPU goes on playing (bgs_grid_sink_create): the boards cross PCIe bit-packed (16 B per
    6x7 Connect board instead of 42), worker threads expand them.  `submit` / `rollout` / `wait` / `completed` as for a
    RewardSink, with int8[n, H, W] destinations; a `RolloutExecutor` takes one as its sink."""

    def __init__(self, like: "_Batch", slots: int = 4, threads: int = 4):
        self._handle = _abi.c_handle()
        self._alive = {}
        self.max_games = like.n
        self._cells = like.height * like.width
        _abi.check(_abi.lib().bgs_grid_sink_create(like._handle, int(slots), int(threads), ctypes.byref(self._handle)))

    def _destination(self, host_grid, n_games: int) -> int:
        return _reward_destination(host_grid, n_games, self._cells)

    def submit_packed(self, *args, **kwargs):
        raise TypeError("a grid sink takes boards, not outcome codes")


class DeviceView:
    """A batch buffer as a `__cuda_array_interface__` object (version 2; ROCm frameworks use the same protocol): a
    zero-copy hand-over to torch (`torch.as_tensor(view, device="cuda")`), CuPy or Numba without importing any of
    them here.  From a torch tensor, DLPack is one call away (`tensor.__dlpack__()`)."""

    def __init__(self, owner, ptr: int, shape, typestr: str):
        self._owner = owner  # keeps the batch (and its arena) alive
        self.__cuda_array_interface__ = {
            "shape": tuple(int(x) for x in shape),
            "typestr": typestr,
            "data": (int(ptr), False),
            "version": 2,
            "strides": None,
        }


class _Batch:
    """Common part of ConnectBatch / BounceBatch: lifetime, stepping, observation."""

    game = 0

    def __init__(self, n: int, height: int, width: int, device: int, use_torch: Optional[bool]):
        self.n = int(n)
        self.height = int(height)
        self.width = int(width)
        self.device = int(device)
        self._handle = _abi.c_handle()
        self._arena = None
        self._torch = None
        if use_torch is None or use_torch:
            self._torch = _torch_cuda()
            if use_torch and self._torch is None:
                raise RuntimeError("use_torch=True but torch with a visible GPU is not available")

    # ---- lifetime -------------------------------------------------------------------------------
    def _make_arena(self, nbytes: int):
        if self._torch is None:
            return None, 0
        self._arena = self._torch.empty(nbytes, dtype=self._torch.uint8, device=f"cuda:{self.device}")
        return ctypes.c_void_p(self._arena.data_ptr()), nbytes

    def _after_create(self):
        nbytes, generic = ctypes.c_size_t(), ctypes.c_int()
        _abi.check(_abi.lib().bgs_legal_bytes(self._handle, ctypes.byref(nbytes), ctypes.byref(generic)))
        self._legal_bytes = nbytes.value   # bytes per board of bgs_transition's legal-move record
        self.generic = bool(generic.value)  # served by the generic kernels (geometry beyond the bit-packed limits)
        if self._torch is not None:
            self.set_stream(self._torch.cuda.current_stream(self.device).cuda_stream)

    def close(self) -> None:
        if self._handle:
            _abi.lib().bgs_destroy(self._handle)
            self._handle = _abi.c_handle()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, hip_stream: int) -> None:
        _abi.check(_abi.lib().bgs_set_stream(self._handle, ctypes.c_void_p(hip_stream)))

    def set_first_game(self, first_game: int) -> None:
        """Global id of board 0: RNG streams are keyed by global game id, so shards reproduce the unsharded run."""
        _abi.check(_abi.lib().bgs_set_first_game(self._handle, ctypes.c_uint64(first_game)))

    def set_rng_contract(self, contract: str) -> None:
        """Connect: "per-block" (default: a philox word per block of four plies) or "per-ply" (strict: a word per ply, as
        Bounce draws -- one independent uniform choice per ply, what `random.choice` gives a caller of the reference,
        README.md:62).  Applies to every later random step / rollout of this batch (bgs_set_rng_contract)."""
        codes = {"per-block": _abi.RNG_PER_BLOCK, "per-ply": _abi.RNG_PER_PLY}
        if contract not in codes:
            raise ValueError(f"unknown RNG contract {contract!r}: 'per-block' or 'per-ply'")
        _abi.check(_abi.lib().bgs_set_rng_contract(self._handle, codes[contract]))

    def set_launches_in_flight(self, launches: int) -> None:
        """A hint: how many rollout launches the caller keeps in flight on the device (1, the default: one at a time).
        Results never depend on it; the Bounce rollout shapes its launch by it (bgs_set_launches_in_flight).  The
        rollout executor and `RolloutPipeline` pass their depth."""
        _abi.check(_abi.lib().bgs_set_launches_in_flight(self._handle, int(launches)))

    def synchronize(self) -> None:
        _abi.check(_abi.lib().bgs_synchronize(self._handle))

    # ---- the hot path ---------------------------------------------------------------------------
    def reset(self) -> None:
        _abi.check(_abi.lib().bgs_reset(self._handle))

    def step_random(self, seed: int = DEFAULT_SEED, plies: int = 1) -> None:
        """`plies` uniformly sampled plies on every running board (one launch where the kernel can keep the boards
        in registers in between)."""
        _abi.check(_abi.lib().bgs_step_random_n(self._handle, ctypes.c_uint64(seed), ctypes.c_int32(plies)))

    def rollout(self, seed: int = DEFAULT_SEED, max_plies: int = 2**31 - 1, from_initial: bool = False) -> None:
        flags = _abi.ROLLOUT_FROM_INITIAL if from_initial else 0
        _abi.check(_abi.lib().bgs_rollout(self._handle, ctypes.c_uint64(seed), ctypes.c_int32(max_plies), ctypes.c_uint32(flags)))

    def _step_actions(self, actions, per_board: int, want_status: bool):
        status = np.zeros(self.n, dtype=np.int32) if want_status else None
        sp = _ptr(status, ctypes.c_int32) if want_status else None
        if self._torch is not None and isinstance(actions, self._torch.Tensor):
            t = actions
            if not (t.is_cuda and t.dtype == self._torch.int32 and t.is_contiguous() and t.numel() == self.n * per_board):
                raise TypeError("device actions must be a contiguous int32 CUDA tensor of the batch's shape")
            _abi.check(_abi.lib().bgs_step_actions(self._handle, ctypes.c_void_p(t.data_ptr()), 1, sp))
        else:
            a = np.ascontiguousarray(actions, dtype=np.int32)
            if a.size != self.n * per_board:
                raise TypeError(f"expected {self.n * per_board} action entries, got {a.size}")
            _abi.check(_abi.lib().bgs_step_actions(self._handle, ctypes.c_void_p(a.ctypes.data), 0, sp))
        return status

    @property
    def steps(self) -> int:
        """env-steps applied since the last reset (transitions on running boards)."""
        v = ctypes.c_uint64(0)
        _abi.check(_abi.lib().bgs_steps(self._handle, ctypes.byref(v)))
        return v.value

    def reset_steps(self) -> None:
        _abi.check(_abi.lib().bgs_reset_steps(self._handle))

    # ---- observation (reference layout, host copies) ------------------------------------------------
    @property
    def grid(self) -> np.ndarray:
        out = np.empty((self.n, self.height, self.width), dtype=np.int8)
        _abi.check(_abi.lib().bgs_read_grid(self._handle, _ptr(out, ctypes.c_int8)))
        return out

    @property
    def player(self) -> np.ndarray:
        out = np.empty(self.n, dtype=np.int8)
        _abi.check(_abi.lib().bgs_read_player(self._handle, _ptr(out, ctypes.c_int8)))
        return out

    @property
    def has_ended(self) -> np.ndarray:
        out = np.empty(self.n, dtype=np.uint8)
        _abi.check(_abi.lib().bgs_read_ended(self._handle, _ptr(out, ctypes.c_uint8)))
        return out.astype(bool)

    @property
    def winner(self) -> np.ndarray:
        out = np.empty(self.n, dtype=np.int8)
        _abi.check(_abi.lib().bgs_read_winner(self._handle, _ptr(out, ctypes.c_int8)))
        return out

    @property
    def reward(self) -> np.ndarray:
        out = np.empty((self.n, 2), dtype=np.int8)
        _abi.check(_abi.lib().bgs_read_reward(self._handle, _ptr(out, ctypes.c_int8)))
        return out

    # ---- asynchronous hand-over to host memory (the batch form of State.reward, connect.cpp:41) ----------------
    def read_reward_async(self, host_dst, event: Optional[HostEvent] = None) -> None:
        """Enqueue reward int8[n, 2] -> `host_dst` (page-locked) on the batch's stream; `event` fires behind the copy."""
        _abi.check(_abi.lib().bgs_read_reward_async(self._handle, ctypes.c_void_p(_host_ptr(host_dst)), event._handle if event else None))

    def read_outcomes_async(self, host_dst, event: Optional[HostEvent] = None) -> None:
        """Enqueue the 2-bit outcome codes uint8[(n + 3) // 4] -> `host_dst` (page-locked); expand with
        `expand_outcomes_host`."""
        _abi.check(_abi.lib().bgs_read_outcomes_async(self._handle, ctypes.c_void_p(_host_ptr(host_dst)), event._handle if event else None))

    def rollout_to_host(self, host_dst, seed: int = DEFAULT_SEED, max_plies: int = 2**31 - 1, from_initial: bool = False,
                        codes: bool = False, event: Optional[HostEvent] = None) -> None:
        """`rollout` + `read_reward_async` (or `read_outcomes_async` with codes=True) in one library call."""
        flags = _abi.ROLLOUT_FROM_INITIAL if from_initial else 0
        _abi.check(
            _abi.lib().bgs_rollout_to_host(
                self._handle, ctypes.c_uint64(seed), ctypes.c_int32(max_plies), ctypes.c_uint32(flags),
                ctypes.c_void_p(_host_ptr(host_dst)), 1 if codes else 0, event._handle if event else None,
            )
        )

    @property
    def plies(self) -> np.ndarray:
        out = np.empty(self.n, dtype=np.int32)
        _abi.check(_abi.lib().bgs_read_plies(self._handle, _ptr(out, ctypes.c_int32)))
        return out

    @property
    def action_count(self) -> np.ndarray:
        out = np.empty(self.n, dtype=np.int32)
        _abi.check(_abi.lib().bgs_read_action_count(self._handle, _ptr(out, ctypes.c_int32)))
        return out

    def write_state(self, grid, player=None, winner=None, plies=None) -> np.ndarray:
        """Load boards in the reference layout; returns per-board status (0 ok, -1 malformed and left untouched)."""
        g = np.ascontiguousarray(grid, dtype=np.int8)
        if g.shape != (self.n, self.height, self.width):
            raise TypeError(f"grid must have shape {(self.n, self.height, self.width)}, got {g.shape}")
        p = None if player is None else np.ascontiguousarray(player, dtype=np.int8)
        w = None if winner is None else np.ascontiguousarray(winner, dtype=np.int8)
        l = None if plies is None else np.ascontiguousarray(plies, dtype=np.int32)
        status = np.zeros(self.n, dtype=np.int32)
        _abi.check(
            _abi.lib().bgs_write_state(
                self._handle,
                _ptr(g, ctypes.c_int8),
                None if p is None else _ptr(p, ctypes.c_int8),
                None if w is None else _ptr(w, ctypes.c_int8),
                None if l is None else _ptr(l, ctypes.c_int32),
                _ptr(status, ctypes.c_int32),
            )
        )
        return status

    def transition(self, grid=None, player=None, winner=None, plies=None, actions=None):
        """One round trip for the object API: optionally load boards, optionally apply one chosen move per board, then
        observe.  Returns (status int32[n], grid, player, winner, plies, legal, reward) with `legal` the Connect mask
        uint8[n, W] or the Bounce target masks uint64[n, W + 1] and `reward` int8[n, 2] as the device holds it."""
        n = self.n
        i8 = ctypes.c_int8
        g = p = w = l = a = None
        if grid is not None:
            g = np.ascontiguousarray(grid, dtype=np.int8)
            if g.shape != (n, self.height, self.width):
                raise TypeError(f"grid must have shape {(n, self.height, self.width)}, got {g.shape}")
            p = np.ascontiguousarray(player, dtype=np.int8)
            w = np.ascontiguousarray(winner, dtype=np.int8)
            l = None if plies is None else np.ascontiguousarray(plies, dtype=np.int32)
        if actions is not None:
            a = np.ascontiguousarray(actions, dtype=np.int32)
            if a.size != n * self._action_width:
                raise TypeError(f"expected {n * self._action_width} action entries, got {a.size}")
        status = np.zeros(n, dtype=np.int32)
        grid_out = np.empty((n, self.height, self.width), dtype=np.int8)
        player_out = np.empty(n, dtype=np.int8)
        winner_out = np.empty(n, dtype=np.int8)
        plies_out = np.empty(n, dtype=np.int32)
        legal_out = self._empty_legal()
        reward_out = np.empty((n, 2), dtype=np.int8)
        _abi.check(
            _abi.lib().bgs_transition(
                self._handle,
                None if g is None else _ptr(g, i8),
                None if p is None else _ptr(p, i8),
                None if w is None else _ptr(w, i8),
                None if l is None else _ptr(l, ctypes.c_int32),
                None if a is None else _ptr(a, ctypes.c_int32),
                _ptr(status, ctypes.c_int32),
                _ptr(grid_out, i8),
                _ptr(player_out, i8),
                _ptr(winner_out, i8),
                _ptr(plies_out, ctypes.c_int32),
                ctypes.c_void_p(legal_out.ctypes.data),
                _ptr(reward_out, i8),
            )
        )
        return status, grid_out, player_out, winner_out, plies_out, legal_out, reward_out

    def one_board_call(self) -> "OneBoardCall":
        return OneBoardCall(self)

    # ---- device-side hand-over (torch / RCCL plumbing) -----------------------------------------------
    def buffer(self, buffer_id: int):
        """(device pointer, bytes) of one of the batch's buffers (see bgs_buffer_id in include/bgs.h)."""
        p = ctypes.c_void_p()
        sz = ctypes.c_size_t()
        _abi.check(_abi.lib().bgs_buffer(self._handle, buffer_id, ctypes.byref(p), ctypes.byref(sz)))
        return p.value, sz.value

    def device_view(self, what: str = "reward") -> DeviceView:
        """`__cuda_array_interface__` view of a batch buffer without torch: "reward" int8[n, 2], "status" uint8[n],
        "planes" uint64[planes, n]."""
        if what == "reward":
            ptr, _ = self.buffer(_abi.BUF_REWARD)
            return DeviceView(self, ptr, (self.n, 2), "|i1")
        if what == "status":
            ptr, _ = self.buffer(_abi.BUF_STATUS)
            return DeviceView(self, ptr, (self.n,), "|u1")
        if what == "planes":
            ptr, nbytes = self.buffer(_abi.BUF_PLANES)
            return DeviceView(self, ptr, (nbytes // (8 * self.n), self.n), "<u8")
        raise ValueError(f"unknown device view {what!r}")

    def _arena_view(self, buffer_id: int):
        if self._arena is None:
            raise RuntimeError("device views need the torch-owned arena (construct the batch with torch + GPU available)")
        ptr, nbytes = self.buffer(buffer_id)
        off = ptr - self._arena.data_ptr()
        return self._arena[off : off + nbytes]

    def reward_tensor(self):
        """Zero-copy torch view int8[n, 2] of the device reward buffer (what the RCCL gather ships)."""
        return self._arena_view(_abi.BUF_REWARD).view(self._torch.int8).view(self.n, 2)

    def status_tensor(self):
        return self._arena_view(_abi.BUF_STATUS)

    def steps_tensor(self):
        """Device view of the sharded env-step counter (int64 words; their SUM is the count)."""
        return self._arena_view(_abi.BUF_STEPS).view(self._torch.int64)

    def outcomes_tensor(self, out=None):
        """uint8[(n + 3) // 4] on the device: 2-bit outcome codes (0 running, 1 / 2 winner, 3 draw), 4 boards per
        byte -- the compact form of the rewards that ranks exchange (see simulator.sharding)."""
        t = self._torch
        if t is None:
            raise RuntimeError("outcomes_tensor needs torch with a GPU")
        if out is None:
            out = t.empty((self.n + 3) // 4, dtype=t.uint8, device=f"cuda:{self.device}")
        _abi.check(_abi.lib().bgs_pack_outcomes(self._handle, ctypes.c_void_p(out.data_ptr())))
        return out

    def rollout_outcomes_tensor(self, out, seed: int = DEFAULT_SEED, max_plies: int = 2**31 - 1, from_initial: bool = False):
        """`rollout` + `outcomes_tensor(out)` in one library call (bgs_rollout_pack): the rollout kernel writes the codes
        itself where it can.  `out`: CUDA uint8 tensor of ((n + 63) // 64) * 16 bytes."""
        if out.numel() < (self.n + 63) // 64 * 16 or not out.is_cuda or not out.is_contiguous():
            raise TypeError("outcome buffer must be a contiguous CUDA uint8 tensor of ((n + 63) // 64) * 16 bytes")
        flags = _abi.ROLLOUT_FROM_INITIAL if from_initial else 0
        _abi.check(_abi.lib().bgs_rollout_pack(self._handle, ctypes.c_uint64(seed), ctypes.c_int32(max_plies),
                                               ctypes.c_uint32(flags), ctypes.c_void_p(out.data_ptr())))
        return out

    def grid_tensor(self, out=None):
        """Observation tensor int8[n, H, W] on the device (no host round trip), e.g. as policy-network input."""
        t = self._torch
        if t is None:
            raise RuntimeError("grid_tensor needs torch with a GPU")
        if out is None:
            out = t.empty((self.n, self.height, self.width), dtype=t.int8, device=f"cuda:{self.device}")
        _abi.check(_abi.lib().bgs_export_device(self._handle, ord("g"), ctypes.c_void_p(out.data_ptr())))
        return out


    def _export(self, what: str, out):
        _abi.check(_abi.lib().bgs_export_device(self._handle, ord(what), ctypes.c_void_p(out.data_ptr())))
        return out

    def action_count_tensor(self, out=None):
        """int32[n] on the device: len(state.actions) per board (0 once ended)."""
        t = self._need_torch("action_count_tensor")
        if out is None:
            out = t.empty(self.n, dtype=t.int32, device=f"cuda:{self.device}")
        return self._export("c", out)

    def reward_copy_tensor(self, out=None):
        """int8[n, 2] on the device: a copy of the reward buffer (bgs_export_device 'r')."""
        t = self._need_torch("reward_copy_tensor")
        if out is None:
            out = t.empty((self.n, 2), dtype=t.int8, device=f"cuda:{self.device}")
        return self._export("r", out)

    def env_step(self, actions, observation=None, ended=None, reward=None, status=None, auto_reset: bool = True):
        """The step of a vector environment (bgs_env_step): `step_actions_observe` plus `reward` int8[n, 2] -- the finished
        game's pair where `ended` is set, 0 / 0 while a game runs -- and, with auto_reset, boards that have ended put back to
        the initial state in the same call, so that the returned observation is already the new game's.  All device tensors,
        no synchronisation.  Returns the observation tensor."""
        return self._observe(actions, observation, ended, reward, status, _abi.ENV_AUTO_RESET if auto_reset else 0)

    def step_actions_observe(self, actions, observation=None, ended=None, status=None):
        """ONE library call per policy ply (bgs_step_actions_observe): apply `actions` -- a DEVICE tensor, int32[n] columns for
        Connect, int32[n, 4] moves for Bounce; negative = skip the board -- and write the observation of the boards after the
        move for the policy's next choice: Connect the legal mask uint8[n, width], Bounce the target masks int64[n, width + 1]
        (`observation`, allocated when None), plus `ended` uint8[n] and `status` int32[n] (per-board result) when given.
        Everything stays on the device and on the batch's stream: no synchronisation, capturable in a HIP graph.  Returns the
        observation tensor.  The loop: obs = batch.legal_tensor(); while ...: obs = batch.step_actions_observe(policy(obs), obs)."""
        return self._observe(actions, observation, ended, None, status, 0)

    def _observe(self, actions, observation, ended, reward, status, flags: int):
        t = self._need_torch("step_actions_observe")
        width = 1 if self.game == _abi.GAME_CONNECT else 4
        want = (self.n,) if width == 1 else (self.n, 4)
        if not (hasattr(actions, "data_ptr") and actions.is_cuda and actions.dtype == t.int32 and tuple(actions.shape) == want
                and actions.is_contiguous()):
            raise TypeError(f"actions must be a contiguous int32 device tensor of shape {want}")
        if observation is None:
            observation = (t.empty((self.n, self.width), dtype=t.uint8, device=actions.device) if width == 1
                           else t.empty((self.n, self.width + 1), dtype=t.int64, device=actions.device))
        shape = (self.n, self.width) if width == 1 else (self.n, self.width + 1)
        dtypes = (t.uint8,) if width == 1 else (t.int64, getattr(t, "uint64", t.int64))   # (64-bit masks: either signedness)
        if not (observation.is_cuda and observation.dtype in dtypes and tuple(observation.shape) == shape and observation.is_contiguous()):
            raise TypeError(f"observation must be a contiguous {dtypes[0]} device tensor of shape {shape}")
        for name, buf, dt in (("ended", ended, t.uint8), ("status", status, t.int32)):
            if buf is not None and not (buf.is_cuda and buf.dtype == dt and tuple(buf.shape) == (self.n,) and buf.is_contiguous()):
                raise TypeError(f"{name} must be a contiguous {dt} device tensor of shape ({self.n},)")
        if reward is not None and not (reward.is_cuda and reward.dtype == t.int8 and tuple(reward.shape) == (self.n, 2) and reward.is_contiguous()):
            raise TypeError(f"reward must be a contiguous int8 device tensor of shape ({self.n}, 2)")
        _abi.check(_abi.lib().bgs_env_step(
            self._handle, ctypes.c_void_p(actions.data_ptr()), ctypes.c_void_p(observation.data_ptr()),
            ctypes.c_void_p(ended.data_ptr()) if ended is not None else None,
            ctypes.c_void_p(reward.data_ptr()) if reward is not None else None,
            ctypes.c_void_p(status.data_ptr()) if status is not None else None, ctypes.c_uint32(flags)))
        return observation

    def _need_torch(self, who: str):
        if self._torch is None:
            raise RuntimeError(f"{who} needs torch with a GPU")
        return self._torch

    def _device_tensors(self, who: str, specs, align: int = 16):
        """The device tensors of a `*_tensor` call, in order: specs are (name, tensor or None, shape[, dtype name[,
        optional]]), the dtype "int32" and not optional unless given.  A tensor that is None is allocated unless it is
        optional; one that is there must be a contiguous device tensor of that dtype and shape whose address is a
        multiple of `align`, else TypeError names the argument."""
        t = self._need_torch(who)
        rule = f", {align}-byte aligned" if align > 1 else ""
        tensors = []
        for name, x, shape, *rest in specs:
            dtype, optional = rest + ["int32", False][len(rest):]
            if x is None and not optional:
                x = t.empty(shape, dtype=getattr(t, dtype), device=f"cuda:{self.device}")
            if x is not None and not (x.is_cuda and x.dtype == getattr(t, dtype) and tuple(x.shape) == shape and x.is_contiguous()
                                      and x.data_ptr() % align == 0):
                raise TypeError(f"{name} must be a contiguous{rule} {dtype} device tensor of shape {shape}")
            tensors.append(x)
        return tensors

    def _search_workspace(self, who: str, workspace, size_query, cache_key):
        """The workspace of a `search_*_tensor` call: the caller's, or when None the batch's own for cache_key(),
        allocated on first use.  size_query() runs on every call without a workspace, before the key is made: it refuses
        bad arguments (ValueError) before anything is allocated for them."""
        t = self._need_torch(who)
        if workspace is None:
            need, key = size_query(), cache_key()
            workspace = self._search_workspaces.get(key)
            if workspace is None:
                workspace = self._search_workspaces[key] = t.empty(need, dtype=t.uint8, device=f"cuda:{self.device}")
        if not (workspace.is_cuda and workspace.dtype == t.uint8 and workspace.is_contiguous()):
            raise TypeError("workspace must be a contiguous uint8 device tensor")
        return workspace

    def _size_query(self, entry: str, *sizes) -> int:
        """what the `*_bytes` entry point `entry` answers for the int32 `sizes`"""
        nbytes = ctypes.c_size_t()
        _abi.check(getattr(_abi.lib(), entry)(self._handle, *(ctypes.c_int32(x) for x in sizes), ctypes.byref(nbytes)))
        return nbytes.value

    def _analysis(self, who: str, entry: str, scalars, specs, tensors=None, workspace=None, sizing=None):
        """The one body of every analysis call, host and tensor form: `entry`(handle, *scalars, the outputs[, a workspace
        and its bytes], on_device), once; returns the outputs in the order of `specs`.  specs are (name, shape[, dtype
        name[, optional]]) in ABI order, what `_device_tensors` takes less the tensor: the one place where a call's output
        shapes and dtypes are written.  tensors None is the host form, numpy arrays made here; else they are the caller's
        device tensors in that order (None: allocated), checked by `_device_tensors` under the name `who`.  An optional
        output that is not there goes to the library as NULL.  sizing is the (size_query, cache_key) of a search
        (`_search_workspace`): its tensor form takes `workspace` or the batch's cached one, its host form passes None, 0
        and the library allocates.  A `workspace` without sizing (a forest's buffer) is passed as it is."""
        if tensors is None:
            outs = []
            for _, shape, *rest in specs:
                dtype, optional = rest + ["int32", False][len(rest):]
                outs.append(None if optional else np.empty(shape, dtype=dtype))
            pointers = [None if x is None else ctypes.c_void_p(x.ctypes.data) for x in outs]
        else:
            outs = self._device_tensors(who, [(name, x, *rest) for (name, *rest), x in zip(specs, tensors)])
            pointers = [None if x is None else ctypes.c_void_p(x.data_ptr()) for x in outs]
            if sizing is not None:
                workspace = self._search_workspace(who, workspace, *sizing)
        if workspace is not None:
            pointers += [ctypes.c_void_p(workspace.data_ptr()), ctypes.c_size_t(workspace.numel())]
        elif sizing is not None:
            pointers += [None, 0]
        _abi.check(getattr(_abi.lib(), entry)(self._handle, *scalars, *pointers, 0 if tensors is None else 1))
        return tuple(outs)

    def _search_specs(self, proving: bool = False, carried: bool = False):
        """the outputs of a tree search of this batch, a proving one or a forest's, as `_analysis` takes them"""
        n, row = (self.n,), self._per_action()
        specs = [("counts", row + (3,)), ("visits", row)] + [(name, n) for name in self._search_counters]
        if proving:
            specs += [("proved", row, "int8"), ("done", n)]
        if carried:
            specs += [("carried", n)]
        return specs

    def _evaluate(self, who: str, entry: str, tensors, seed: int, playouts: int, max_plies: int, policy: str):
        """the flat evaluation of `policy`, host or tensor form: "uniform" is `entry` itself (bgs_connect_evaluate_actions,
        bgs_bounce_evaluate_moves), any other policy goes through `entry`_policy, which takes the policy's code as well"""
        scalars = _playout_args(seed, policy, playouts, max_plies)
        if scalars[-1] == _abi.POLICY_UNIFORM:
            scalars.pop()
        else:
            entry += "_policy"
        return self._analysis(who, entry, scalars, [("out", self._per_action() + (3,))], tensors)[0]

    def _halving(self, who: str, entry: str, tensors, seed: int, budget: int, max_plies: int, policy: str):
        """the sequential-halving evaluation, host or tensor form"""
        row = self._per_action()
        return self._analysis(who, entry, _playout_args(seed, policy, budget, max_plies),
                              [("counts", row + (3,)), ("given", row), ("best", (self.n,))], tensors)

    def _solve(self, who: str, entry: str, tensors, depth: int, max_nodes: int, with_plies: bool):
        """the exact solve, host or tensor form: (codes, plies or None).  The node counter, the third output of the entry
        point, is never asked for: it goes as NULL"""
        row = self._per_action()
        specs = [("codes", row, "int8"), ("plies", row, "int16", not with_plies), ("nodes", (1,), "uint64", True)]
        return self._analysis(who, entry, [ctypes.c_int32(int(depth)), ctypes.c_int64(max_nodes)], specs,
                              None if tensors is None else tensors + (None,))[:2]

    # ---- snapshot / restore in the reference's wire format (State.to_json / State.from_json) -------------------
    def to_json_states(self) -> list:
        """The batch as a list of reference-shaped State JSON dicts {"grid", "player", "winner"}
        (tests/test_connect.py:131-138, tests/test_bounce.py:392-403)."""
        grid, player, winner = self.grid, self.player, self.winner
        return [{"grid": grid[i].tolist(), "player": int(player[i]), "winner": int(winner[i])} for i in range(self.n)]

    def from_json_states(self, states) -> np.ndarray:
        """Load a list of n State JSON dicts; returns per-board status (0 ok, -1 malformed and left untouched)."""
        if len(states) != self.n:
            raise TypeError(f"expected {self.n} states, got {len(states)}")
        try:
            grid = np.array([s["grid"] for s in states], dtype=np.int8)
            player = np.array([s["player"] for s in states], dtype=np.int8)
            winner = np.array([s["winner"] for s in states], dtype=np.int8)
        except (KeyError, TypeError, ValueError) as exc:
            raise RuntimeError(f"invalid state JSON: {exc}") from None
        return self.write_state(grid, player, winner)


def expand_outcomes(packed, n: int, out=None):
    """Packed 2-bit outcome codes (CUDA uint8 tensor) of n boards -> reward int8[n, 2] on the same device."""
    import torch

    if not packed.is_cuda or packed.dtype != torch.uint8 or not packed.is_contiguous() or packed.numel() < (n + 3) // 4:
        raise TypeError("packed outcomes must be a contiguous CUDA uint8 tensor of (n + 3) // 4 bytes")
    if out is None:
        out = torch.empty((n, 2), dtype=torch.int8, device=packed.device)
    stream = torch.cuda.current_stream(packed.device).cuda_stream
    _abi.check(
        _abi.lib().bgs_expand_outcomes(
            packed.device.index, ctypes.c_void_p(stream), ctypes.c_void_p(packed.data_ptr()), n, ctypes.c_void_p(out.data_ptr())
        )
    )
    return out


class OneBoardCall:
    """`bgs_transition` on a one-board batch with everything that does not change between calls made once: the input
    and output arrays, their ctypes pointers and the bound function.  The object API makes one such call per State;
    building seven arrays and thirteen pointer objects per call cost as much as the device round trip."""

    def __init__(self, batch: "GameBatch"):
        if batch.n != 1:
            raise ValueError("OneBoardCall serves one-board batches")
        self.batch = batch
        h, w = batch.height, batch.width
        self.grid_in = np.empty((h, w), dtype=np.int8)
        self.player_in = np.zeros(1, dtype=np.int8)
        self.winner_in = np.zeros(1, dtype=np.int8)
        self.plies_in = np.zeros(1, dtype=np.int32)
        self.action_in = np.zeros(batch._action_width, dtype=np.int32)
        self.status = np.zeros(1, dtype=np.int32)
        self.grid_out = np.empty((h, w), dtype=np.int8)
        self.player_out = np.empty(1, dtype=np.int8)
        self.winner_out = np.empty(1, dtype=np.int8)
        self.plies_out = np.empty(1, dtype=np.int32)
        self.legal_out = batch._empty_legal()
        self.reward_out = np.empty(2, dtype=np.int8)
        i8, i32 = ctypes.c_int8, ctypes.c_int32
        self._load = (_ptr(self.grid_in, i8), _ptr(self.player_in, i8), _ptr(self.winner_in, i8))
        self._plies = _ptr(self.plies_in, i32)
        self._action = _ptr(self.action_in, i32)
        self._out = (
            _ptr(self.status, i32), _ptr(self.grid_out, i8), _ptr(self.player_out, i8), _ptr(self.winner_out, i8),
            _ptr(self.plies_out, i32), ctypes.c_void_p(self.legal_out.ctypes.data), _ptr(self.reward_out, i8),
        )
        self._fn = _abi.lib().bgs_transition
        self._none3 = (None, None, None)

    def __call__(self, grid=None, player: int = 0, winner: int = -1, plies=None, action=None) -> int:
        """Optional load (grid int8[h, w] + player + winner [+ plies]), optional move (an int or a sequence of
        `_action_width` ints), then observe into the `*_out` arrays.  Returns the board's status (0, or a BGS_ERR_*)."""
        load = self._none3
        if grid is not None:
            self.grid_in[...] = grid
            self.player_in[0] = player
            self.winner_in[0] = winner
            load = self._load
            if plies is not None:
                self.plies_in[0] = plies
        if action is not None:
            self.action_in[...] = action
        rc = self._fn(
            self.batch._handle, *load, None if grid is None or plies is None else self._plies,
            None if action is None else self._action, *self._out,
        )
        if rc:
            _abi.check(rc)
        return int(self.status[0])


class _Forest:
    """What SearchForest and MovesForest share: the device buffer, the first-search rule and one body a call.  The
    per-game part: `_search_entry` and `_advance_entry`, `_maker` (the batch's method that makes the forest, for the
    missing-torch message), `_moves` (the name of the `advance` input) and `_sizes()`, the size arguments of both entry
    points; the outputs are the batch's `_search_specs(carried=True)`."""

    def _open(self, nbytes: int) -> None:
        t = self.batch._need_torch(self._maker)
        self._buffer = t.zeros(nbytes, dtype=t.uint8, device=f"cuda:{self.batch.device}")   # (zeros: every tree empty)
        self._fresh = True

    def close(self) -> None:
        self._buffer = None

    def _search(self, tensors, seed, iterations, leaf_playouts, explore, max_plies, policy, restart):
        if self._buffer is None:
            raise RuntimeError("the forest is closed")
        scalars = _playout_args(seed, policy, iterations, leaf_playouts, explore, max_plies)
        scalars += [*(ctypes.c_int32(x) for x in self._sizes()), 1 if restart or self._fresh else 0]
        outs = self.batch._analysis("search_tensor", self._search_entry, scalars, self.batch._search_specs(carried=True), tensors,
                                    self._buffer)
        self._fresh = False
        return outs

    def _advance(self, moves, kept=None, on_device: bool = False):
        n = self.batch.n
        if on_device:   # (moves is an input: "optional", so that it is checked and never allocated)
            moves, kept = self.batch._device_tensors("advance_tensor", [(self._moves, moves, (n,), "int32", True), ("kept", kept, (n,))],
                                                     align=1)
            pointers = moves.data_ptr(), kept.data_ptr()
        else:
            moves = np.ascontiguousarray(moves, dtype=np.int32)
            if moves.shape != (n,):
                raise TypeError(f"{self._moves} must be int32[{n}]")
            kept = np.empty(n, dtype=np.int32)
            pointers = moves.ctypes.data, kept.ctypes.data
        if self._buffer is None:
            raise RuntimeError("the forest is closed")
        _abi.check(getattr(_abi.lib(), self._advance_entry)(
            self.batch._handle, ctypes.c_void_p(pointers[0]), *(ctypes.c_int32(x) for x in self._sizes()), ctypes.c_void_p(pointers[1]),
            ctypes.c_void_p(self._buffer.data_ptr()), ctypes.c_size_t(self._buffer.numel()), 1 if on_device else 0))
        return kept


class _Guided:
    """What GuidedSearch and GuidedMovesSearch share: the trees' buffer, the output tensors made once, the "begin() comes
    first" rule and one body a call.  The per-game part: `_entry`, `_maker` (the batch's method that makes the object, for
    the messages about tensors), `_scalars()` (the int32 arguments in front of `flags`: the size arguments, `cpuct` and,
    for Bounce, `max_plies`), `_priors` (the shape of `priors` as the TypeError names it; the shape itself is an entry a
    column or move slot of every board), `_leaves` (the indices of the outputs `run` passes to `evaluate`) and the output
    specs, which the constructor hands to `_open` once it has checked its ranges."""

    def _check_cpuct(self, given) -> None:
        if not 0 <= self.cpuct <= 4096:
            raise ValueError(f"cpuct must be 0 .. 4096, c_puct in Q8 (got {given})")

    def _open(self, nbytes: int, specs) -> None:
        batch = self.batch
        t = batch._need_torch(self._maker)
        self._buffer = t.zeros(nbytes, dtype=t.uint8, device=f"cuda:{batch.device}")
        self._outputs = tuple(batch._device_tensors(self._maker, [(name, None, *rest) for name, *rest in specs]))
        self._fresh = True

    def close(self) -> None:
        self._buffer = None

    def _call(self, flags: int, priors, values):
        if self._buffer is None:
            raise RuntimeError("the guided search is closed")
        if self._fresh and not flags & _abi.GUIDED_RESTART:
            raise RuntimeError("begin() comes first: fresh memory holds no trees")
        pointers = [None, None]
        if not flags & _abi.GUIDED_RESTART:   # (inputs: "optional", so that they are checked and never allocated)
            priors, values = self.batch._device_tensors(self._maker, [("priors", priors, self.batch._per_action(), "float32", True),
                                                                      ("values", values, (self.batch.n,), "float32", True)])
            if priors is None or values is None:
                raise TypeError(f"priors and values are the evaluator's device tensors: {self._priors} and float32[n]")
            pointers = [ctypes.c_void_p(priors.data_ptr()), ctypes.c_void_p(values.data_ptr())]
        _abi.check(getattr(_abi.lib(), self._entry)(
            self.batch._handle, *(ctypes.c_int32(x) for x in self._scalars()), ctypes.c_uint32(flags), *pointers,
            *(ctypes.c_void_p(x.data_ptr()) for x in self._outputs), ctypes.c_void_p(self._buffer.data_ptr()),
            ctypes.c_size_t(self._buffer.numel())))
        self._fresh = False
        return self._outputs

    def begin(self):
        """Empty every tree (BGS_GUIDED_RESTART): the leaves that come back are the roots."""
        return self._call(_abi.GUIDED_RESTART, None, None)

    def step(self, priors, values):
        """One simulation: apply (priors, values) to the leaves of the previous call, descend to the next leaves."""
        return self._call(0, priors, values)

    def _run(self, evaluate, simulations: int):
        if simulations < 1:
            raise ValueError(f"simulations must be >= 1 (got {simulations})")
        outs = self.begin()
        for _ in range(int(simulations) - 1):
            outs = self.step(*evaluate(*(outs[i] for i in self._leaves)))
        return self.finish(*evaluate(*(outs[i] for i in self._leaves)))


class ConnectBatch(_Batch):
    """N Connect-k boards: ``Config(height, width, count)`` (reference connect.cpp:26) times n."""

    game = _abi.GAME_CONNECT
    _action_width = 1
    _search_counters = ("best", "nodes")   # the int32[n] outputs of a tree search

    def _per_action(self):
        """the shape of an entry a column of every board"""
        return (self.n, self.width)

    def _empty_legal(self):
        return np.empty((self.n, self.width), dtype=np.uint8)

    def __init__(self, height: int, width: int, count: int, n: int, device: int = 0, use_torch: Optional[bool] = None):
        super().__init__(n, height, width, device, use_torch)
        self.count = int(count)
        self._search_workspaces = {}   # iterations -> the uint8 device tensor search_actions_tensor allocated
        nbytes = ctypes.c_size_t()
        _abi.check(_abi.lib().bgs_connect_arena_bytes(self.height, self.width, self.count, self.n, ctypes.byref(nbytes)))
        arena, arena_bytes = self._make_arena(nbytes.value)
        _abi.check(
            _abi.lib().bgs_connect_create(
                self.height, self.width, self.count, self.n, self.device, arena, arena_bytes, ctypes.byref(self._handle)
            )
        )
        self._after_create()

    def step_actions(self, columns, want_status: bool = True):
        """columns int32[n]; a negative entry skips the board.  Returns per-board status (0 / -2 illegal)."""
        return self._step_actions(columns, 1, want_status)

    def evaluate_actions(self, seed: int = DEFAULT_SEED, playouts: int = 256, max_plies: int = 2**31 - 1,
                         policy: str = "uniform") -> np.ndarray:
        """Flat Monte-Carlo evaluation of every column of every board (bgs_connect_evaluate_actions), one launch:
        int32[n, width, 3] = (wins, draws, losses) of the player to move, over `playouts` games that start with that
        column and continue by the uniform random policy until they end or hold `max_plies` plies (a capped game counts in
        none of the three).  Illegal columns and ended boards give 0, 0, 0.  The boards are not modified.  Playout p of
        column c of board i is game ((first_game + i) * width + c) * playouts + p of the batch's RNG contract.
        policy="decisive" (bgs_connect_evaluate_actions_policy): the same games and draws, but a ply takes a winning
        column when there is one, else blocks the opponent's winning column when there is one, else plays uniformly --
        the ply's draw indexes the winning, else the blocking, else the legal columns."""
        return self._evaluate("evaluate_actions", "bgs_connect_evaluate_actions", None, seed, playouts, max_plies, policy)

    def evaluate_actions_tensor(self, out=None, seed: int = DEFAULT_SEED, playouts: int = 256, max_plies: int = 2**31 - 1,
                                policy: str = "uniform"):
        """`evaluate_actions` into a device tensor int32[n, width, 3] (allocated when None), enqueued on the batch's stream
        with no synchronisation.  Every entry is written."""
        return self._evaluate("evaluate_actions_tensor", "bgs_connect_evaluate_actions", (out,), seed, playouts, max_plies, policy)

    def halving_min_budget(self) -> int:
        """the least budget of `evaluate_actions_halving`: width * max(1, ceil(log2 width)), a playout a column a round"""
        return self.width * max(1, (self.width - 1).bit_length())

    def evaluate_actions_halving(self, seed: int = DEFAULT_SEED, budget: int = 1024, max_plies: int = 2**31 - 1,
                                 policy: str = "uniform"):
        """Sequential-halving Monte-Carlo evaluation of every board (bgs_connect_evaluate_actions_halving), one launch:
        (counts int32[n, width, 3], given int32[n, width], best int32[n]).  `budget` playouts a board are spent in
        R = max(1, ceil(log2 A)) rounds over its A legal columns: in round r every surviving column plays
        floor(budget / (survivors * R)) further playouts, then the better half (rounded up) survives, ranked by
        2 * wins + draws over all rounds so far, ties to the lower column.  `best` is the last survivor (-1 for an ended
        board), `given` the playouts a column was given, `counts` its cumulative (wins, draws, losses) for the player to
        move.  Playout p of column c of board i is game ((first_game + i) * width + c) * budget + p, played as
        `evaluate_actions(playouts=budget, policy=policy)` plays it: a column's counts are those of its first `given`
        playouts there.  The boards are not modified."""
        return self._halving("evaluate_actions_halving", "bgs_connect_evaluate_actions_halving", None, seed, budget, max_plies, policy)

    def evaluate_actions_halving_tensor(self, counts=None, given=None, best=None, seed: int = DEFAULT_SEED, budget: int = 1024,
                                        max_plies: int = 2**31 - 1, policy: str = "uniform"):
        """`evaluate_actions_halving` into device tensors int32[n, width, 3], int32[n, width] and int32[n] (allocated when
        None), enqueued on the batch's stream with no synchronisation: (counts, given, best).  Every entry is written."""
        return self._halving("evaluate_actions_halving_tensor", "bgs_connect_evaluate_actions_halving", (counts, given, best), seed, budget,
                             max_plies, policy)

    def search_workspace_bytes(self, iterations: int = 256) -> int:
        """bytes of device memory `search_actions` needs for its trees at `iterations` (bgs_connect_search_workspace_bytes)"""
        return self._size_query("bgs_connect_search_workspace_bytes", iterations)

    def search_actions(self, seed: int = DEFAULT_SEED, iterations: int = 256, leaf_playouts: int = 64, explore: int = DEFAULT_EXPLORE,
                       max_plies: int = 2**31 - 1, policy: str = "uniform"):
        """Batched UCT tree search of every board (bgs_connect_search_actions), one launch: (counts int32[n, width, 3],
        visits int32[n, width], best int32[n], nodes int32[n]).  Every running board is the root of a tree of its own,
        grown by `iterations` iterations: descend by UCB (integer arithmetic, include/bgs.h) to an edge never played,
        make its node, play `leaf_playouts` playouts from there by `policy`, and add them to every edge of the path.
        `explore` is about 45426 * C * C for a UCB1 constant C on rewards in [0, 1] (0: pure exploitation; at most
        2**18).  `visits` are the playouts through every root column, `counts` their (wins, draws, losses) for the player
        to move, `best` the column with the most visits (-1 for an ended board), `nodes` the nodes made.  Playout j of
        iteration t of board i is game ((first_game + i) * iterations + t) * leaf_playouts + j of the batch's RNG contract.
        The boards are not modified; the library allocates the trees' memory around the call."""
        return self._search("search_actions", False, None, None, seed, iterations, leaf_playouts, explore, max_plies, policy)

    def search_actions_tensor(self, counts=None, visits=None, best=None, nodes=None, seed: int = DEFAULT_SEED, iterations: int = 256,
                              leaf_playouts: int = 64, explore: int = DEFAULT_EXPLORE, max_plies: int = 2**31 - 1,
                              policy: str = "uniform", workspace=None):
        """`search_actions` into device tensors int32[n, width, 3], int32[n, width], int32[n] and int32[n] (allocated when
        None), enqueued on the batch's stream with no synchronisation: (counts, visits, best, nodes).  Every entry is
        written.  `workspace`: a contiguous, 256-byte aligned uint8 device tensor of at least
        `search_workspace_bytes(iterations)` bytes; None: a tensor of the batch's own, allocated on first use and kept per
        `iterations`.  The workspace needs no preparation, and calls on one stream may share it."""
        return self._search("search_actions_tensor", False, (counts, visits, best, nodes), workspace, seed, iterations, leaf_playouts,
                            explore, max_plies, policy)

    def _search(self, who: str, proving: bool, tensors, workspace, seed, iterations, leaf_playouts, explore, max_plies, policy):
        """the plain or the proving tree search, host or tensor form; both share the workspaces cached per `iterations`"""
        return self._analysis(who, "bgs_connect_search_actions_proving" if proving else "bgs_connect_search_actions",
                              _playout_args(seed, policy, iterations, leaf_playouts, explore, max_plies), self._search_specs(proving),
                              tensors, workspace, (lambda: self.search_workspace_bytes(iterations), lambda: int(iterations)))

    def search_actions_proving(self, seed: int = DEFAULT_SEED, iterations: int = 256, leaf_playouts: int = 64,
                               explore: int = DEFAULT_EXPLORE, max_plies: int = 2**31 - 1, policy: str = "uniform"):
        """`search_actions` that keeps the game-end facts it meets (bgs_connect_search_actions_proving; MCTS-Solver), one
        launch: (counts, visits, best, nodes, proved int8[n, width], done int32[n]).  An edge that ends the game is tagged
        a win or a draw, the tags are backed up by minimax beside the averages, a tagged edge is never descended again,
        and a root whose value is proved stops iterating.  `proved` holds the root's tags in the solver's codes:
        SOLVE_WIN / SOLVE_DRAW / SOLVE_LOSS for a proved column, SOLVE_UNKNOWN for a legal column still open, SOLVE_NONE
        for an illegal column or an ended board.  `done` is the number of iterations run (`iterations` for a root left
        undecided, 0 for an ended board).  `best` is the proved win if there is one, else the most visited column among
        those not proved lost.  A root whose search tags nothing returns what `search_actions` returns.  The workspace is
        `search_actions`'s."""
        return self._search("search_actions_proving", True, None, None, seed, iterations, leaf_playouts, explore, max_plies, policy)

    def search_actions_proving_tensor(self, counts=None, visits=None, best=None, nodes=None, proved=None, done=None,
                                      seed: int = DEFAULT_SEED, iterations: int = 256, leaf_playouts: int = 64,
                                      explore: int = DEFAULT_EXPLORE, max_plies: int = 2**31 - 1, policy: str = "uniform",
                                      workspace=None):
        """`search_actions_proving` into device tensors (allocated when None; `proved` is int8[n, width], the others int32
        as in `search_actions_tensor`), enqueued on the batch's stream with no synchronisation: (counts, visits, best,
        nodes, proved, done).  Every entry is written.  `workspace` is `search_actions_tensor`'s, and the batch's own
        cached workspace serves both."""
        return self._search("search_actions_proving_tensor", True, (counts, visits, best, nodes, proved, done), workspace, seed, iterations,
                            leaf_playouts, explore, max_plies, policy)

    def forest_bytes(self, capacity: int) -> int:
        """bytes of device memory a forest of this batch takes at `capacity` nodes a tree (bgs_connect_forest_bytes)"""
        return self._size_query("bgs_connect_forest_bytes", capacity)

    def search_forest(self, capacity: int) -> "SearchForest":
        """A forest for this batch: one search tree per board with room for `capacity` nodes, kept on the device from
        search to search (`SearchForest`).  The forest belongs to this batch's shape; close it before the batch."""
        return SearchForest(self, capacity)

    def guided_bytes(self, capacity: int) -> int:
        """bytes of device memory the guided trees of this batch take at `capacity` nodes a tree (bgs_connect_guided_bytes)"""
        return self._size_query("bgs_connect_guided_bytes", capacity)

    def guided_search(self, capacity: int, cpuct: int = DEFAULT_CPUCT) -> "GuidedSearch":
        """A PUCT search of this batch whose leaves the caller evaluates, e.g. with a policy/value network: one tree per
        board with room for `capacity` nodes, `cpuct` = c_puct in Q8 (`GuidedSearch`).  Close it before the batch."""
        return GuidedSearch(self, capacity, cpuct)

    def solve_actions(self, depth: Optional[int] = None, max_nodes: int = DEFAULT_SOLVE_NODES, with_plies: bool = True):
        """Exact solve of every column of every board (bgs_connect_solve_actions), one launch: (codes int8[n, width],
        plies int16[n, width] or None).  Seen from the player to move; lines of at most `depth` plies from the board,
        the column itself counted (None: a full solve).  Codes: SOLVE_WIN 1 / SOLVE_LOSS -1 (plies: to the end, the
        winner fastest, the loser slowest), SOLVE_DRAW 0 (plies: the board's empty cells), SOLVE_UNKNOWN 2 (the horizon
        cut some lines), SOLVE_BUDGET 3 (the search of that column visited more than `max_nodes` positions),
        SOLVE_NONE -2 (an illegal column or an ended board).  The boards and `steps` are not modified."""
        depth = self.height * self.width if depth is None else depth
        return self._solve("solve_actions", "bgs_connect_solve_actions", None, depth, max_nodes, with_plies)

    def solve_actions_tensor(self, codes=None, plies=None, depth: Optional[int] = None, max_nodes: int = DEFAULT_SOLVE_NODES,
                             with_plies: bool = True):
        """`solve_actions` into device tensors int8[n, width] and int16[n, width] (allocated when None; plies only
        `with_plies` or when given), enqueued on the batch's stream with no synchronisation: (codes, plies or None)."""
        depth = self.height * self.width if depth is None else depth
        return self._solve("solve_actions_tensor", "bgs_connect_solve_actions", (codes, plies), depth, max_nodes, with_plies)

    def solve_moves(self, *args, **kwargs):
        """Not available for Connect: solve_moves is the Bounce horizon search; Connect has `solve_actions`."""
        raise ValueError("solve_moves: Bounce batches only (Connect boards: solve_actions)")

    solve_moves_tensor = solve_moves

    def evaluate_moves_halving(self, *args, **kwargs):
        """Not available for Connect: evaluate_moves_halving covers Bounce boards; Connect has `evaluate_actions_halving`."""
        raise ValueError("evaluate_moves_halving: Bounce batches only (Connect boards: evaluate_actions_halving)")

    evaluate_moves_halving_tensor = evaluate_moves_halving

    def search_moves(self, *args, **kwargs):
        """Not available for Connect: search_moves is the Bounce tree search; Connect has `search_actions`."""
        raise ValueError("search_moves: Bounce batches only (Connect boards: search_actions)")

    search_moves_tensor = search_moves_workspace_bytes = search_moves

    def search_moves_proving(self, *args, **kwargs):
        """Not available for Connect: search_moves_proving is the Bounce proving search; Connect has `search_actions_proving`."""
        raise ValueError("search_moves_proving: Bounce batches only (Connect boards: search_actions_proving)")

    search_moves_proving_tensor = search_moves_proving

    @property
    def legal(self) -> np.ndarray:
        out = np.empty((self.n, self.width), dtype=np.uint8)
        _abi.check(_abi.lib().bgs_read_legal(self._handle, _ptr(out, ctypes.c_uint8)))
        return out

    def legal_tensor(self, out=None):
        t = self._torch
        if t is None:
            raise RuntimeError("legal_tensor needs torch with a GPU")
        if out is None:
            out = t.empty((self.n, self.width), dtype=t.uint8, device=f"cuda:{self.device}")
        _abi.check(_abi.lib().bgs_export_device(self._handle, ord("l"), ctypes.c_void_p(out.data_ptr())))
        return out


class SearchForest(_Forest):
    """One UCT tree per board of a ConnectBatch, kept on the device from search to search (bgs_connect_forest_search /
    bgs_connect_forest_advance, include/bgs.h): `ConnectBatch.search_forest(capacity)` makes one.  A tree has room for
    `capacity` nodes, the root included.

    The loop of an agent: `search`, play a column a board (`ConnectBatch.step_actions`), `advance` by the same columns --
    the subtree under the column played becomes the tree --, and after the opponent's reply `advance` again and `search`:
    the nodes that were carried are counted in `carried`.  A tree whose recorded root is not its board's position when a
    search starts (the board was loaded, reset or stepped without `advance`) is started anew by that search.

    The object owns the device buffer (a torch tensor) and belongs to the batch it was made from; its first search
    restarts every tree, whatever `restart` says, because fresh memory holds no trees."""

    _search_entry, _advance_entry = "bgs_connect_forest_search", "bgs_connect_forest_advance"
    _maker, _moves = "search_forest", "columns"

    def __init__(self, batch: ConnectBatch, capacity: int):
        self.batch = batch
        self.capacity = int(capacity)
        self._open(batch.forest_bytes(self.capacity))      # (refuses Bounce, generic boards and a bad capacity)

    def _sizes(self):
        return (self.capacity,)

    def search(self, seed: int = DEFAULT_SEED, iterations: int = 256, leaf_playouts: int = 64, explore: int = DEFAULT_EXPLORE,
               max_plies: int = 2**31 - 1, policy: str = "uniform", restart: bool = False):
        """`iterations` further iterations on every tree (bgs_connect_forest_search), one launch: (counts int32[n, width,
        3], visits int32[n, width], best int32[n], nodes int32[n], carried int32[n]).  `counts` are those of this call's
        playouts, `visits` the root's, carried visits included, `nodes` the nodes in the tree afterwards and `carried`
        the nodes it started with, the root not counted in either.  Vary `seed` from call to call: playout j of iteration
        t of board i is game ((first_game + i) * iterations + t) * leaf_playouts + j of every call.  `restart` empties
        every tree first."""
        return self._search(None, seed, iterations, leaf_playouts, explore, max_plies, policy, restart)

    def search_tensor(self, counts=None, visits=None, best=None, nodes=None, carried=None, seed: int = DEFAULT_SEED,
                      iterations: int = 256, leaf_playouts: int = 64, explore: int = DEFAULT_EXPLORE, max_plies: int = 2**31 - 1,
                      policy: str = "uniform", restart: bool = False):
        """`search` into device tensors int32[n, width, 3], int32[n, width] and three int32[n] (allocated when None),
        enqueued on the batch's stream with no synchronisation: (counts, visits, best, nodes, carried)."""
        return self._search((counts, visits, best, nodes, carried), seed, iterations, leaf_playouts, explore, max_plies, policy, restart)

    def advance(self, columns) -> np.ndarray:
        """Re-root every tree by its board's column (bgs_connect_forest_advance): columns int32[n], a negative entry
        leaves the tree as it is.  Returns kept int32[n], the nodes a tree holds afterwards, the root not counted: the
        subtree under the column, or 0 where there was none (the next search starts that tree anew).  The boards are
        neither read nor stepped: play the same columns with `ConnectBatch.step_actions`."""
        return self._advance(columns)

    def advance_tensor(self, columns, kept=None):
        """`advance` with `columns` and `kept` as int32[n] device tensors (kept allocated when None), enqueued on the
        batch's stream with no synchronisation: kept."""
        return self._advance(columns, kept, on_device=True)


class GuidedSearch(_Guided):
    """PUCT tree search of a ConnectBatch with caller-evaluated leaves (bgs_connect_guided_step, include/bgs.h):
    `ConnectBatch.guided_search(capacity, cpuct)` makes one.  One tree per board, `capacity` nodes a tree, the root
    included; `cpuct` is c_puct in Q8 (320 = 1.25).

    Every call is one launch on the batch's stream, with no synchronisation: it applies the evaluator's rows to the leaves
    the previous call handed out, and hands out the next ones.  `begin()` empties the trees and returns the roots as
    leaves; `step(priors, values)` is one simulation; `finish(priors, values)` applies the last evaluation and selects
    nothing.  Each returns the same seven device tensors, allocated once and rewritten by every call:
    (leaf_grid int8[n, h, w], leaf_player int8[n], leaf_kind int32[n], visits int32[n, w], scores int32[n, w],
    best int32[n], nodes int32[n]).  `priors` float32[n, w] and `values` float32[n] are the evaluator's output for
    (leaf_grid, leaf_player) of the previous call: a value is seen from the player to move at the leaf, in [-1, 1]; rows
    whose leaf_kind is not GUIDED_EVALUATE are ignored.  A board that was stepped or reset between two calls restarts its
    tree on its own.  The boards and `steps` are not modified.

    The object owns the device buffer of the trees (a torch tensor) and belongs to the batch it was made from."""

    _entry, _maker, _priors, _leaves = "bgs_connect_guided_step", "guided_search", "float32[n, width]", (0, 1)

    def __init__(self, batch: "ConnectBatch", capacity: int, cpuct: int = DEFAULT_CPUCT):
        self.batch = batch
        self.capacity = int(capacity)
        self.cpuct = int(cpuct)
        self._check_cpuct(cpuct)
        n, h, w = batch.n, batch.height, batch.width
        self._open(batch.guided_bytes(self.capacity),      # (refuses Bounce, generic boards and a bad capacity)
                   [("leaf_grid", (n, h, w), "int8"), ("leaf_player", (n,), "int8"), ("leaf_kind", (n,)), ("visits", (n, w)),
                    ("scores", (n, w)), ("best", (n,)), ("nodes", (n,))])

    def _scalars(self):
        return (self.capacity, self.cpuct)

    def finish(self, priors, values):
        """Apply (priors, values) to the leaves of the previous call and select nothing (BGS_GUIDED_FINISH): every
        leaf_kind comes back GUIDED_IDLE, and visits, scores, best and nodes are final."""
        return self._call(_abi.GUIDED_FINISH, priors, values)

    def run(self, evaluate, simulations: int):
        """`begin`, `simulations` evaluations a tree, `finish`: evaluate(leaf_grid, leaf_player) -> (priors float32[n, w],
        values float32[n]) is called once a simulation on the device tensors of the leaves (the first call sees the
        roots) and returns device tensors.  Returns what `finish` returns."""
        return self._run(evaluate, simulations)


class GuidedForest(GuidedSearch):
    """A GuidedSearch whose trees are kept from move to move (bgs_connect_guided_advance, include/bgs.h):
    `GuidedForest(batch, capacity, cpuct)` makes one for a ConnectBatch -- the batch has no maker method for it.  The
    re-rooting bounds the room of a tree: `capacity` <= GUIDED_ADVANCE_MAX_CAPACITY.

    The loop of self-play: `run(evaluate, simulations)` once, then per move: pick a column a board from `visits`, play
    it (`ConnectBatch.step_actions` or `step_actions_observe`), `advance` by the same columns -- the subtree under the
    column played becomes the tree, with every evaluation in it --, and `run(evaluate, simulations, carry=True)`, which
    searches on from what was kept.  A tree whose column had no subtree, or whose board is not at the recorded position
    when the next step looks (it was not stepped, or stepped elsewhere, or reset), starts anew on its own.  `visits`,
    `scores` and `nodes` of a carried tree include what was carried.

    `begin`, `step`, `finish` and `close` are GuidedSearch's."""

    def __init__(self, batch: "ConnectBatch", capacity: int, cpuct: int = DEFAULT_CPUCT):
        if capacity > _abi.GUIDED_ADVANCE_MAX_CAPACITY:
            raise ValueError(f"capacity must be at most {_abi.GUIDED_ADVANCE_MAX_CAPACITY} nodes a tree for trees that are advanced "
                             f"(got {capacity})")
        super().__init__(batch, capacity, cpuct)
        t = batch._torch
        # what `resume` hands the step: rows that no tree reads, because no tree has a leaf pending
        self._no_rows = (t.zeros(batch._per_action(), dtype=t.float32, device=f"cuda:{batch.device}"),
                         t.zeros((batch.n,), dtype=t.float32, device=f"cuda:{batch.device}"))
        self._last = None       # the last call: "begin", "step", "finish", "advance", "resume"; None: fresh memory

    def _call(self, flags: int, priors, values):
        outs = super()._call(flags, priors, values)
        self._last = "begin" if flags & _abi.GUIDED_RESTART else "finish" if flags & _abi.GUIDED_FINISH else "step"
        return outs

    def advance(self, columns, kept=None):
        """Re-root every tree by its board's column (bgs_connect_guided_advance), enqueued on the batch's stream with no
        synchronisation: `columns` is an int32[n] device tensor, a negative entry leaves the tree as it is.  Returns
        `kept`, an int32[n] device tensor (allocated when None): the nodes a tree holds afterwards, the root not counted
        -- the subtree under the column, or 0 where there was none (the next step starts that tree anew).  The boards
        are neither read nor stepped: play the same columns with `ConnectBatch.step_actions` before the next step.
        RuntimeError while an evaluation is pending (the last call was `begin` or `step`): `finish` comes first."""
        if self._buffer is None:
            raise RuntimeError("the guided search is closed")
        if self._last is None:
            raise RuntimeError("begin() comes first: fresh memory holds no trees")
        if self._last in ("begin", "step"):
            raise RuntimeError("finish() comes first: an evaluation is pending, and an advance would drop it")
        n = self.batch.n    # (columns is an input: "optional", so that it is checked and never allocated)
        columns, kept = self.batch._device_tensors("GuidedForest.advance", [("columns", columns, (n,), "int32", True), ("kept", kept, (n,))])
        if columns is None:
            raise TypeError(f"columns must be an int32 device tensor of shape ({n},)")
        _abi.check(_abi.lib().bgs_connect_guided_advance(
            self.batch._handle, ctypes.c_void_p(columns.data_ptr()), ctypes.c_int32(self.capacity), ctypes.c_void_p(kept.data_ptr()),
            ctypes.c_void_p(self._buffer.data_ptr()), ctypes.c_size_t(self._buffer.numel())))
        self._last = "advance"
        return kept

    def resume(self):
        """The step with nothing to apply, on rows the object holds itself: every tree reports and selects its next
        leaf, a carried tree from what it holds, an emptied one from its board.  Returns the seven outputs; `step` or
        `finish` take the evaluator's rows for them, as after `begin`.  (A second `resume` in their place would feed
        those leaves the object's own rows: zeros, that is flat priors and a value of 0.)
        RuntimeError unless the last call was `finish`, `advance` or `resume`."""
        if self._buffer is None:
            raise RuntimeError("the guided search is closed")
        if self._last not in ("finish", "advance", "resume"):
            raise RuntimeError("resume() follows finish(), advance() or resume()" +
                               (": begin() comes first, fresh memory holds no trees" if self._last is None else
                                ": an evaluation is pending, finish() comes first"))
        outs = self._call(0, *self._no_rows)
        self._last = "resume"
        return outs

    def run(self, evaluate, simulations: int, carry: bool = False):
        """`GuidedSearch.run`, and with `carry` the same on the trees as they are: `resume` in place of `begin`, then
        `simulations` evaluations a tree and `finish`.  A carried root has its P, so all `simulations` evaluations go
        below it.  RuntimeError with `carry` on fresh memory."""
        if not carry:
            return self._run(evaluate, simulations)
        if simulations < 1:
            raise ValueError(f"simulations must be >= 1 (got {simulations})")
        if self._last is None:
            raise RuntimeError("carry=True on fresh memory: there are no trees to carry")
        outs = self.resume()
        for _ in range(int(simulations) - 1):
            outs = self.step(*evaluate(*(outs[i] for i in self._leaves)))
        return self.finish(*evaluate(*(outs[i] for i in self._leaves)))


class BounceBatch(_Batch):
    """N Bounce boards sharing one start grid: ``Config(grid)`` (reference bounce.cpp:26) times n."""

    game = _abi.GAME_BOUNCE
    _action_width = 4
    _search_counters = ("best", "nodes", "used")   # the int32[n] outputs of a tree search

    def _per_action(self):
        """the shape of an entry a move slot of every board: [i, x, c] is the move of column x's piece to cell c"""
        return (self.n, self.width, self.height * self.width)

    def _empty_legal(self):
        if self.generic:  # wide record: int32 active row, then uint8 flags[W][H * W] (include/bgs.h, bgs_legal_bytes)
            return np.empty((self.n, self._legal_bytes), dtype=np.uint8)
        return np.empty((self.n, self.width + 1), dtype=np.uint64)

    def decode_moves(self, legal_row, winner: int):
        """One board's legal-move record (either format) -> tuple of ((sx, sy), (tx, ty)) in canonical order."""
        width, height = self.width, self.height
        moves = []
        if winner != -1:
            return ()
        if self.generic:
            row = int(legal_row[:4].view(np.int32)[0])
            if row < 0:
                return ()
            flags = legal_row[4 : 4 + width * height * width].reshape(width, height * width)
            for x in range(width):
                for c in np.flatnonzero(flags[x]):
                    moves.append(((x, row), (int(c) % width, int(c) // width)))
            return tuple(moves)
        masks = legal_row.tolist()
        row = masks[width]
        if row >= height:  # all ones: nothing can move
            return ()
        cells = self._cells  # cell index -> (x, y), built once
        for x in range(width):
            m = masks[x]
            source = (x, row)
            while m:
                low = m & -m
                moves.append((source, cells[low.bit_length() - 1]))
                m ^= low
        return tuple(moves)

    def __init__(self, grid, n: int, device: int = 0, use_torch: Optional[bool] = None):
        cfg = np.ascontiguousarray(grid)
        if cfg.ndim != 2:
            raise TypeError("Bounce config grid must be 2-dimensional")
        if not np.issubdtype(cfg.dtype, np.integer):
            raise TypeError("Bounce config grid must be an integer array")
        if cfg.size and (cfg.min() < -128 or cfg.max() > 127):
            raise TypeError("Bounce config grid does not fit int8")
        cfg = cfg.astype(np.int8)
        super().__init__(n, cfg.shape[0], cfg.shape[1], device, use_torch)
        self.config_grid = cfg
        self._search_workspaces = {}   # (iterations, edges) -> the uint8 device tensor search_moves_tensor allocated
        nbytes = ctypes.c_size_t()
        _abi.check(_abi.lib().bgs_bounce_arena_bytes(self.height, self.width, self.n, ctypes.byref(nbytes)))
        arena, arena_bytes = self._make_arena(nbytes.value)
        _abi.check(
            _abi.lib().bgs_bounce_create(
                _ptr(cfg, ctypes.c_int8), self.height, self.width, self.n, self.device, arena, arena_bytes, ctypes.byref(self._handle)
            )
        )
        self._cells = tuple((c % self.width, c // self.width) for c in range(self.height * self.width))
        self._after_create()

    def evaluate_actions(self, *args, **kwargs):
        """Not available for Bounce: evaluate_actions covers bit-packed Connect boards; Bounce has `evaluate_moves`."""
        raise ValueError("evaluate_actions: Connect batches only (Bounce boards: evaluate_moves)")

    evaluate_actions_tensor = evaluate_actions

    def evaluate_actions_halving(self, *args, **kwargs):
        """Not available for Bounce: sequential halving covers bit-packed Connect boards; Bounce has `evaluate_moves`."""
        raise ValueError("evaluate_actions_halving: Connect batches only (Bounce boards: evaluate_moves)")

    evaluate_actions_halving_tensor = evaluate_actions_halving

    def search_actions(self, *args, **kwargs):
        """Not available for Bounce: the tree search covers bit-packed Connect boards; Bounce has `evaluate_moves_halving`."""
        raise ValueError("search_actions: Connect batches only (Bounce boards: evaluate_moves_halving)")

    search_actions_tensor = search_workspace_bytes = search_actions

    def search_actions_proving(self, *args, **kwargs):
        """Not available for Bounce: search_actions_proving is the Connect proving search; Bounce has `search_moves_proving`."""
        raise ValueError("search_actions_proving: Connect batches only (Bounce boards: search_moves_proving)")

    search_actions_proving_tensor = search_actions_proving

    def search_forest(self, *args, **kwargs):
        """Not available for Bounce: trees that persist between searches cover bit-packed Connect boards."""
        raise ValueError("search_forest: Connect batches only (Bounce boards: search_moves)")

    forest_bytes = search_forest

    def guided_search(self, *args, **kwargs):
        """Not available for Bounce: `guided_search` and `guided_bytes` are the Connect calls, a prior a column.  Bounce
        has `guided_moves_search` and `guided_moves_bytes`, a prior a move slot."""
        raise ValueError("guided_search: Connect batches only")

    guided_bytes = guided_search

    def guided_default_edges(self, nodes: int) -> int:
        """the edge pool `guided_moves_search` takes with edges=None: `search_min_edges()` + 32 * (nodes - 1), the allowance
        of `search_moves`: 32 edges a node that is not the root"""
        return self.search_min_edges() + 32 * max(int(nodes) - 1, 0)

    def guided_moves_bytes(self, nodes: int, edges: Optional[int] = None) -> int:
        """bytes of device memory the guided trees of this batch take at `nodes` nodes and `edges` pool edges a tree (None:
        `guided_default_edges(nodes)`; bgs_bounce_guided_bytes)"""
        return self._size_query("bgs_bounce_guided_bytes", nodes, self.guided_default_edges(nodes) if edges is None else int(edges))

    def guided_moves_search(self, nodes: int, edges: Optional[int] = None, cpuct: int = DEFAULT_CPUCT,
                            max_plies: int = 65535) -> "GuidedMovesSearch":
        """A PUCT search of this batch whose leaves the caller evaluates, e.g. with a policy/value network: one tree per
        board with room for `nodes` nodes, the root included, and `edges` pool edges (None: `guided_default_edges(nodes)`),
        `cpuct` = c_puct in Q8; a position that holds `max_plies` plies is a draw (`GuidedMovesSearch`).  Close it before
        the batch."""
        return GuidedMovesSearch(self, nodes, edges, cpuct, max_plies)

    def solve_actions(self, *args, **kwargs):
        """Not available for Bounce: the exact solver covers bit-packed Connect boards (Bounce games can cycle)."""
        raise ValueError("solve_actions: Connect batches only")

    solve_actions_tensor = solve_actions

    def evaluate_moves(self, seed: int = DEFAULT_SEED, playouts: int = 256, max_plies: int = 2**31 - 1,
                       policy: str = "uniform") -> np.ndarray:
        """Flat Monte-Carlo evaluation of every legal move of every board (bgs_bounce_evaluate_moves), one launch:
        int32[n, W, H * W, 3]; entry [i, x, c] = (wins, draws, losses) of the player to move over `playouts` games that
        start with the move of the piece in column x of the active row to cell c = ty * W + tx (bit c of targets[i, x])
        and continue by the uniform random policy until they end or hold `max_plies` plies (clamped to 65535; a capped game
        counts in none of the three).  Illegal slots and ended boards give 0, 0, 0.  The boards are not modified.
        Playout p of slot s = x * H * W + c of board i is game ((first_game + i) * W * H * W + s) * playouts + p.
        policy="decisive" (bgs_bounce_evaluate_moves_policy): the same games and draws, but a ply whose side to move can
        land in its goal row does so -- the ply's draw indexes the winning moves, else all moves.  There is no blocking
        step."""
        return self._evaluate("evaluate_moves", "bgs_bounce_evaluate_moves", None, seed, playouts, max_plies, policy)

    def evaluate_moves_tensor(self, out=None, seed: int = DEFAULT_SEED, playouts: int = 256, max_plies: int = 2**31 - 1,
                              policy: str = "uniform"):
        """`evaluate_moves` into a device tensor int32[n, W, H * W, 3] (allocated when None), enqueued on the batch's stream
        with no synchronisation.  Every entry is written."""
        return self._evaluate("evaluate_moves_tensor", "bgs_bounce_evaluate_moves", (out,), seed, playouts, max_plies, policy)

    @staticmethod
    def halving_min_budget(moves: int) -> int:
        """the least budget of `evaluate_moves_halving` for a board with `moves` legal moves: moves * max(1, ceil(log2
        moves)), a playout a move a round"""
        return int(moves) * max(1, (int(moves) - 1).bit_length())

    def evaluate_moves_halving(self, seed: int = DEFAULT_SEED, budget: int = 1024, max_plies: int = 2**31 - 1,
                               policy: str = "uniform"):
        """Sequential-halving Monte-Carlo evaluation of every board (bgs_bounce_evaluate_moves_halving), one launch:
        (counts int32[n, W, H * W, 3], given int32[n, W, H * W], best int32[n]); entry [i, x, c] is the move of the piece
        in column x of the active row to cell c = ty * W + tx, as in `evaluate_moves`.  `budget` playouts a board are
        spent in R = max(1, ceil(log2 A)) rounds over its A legal moves: in round r every surviving move plays
        floor(budget / (survivors * R)) further playouts, then the better half (rounded up) survives, ranked by
        2 * wins + draws over all rounds so far, ties to the lower slot x * H * W + c.  `best` is the slot of the last
        survivor, `given` the playouts a move was given, `counts` its cumulative (wins, draws, losses) for the player to
        move.  A board that has ended or has no legal move: all zeros and best = -1.  A running board with
        budget < `halving_min_budget(A)`: all zeros and best = HALVING_SHORT; the other boards are evaluated as usual.
        Playout p of slot s of board i is game ((first_game + i) * W * H * W + s) * budget + p, played as
        `evaluate_moves(playouts=budget, policy=policy)` plays it: a move's counts are those of its first `given`
        playouts there.  The boards are not modified."""
        return self._halving("evaluate_moves_halving", "bgs_bounce_evaluate_moves_halving", None, seed, budget, max_plies, policy)

    def evaluate_moves_halving_tensor(self, counts=None, given=None, best=None, seed: int = DEFAULT_SEED, budget: int = 1024,
                                      max_plies: int = 2**31 - 1, policy: str = "uniform"):
        """`evaluate_moves_halving` into device tensors int32[n, W, H * W, 3], int32[n, W, H * W] and int32[n] (allocated
        when None), enqueued on the batch's stream with no synchronisation: (counts, given, best).  Every entry is
        written."""
        return self._halving("evaluate_moves_halving_tensor", "bgs_bounce_evaluate_moves_halving", (counts, given, best), seed, budget,
                             max_plies, policy)

    def search_min_edges(self) -> int:
        """BGS_BOUNCE_SEARCH_MIN_EDGES(H, W): the most arms a position of this geometry can have, W * W * (H - 2)"""
        return self.width * self.width * (self.height - 2) if self.height >= 3 else 1

    def search_default_edges(self, iterations: int) -> int:
        """the edge pool `search_moves` takes with edges=None: min((T + 1) * MIN, MIN + 32 * T), MIN = `search_min_edges()`.
        The 32 edges a node are an allowance over the about 12 arms of a node of the default board; it is NOT measured:
        docs/EXPERIMENTS.md section 28 holds the share of roots whose pool ran dry, once a GPU run has produced it."""
        least, t = self.search_min_edges(), max(int(iterations), 0)
        return min((t + 1) * least, least + 32 * t, 2**31 - 1)

    def search_moves_workspace_bytes(self, iterations: int = 256, edges: Optional[int] = None) -> int:
        """bytes of device memory `search_moves` needs for its trees at `iterations` and `edges` (None: the default pool;
        bgs_bounce_search_workspace_bytes)"""
        edges = self.search_default_edges(iterations) if edges is None else int(edges)
        return self._size_query("bgs_bounce_search_workspace_bytes", iterations, edges)

    def search_moves(self, seed: int = DEFAULT_SEED, iterations: int = 256, leaf_playouts: int = 64, explore: int = DEFAULT_EXPLORE,
                     max_plies: int = 2**31 - 1, policy: str = "uniform", edges: Optional[int] = None):
        """Batched UCT tree search of every board (bgs_bounce_search_moves), one launch: (counts int32[n, W, H * W, 3],
        visits int32[n, W, H * W], best int32[n], nodes int32[n], used int32[n]); entry [i, x, c] is the move of the piece
        in column x of the active row to cell c = ty * W + tx, as in `evaluate_moves`.  Every running board is the root of
        a tree of its own, grown by `iterations` iterations: descend by UCB (integer arithmetic, include/bgs.h) over the
        legal moves to an edge without a node, make its node if the pool has room, play `leaf_playouts` playouts from
        there by `policy`, and add them to every edge of the path.  `explore` is about 45426 * C * C for a UCB1 constant
        C on rewards in [0, 1] (0: pure exploitation; at most 2**18).  `visits` are the playouts through every root move,
        `counts` their (wins, draws, losses) for the player to move, `best` the slot x * H * W + c with the most visits
        (-1 for a board that has ended or has no move), `nodes` the nodes made, `used` the pool edges in use at the end.
        `edges` is the edge pool of a root, at least `search_min_edges()`; None: `search_default_edges(iterations)`, an
        allowance of 32 edges a node that is not measured (docs/EXPERIMENTS.md section 28).  A node that does not fit is
        not made and its edge is tried again later: used + (the arms of some position) > edges says the pool ran dry.
        Playout j of iteration t of board i is game ((first_game + i) * iterations + t) * leaf_playouts + j; `max_plies`
        is clamped to 65535.  The boards are not modified; the library allocates the trees' memory around the call."""
        return self._search("search_moves", False, None, None, seed, iterations, leaf_playouts, explore, max_plies, policy, edges)

    def search_moves_tensor(self, counts=None, visits=None, best=None, nodes=None, used=None, seed: int = DEFAULT_SEED,
                            iterations: int = 256, leaf_playouts: int = 64, explore: int = DEFAULT_EXPLORE, max_plies: int = 2**31 - 1,
                            policy: str = "uniform", edges: Optional[int] = None, workspace=None):
        """`search_moves` into device tensors int32[n, W, H * W, 3], int32[n, W, H * W] and three int32[n] (allocated when
        None), enqueued on the batch's stream with no synchronisation: (counts, visits, best, nodes, used).  Every entry
        is written.  `workspace`: a contiguous, 256-byte aligned uint8 device tensor of at least
        `search_moves_workspace_bytes(iterations, edges)` bytes; None: a tensor of the batch's own, allocated on first use
        and kept per (iterations, edges).  The workspace needs no preparation, and calls on one stream may share it."""
        return self._search("search_moves_tensor", False, (counts, visits, best, nodes, used), workspace, seed, iterations, leaf_playouts,
                            explore, max_plies, policy, edges)

    def _search(self, who: str, proving: bool, tensors, workspace, seed, iterations, leaf_playouts, explore, max_plies, policy, edges):
        """the plain or the proving tree search, host or tensor form, with the default edge pool for edges=None; both share
        the workspaces cached per (iterations, edges)"""
        scalars = _playout_args(seed, policy, iterations, leaf_playouts, explore, max_plies)
        edges = self.search_default_edges(iterations) if edges is None else int(edges)
        return self._analysis(who, "bgs_bounce_search_moves_proving" if proving else "bgs_bounce_search_moves",
                              scalars + [ctypes.c_int32(edges)], self._search_specs(proving), tensors, workspace,
                              (lambda: self.search_moves_workspace_bytes(iterations, edges), lambda: (int(iterations), edges)))

    def search_moves_proving(self, seed: int = DEFAULT_SEED, iterations: int = 256, leaf_playouts: int = 64,
                             explore: int = DEFAULT_EXPLORE, max_plies: int = 2**31 - 1, policy: str = "uniform",
                             edges: Optional[int] = None):
        """`search_moves` that keeps the game-end facts it meets (bgs_bounce_search_moves_proving; MCTS-Solver), one launch:
        (counts, visits, best, nodes, used, proved int8[n, W, H * W], done int32[n]).  An edge that ends the game -- a move
        into the goal row, a blocked side -- is tagged a win or a draw, the tags are backed up by minimax beside the
        averages, a tagged edge is never descended again, and a root whose value is proved stops iterating.  `proved`
        holds the root's tags by slot in the solver's codes: SOLVE_WIN / SOLVE_DRAW / SOLVE_LOSS for a proved move,
        SOLVE_UNKNOWN for a legal move still open, SOLVE_NONE for an illegal slot and for a board that has ended or has no
        move.  `done` is the number of iterations run (`iterations` for a root left undecided, 0 for a board without
        moves).  `best` is the proved win if there is one, else the most visited move among those not proved lost.  A
        move whose position holds the cap proves nothing.  A root whose search plays no move that ends the game returns
        what `search_moves` returns.  The workspace and `edges` are `search_moves`'s."""
        return self._search("search_moves_proving", True, None, None, seed, iterations, leaf_playouts, explore, max_plies, policy, edges)

    def search_moves_proving_tensor(self, counts=None, visits=None, best=None, nodes=None, used=None, proved=None, done=None,
                                    seed: int = DEFAULT_SEED, iterations: int = 256, leaf_playouts: int = 64,
                                    explore: int = DEFAULT_EXPLORE, max_plies: int = 2**31 - 1, policy: str = "uniform",
                                    edges: Optional[int] = None, workspace=None):
        """`search_moves_proving` into device tensors (allocated when None; `proved` is int8[n, W, H * W], the others int32
        as in `search_moves_tensor`), enqueued on the batch's stream with no synchronisation: (counts, visits, best, nodes,
        used, proved, done).  Every entry is written.  `workspace` is `search_moves_tensor`'s, and the batch's own cached
        workspace serves both."""
        return self._search("search_moves_proving_tensor", True, (counts, visits, best, nodes, used, proved, done), workspace, seed,
                            iterations, leaf_playouts, explore, max_plies, policy, edges)

    def moves_forest_bytes(self, nodes: int, edges: Optional[int] = None) -> int:
        """bytes of device memory a forest of this batch takes at `nodes` nodes and `edges` pool edges a tree (None: the
        default pool of `search_moves_forest`; bgs_bounce_forest_bytes)"""
        edges = self.search_default_edges(int(nodes) - 1) if edges is None else int(edges)
        return self._size_query("bgs_bounce_forest_bytes", nodes, edges)

    def search_moves_forest(self, nodes: int, edges: Optional[int] = None) -> "MovesForest":
        """A forest for this batch: one search tree per board with room for `nodes` nodes, the root included, and `edges`
        pool edges, kept on the device from search to search (`MovesForest`).  edges=None: `search_default_edges(nodes -
        1)`, the pool `search_moves` takes for as many iterations as the tree can make nodes -- the allowance of 32 edges
        a node that is NOT measured (docs/EXPERIMENTS.md section 28).  The forest belongs to this batch's shape; close it
        before the batch."""
        return MovesForest(self, nodes, edges)

    def slots_to_moves(self, slots) -> np.ndarray:
        """moves int32[n, 4] (source x, y, target x, y: what `step_actions` takes) of slots int32[n] -- the encoding of
        `best`, x * H * W + c -- on the batch's CURRENT boards: the source row is the active row of board i, which the
        slot does not hold.  A negative slot, and a board whose side to move cannot move, give a row of -1 (skipped by
        `step_actions`).  The slot is not checked against the legal moves: `step_actions` does that."""
        slots = np.asarray(slots, dtype=np.int64)
        if slots.shape != (self.n,):
            raise TypeError(f"slots must be int32[{self.n}]")
        hw = self.height * self.width
        row = self.targets[:, self.width]
        moves = np.full((self.n, 4), -1, dtype=np.int32)
        ok = (slots >= 0) & (slots < self.width * hw) & (row < np.uint64(self.height))
        cell = slots[ok] % hw
        moves[ok] = np.stack([slots[ok] // hw, row[ok].astype(np.int64), cell % self.width, cell // self.width], axis=1)
        return moves

    def slots_to_moves_tensor(self, slots, targets=None):
        """`slots_to_moves` on the device: int32[n, 4] of slots int32[n] (a device tensor).  `targets` are the target
        masks int64[n, W + 1] of the batch's current boards (`targets_tensor()`, or what `step_actions_observe` returned
        last); None: they are exported here.  No synchronisation; the result feeds `step_actions_observe`."""
        t = self._need_torch("slots_to_moves_tensor")
        if targets is None:
            targets = self.targets_tensor()
        hw = self.height * self.width
        slot = slots.to(t.int64)
        row = targets[:, self.width].to(t.int64)
        cell = slot % hw
        moves = t.stack([slot // hw, row, cell % self.width, cell // self.width], dim=1)
        ok = (slot >= 0) & (slot < self.width * hw) & (row >= 0) & (row < self.height)      # (all ones: nothing can move)
        return t.where(ok[:, None], moves, t.full_like(moves, -1)).to(t.int32).contiguous()

    def solve_moves(self, depth: int = DEFAULT_BOUNCE_SOLVE_DEPTH, max_nodes: int = DEFAULT_SOLVE_NODES, with_plies: bool = True):
        """Exact horizon search of every legal move of every board (bgs_bounce_solve_moves), one launch: (codes int8[n, W,
        H * W], plies int16[n, W, H * W] or None); entry [i, x, c] is the move of the piece in column x of the active row
        to cell c = ty * W + tx, seen from the player to move, over lines of at most `depth` plies from the board (the
        move itself counted; 1 .. BOUNCE_SOLVE_MAX_DEPTH -- Bounce games can cycle, there is no full solve).  Codes:
        SOLVE_WIN 1 / SOLVE_LOSS -1 (plies: to the end, the winner fastest, the loser slowest), SOLVE_DRAW 0 (the move
        itself ends the game as a draw; plies 1), SOLVE_UNKNOWN 2 (neither side can force a win within the horizon),
        SOLVE_BUDGET 3 (the search of that move visited more than `max_nodes` positions), SOLVE_NONE -2 (an illegal slot,
        an ended board).  The boards and `steps` are not modified."""
        return self._solve("solve_moves", "bgs_bounce_solve_moves", None, depth, max_nodes, with_plies)

    def solve_moves_tensor(self, codes=None, plies=None, depth: int = DEFAULT_BOUNCE_SOLVE_DEPTH,
                           max_nodes: int = DEFAULT_SOLVE_NODES, with_plies: bool = True):
        """`solve_moves` into device tensors int8[n, W, H * W] and int16[n, W, H * W] (allocated when None; plies only
        `with_plies` or when given), enqueued on the batch's stream with no synchronisation: (codes, plies or None)."""
        return self._solve("solve_moves_tensor", "bgs_bounce_solve_moves", (codes, plies), depth, max_nodes, with_plies)

    def step_actions(self, moves, want_status: bool = True):
        """moves int32[n, 4] = source x, y, target x, y; a negative first entry skips the board."""
        return self._step_actions(moves, 4, want_status)

    def targets_tensor(self, out=None):
        """int64[n, W + 1] on the device (bgs_export_device 't'; the bits of `targets`, as torch's signed 64-bit type)."""
        t = self._need_torch("targets_tensor")
        if self.generic:
            raise ValueError("this board does not fit 64-bit target masks: use transition() / decode_moves()")
        if out is None:
            out = t.empty((self.n, self.width + 1), dtype=t.int64, device=f"cuda:{self.device}")
        return self._export("t", out)

    @property
    def targets(self) -> np.ndarray:
        """uint64[n, W + 1]: entry i < W has bit (y * W + x) set for each legal target of the piece in column i of the
        active row; entry W is the active row's y (all ones when nothing can move)."""
        if self.generic:
            raise ValueError("this board does not fit 64-bit target masks: use transition() / decode_moves()")
        out = np.empty((self.n, self.width + 1), dtype=np.uint64)
        _abi.check(_abi.lib().bgs_bounce_read_targets(self._handle, _ptr(out, ctypes.c_uint64)))
        return out


class MovesForest(_Forest):
    """One UCT tree per board of a BounceBatch, kept on the device from search to search (bgs_bounce_forest_search /
    bgs_bounce_forest_advance, include/bgs.h): `BounceBatch.search_moves_forest(nodes, edges)` makes one.  A tree has room
    for `nodes` nodes, the root included, and `edges` pool edges.

    The loop of an agent: `search`, play a move a board (`BounceBatch.step_actions`; `BounceBatch.slots_to_moves` turns
    `best` into its moves BEFORE the boards are stepped), `advance` by the same slots -- the subtree under the move played
    becomes the tree --, and after the opponent's reply `advance` again and `search`: the nodes that were carried are
    counted in `carried`.  A tree whose recorded root is not its board's position and ply count when a search starts (the
    board was loaded, reset or stepped without `advance`), or that was grown under another `max_plies`, is started anew
    by that search.

    The object owns the device buffer (a torch tensor) and belongs to the batch it was made from; its first search
    restarts every tree, whatever `restart` says, because fresh memory holds no trees."""

    _search_entry, _advance_entry = "bgs_bounce_forest_search", "bgs_bounce_forest_advance"
    _maker, _moves = "search_moves_forest", "slots"

    def __init__(self, batch: BounceBatch, nodes: int, edges: Optional[int] = None):
        self.batch = batch
        self.nodes = int(nodes)
        self.edges = batch.search_default_edges(self.nodes - 1) if edges is None else int(edges)
        self._open(batch.moves_forest_bytes(self.nodes, self.edges))     # (refuses Connect, generic boards, bad nodes or edges)

    def _sizes(self):
        return (self.nodes, self.edges)

    def search(self, seed: int = DEFAULT_SEED, iterations: int = 256, leaf_playouts: int = 64, explore: int = DEFAULT_EXPLORE,
               max_plies: int = 2**31 - 1, policy: str = "uniform", restart: bool = False):
        """`iterations` further iterations on every tree (bgs_bounce_forest_search), one launch: (counts int32[n, W, H * W,
        3], visits int32[n, W, H * W], best int32[n], nodes int32[n], used int32[n], carried int32[n]); entry [i, x, c] is
        the move of the piece in column x of the active row to cell c, as in `BounceBatch.search_moves`.  `counts` are
        those of this call's playouts, `visits` the root's, carried visits included, `nodes` the nodes in the tree
        afterwards, `used` its pool edges in use and `carried` the nodes it started with, the root counted in neither
        node count.  Vary `seed` from call to call: playout j of iteration t of board i is game ((first_game + i) *
        iterations + t) * leaf_playouts + j of every call.  `max_plies` is clamped to 65535, and a tree grown under
        another cap is started anew.  `restart` empties every tree first."""
        return self._search(None, seed, iterations, leaf_playouts, explore, max_plies, policy, restart)

    def search_tensor(self, counts=None, visits=None, best=None, nodes=None, used=None, carried=None, seed: int = DEFAULT_SEED,
                      iterations: int = 256, leaf_playouts: int = 64, explore: int = DEFAULT_EXPLORE, max_plies: int = 2**31 - 1,
                      policy: str = "uniform", restart: bool = False):
        """`search` into device tensors int32[n, W, H * W, 3], int32[n, W, H * W] and four int32[n] (allocated when None),
        enqueued on the batch's stream with no synchronisation: (counts, visits, best, nodes, used, carried)."""
        return self._search((counts, visits, best, nodes, used, carried), seed, iterations, leaf_playouts, explore, max_plies, policy,
                            restart)

    def advance(self, slots) -> np.ndarray:
        """Re-root every tree by its board's move (bgs_bounce_forest_advance): slots int32[n] in the encoding of `best`
        (x * H * W + c on the position the tree's root stands for), a negative entry leaves the tree as it is.  Returns
        kept int32[n], the nodes a tree holds afterwards, the root not counted: the subtree under the move, or 0 where
        there was none (the next search starts that tree anew).  The boards are neither read nor stepped: play the same
        moves with `BounceBatch.step_actions`."""
        return self._advance(slots)

    def advance_tensor(self, slots, kept=None):
        """`advance` with `slots` and `kept` as int32[n] device tensors (kept allocated when None), enqueued on the
        batch's stream with no synchronisation: kept."""
        return self._advance(slots, kept, on_device=True)


class GuidedMovesSearch(_Guided):
    """PUCT tree search of a BounceBatch with caller-evaluated leaves (bgs_bounce_guided_step, include/bgs.h):
    `BounceBatch.guided_moves_search(nodes, edges, cpuct, max_plies)` makes one.  One tree per board, `nodes` nodes a tree,
    the root included, and `edges` pool edges; `cpuct` is c_puct in Q8 (320 = 1.25); `max_plies` is clamped to 65535.

    The calls are those of `GuidedSearch`: `begin()` empties the trees and returns the roots as leaves, `step(priors,
    values)` is one simulation, `finish(priors, values)` applies the last evaluation and selects nothing; each is one
    launch on the batch's stream, with no synchronisation.  Each returns the same nine device tensors, allocated once and
    rewritten by every call: (leaf_grid int8[n, H, W], leaf_player int8[n], leaf_kind int32[n], leaf_targets int64[n, W],
    visits int32[n, W, H * W], scores int32[n, W, H * W], best int32[n], nodes int32[n], used int32[n]).  Entry [i, x, c]
    is the move of the piece in column x of the active row to cell c = ty * W + tx, as in `BounceBatch.search_moves`;
    `leaf_targets[i, x]` has bit c set for every legal one of an EVALUATE leaf (the bits of `BounceBatch.targets`, as
    torch's signed 64-bit type) and is zero for every other kind: it is the mask of the evaluator's softmax.  `priors`
    float32[n, W, H * W] and `values` float32[n] are the evaluator's output for the previous call's leaves: a value is seen
    from the player to move at the leaf, in [-1, 1]; rows whose leaf_kind is not GUIDED_EVALUATE are ignored.  A board that
    was stepped or reset between two calls restarts its tree on its own.  The boards and `steps` are not modified.

    The object owns the device buffer of the trees (a torch tensor) and belongs to the batch it was made from."""

    _entry, _maker, _priors, _leaves = "bgs_bounce_guided_step", "guided_moves_search", "float32[n, W, H * W]", (0, 1, 3)

    def __init__(self, batch: "BounceBatch", nodes: int, edges: Optional[int] = None, cpuct: int = DEFAULT_CPUCT,
                 max_plies: int = 65535):
        self.batch = batch
        self.nodes = int(nodes)
        self.edges = batch.guided_default_edges(self.nodes) if edges is None else int(edges)
        self.cpuct = int(cpuct)
        self.max_plies = int(max_plies)
        self._check_cpuct(cpuct)
        if self.max_plies < 1:
            raise ValueError(f"max_plies must be >= 1 (got {max_plies})")
        n, h, w = batch.n, batch.height, batch.width
        self._open(batch.guided_moves_bytes(self.nodes, self.edges),     # (refuses Connect, generic boards, bad nodes or edges)
                   [("leaf_grid", (n, h, w), "int8"), ("leaf_player", (n,), "int8"), ("leaf_kind", (n,)), ("leaf_targets", (n, w), "int64"),
                    ("visits", (n, w, h * w)), ("scores", (n, w, h * w)), ("best", (n,)), ("nodes", (n,)), ("used", (n,))])

    def _scalars(self):
        return (self.nodes, self.edges, self.cpuct, min(self.max_plies, 2**31 - 1))

    def finish(self, priors, values):
        """Apply (priors, values) to the leaves of the previous call and select nothing (BGS_GUIDED_FINISH): every
        leaf_kind comes back GUIDED_IDLE, and visits, scores, best, nodes and used are final."""
        return self._call(_abi.GUIDED_FINISH, priors, values)

    def run(self, evaluate, simulations: int):
        """`begin`, `simulations` evaluations a tree, `finish`: evaluate(leaf_grid, leaf_player, leaf_targets) -> (priors
        float32[n, W, H * W], values float32[n]) is called once a simulation on the device tensors of the leaves (the first
        call sees the roots) and returns device tensors.  Returns what `finish` returns."""
        return self._run(evaluate, simulations)
