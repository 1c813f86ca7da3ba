#!/usr/bin/env python3
"""The exact Bounce solver (bgs_bounce_solve_moves) on one GPU against what a user builds without it.

Default 9x6 board, distinct running mid-game roots (10 uniformly random plies from the start):
  * solve     -- for 2^12 and 2^14 roots and depths 1-5, budget 2^40 (no hits): a warm-up, then three launches timed by
                 events on the batch's stream with the codes and plies left on the device; the median in ms a launch,
                 positions (roots) a second, tasks (legal moves), nodes a second, nodes a task, budget hits;
  * composed  -- the same answers from calls the library had before the solver: `targets` of the roots, every legal move
                 played on a replicated batch (write_state + step_actions), `targets` of the running children, ... level by
                 level to the horizon, winners read back, the negamax reduced in numpy.  Depths 2 and 3, end to end, both
                 sides alike (host arrays in and out, batches created, loaded and closed inside the timed region, a
                 warm-up, the median of three), against `solve_moves` on the same roots.  The composition holds
                 every position of the tree at once, so depth 3 runs on the first 2^10 roots only (about 5 x 10^6 boards
                 at its last level).  Its codes and plies must equal the solver's: `answers_equal`.

    python tools/solve_bounce_rate.py [--out FILE] [--kernel-only] [--depths 1,2,3,4,5]
Prints one JSON object (and writes it to --out)."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "board-game-simulator-python_amd")]
import numpy as np
import torch

from simulator.batch import SOLVE_BUDGET, SOLVE_DRAW, SOLVE_LOSS, SOLVE_NONE, SOLVE_UNKNOWN, SOLVE_WIN, BounceBatch
from simulator.game import _abi

GRID = np.zeros((9, 6), dtype=np.int8)
GRID[1] = GRID[7] = [1, 2, 3, 3, 2, 1]
H, W = GRID.shape
S = W * H * W
NO_BUDGET = 1 << 40
COMPOSED = [(2, 1 << 12), (3, 1 << 10)]   # (depth, roots)


def roots(n, seed=0x0123456789ABCDEF):
    """n distinct running positions after 10 random plies: (grid, player, winner, plies)"""
    b = BounceBatch(GRID, 3 * n)
    b.step_random(seed=seed, plies=10)
    pos = (b.grid, b.player, b.winner, b.plies)
    b.close()
    key = np.concatenate([pos[0].reshape(3 * n, -1).view(np.uint8), pos[1].reshape(-1, 1).view(np.uint8)], axis=1)
    _, first = np.unique(np.ascontiguousarray(key).view(f"V{key.shape[1]}").ravel(), return_index=True)
    keep = np.sort(first[pos[2][first] == -1])[:n]
    assert keep.size == n, "too few distinct running roots"
    return tuple(a[keep].copy() for a in pos)


def load(pos, use_torch=None):
    b = BounceBatch(GRID, pos[0].shape[0], use_torch=use_torch)
    assert (b.write_state(*pos) == 0).all()
    return b


def solve_case(pos, depth):
    n = pos[0].shape[0]
    b = load(pos, use_torch=True)
    codes = torch.empty((n, W, H * W), dtype=torch.int8, device="cuda:0")
    plies = torch.empty((n, W, H * W), dtype=torch.int16, device="cuda:0")
    nodes = torch.zeros(1, dtype=torch.int64, device="cuda:0")

    def launch():
        _abi.check(_abi.lib().bgs_bounce_solve_moves(b._handle, depth, NO_BUDGET, ctypes.c_void_p(codes.data_ptr()),
                                                     ctypes.c_void_p(plies.data_ptr()), ctypes.c_void_p(nodes.data_ptr()), 1))

    launch()   # (warm-up)
    torch.cuda.synchronize()
    times = []
    for _ in range(3):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        launch()
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end))
    ms = float(np.median(times))
    c = codes.cpu().numpy()
    tasks = int((c != SOLVE_NONE).sum())
    visited = int(nodes[0])
    b.close()
    return {"roots": n, "depth": depth, "tasks": tasks, "device_ms": [round(t, 4) for t in times], "device_ms_median": round(ms, 4),
            "positions_per_s": n / (ms * 1e-3), "nodes": visited, "nodes_per_s": visited / (ms * 1e-3),
            "nodes_per_task": round(visited / tasks, 2), "budget_hits": int((c == SOLVE_BUDGET).sum()),
            "codes": {name: int((c == v).sum()) for name, v in (("win", SOLVE_WIN), ("loss", SOLVE_LOSS), ("draw", SOLVE_DRAW),
                                                                 ("unknown", SOLVE_UNKNOWN))}}


def expand(pos):
    """every legal move of the running positions `pos` played on a replicated batch: (parent index, slot, children)"""
    b = load(pos)
    t = b.targets
    b.close()
    s = np.arange(S)
    x, c = s // (H * W), s % (H * W)
    legal = ((t[:, x] >> c.astype(np.uint64)) & np.uint64(1)) != 0          # [m, S]
    parent, slot = np.nonzero(legal)
    moves = np.stack([x[slot], t[parent, W].astype(np.int64), c[slot] % W, c[slot] // W], -1).astype(np.int32)
    kid = load(tuple(a[parent] for a in pos))
    assert (kid.step_actions(moves) == 0).all()
    kids = (kid.grid, kid.player, kid.winner, kid.plies)
    kid.close()
    return parent, slot, kids


def composed(pos, depth):
    """(codes, plies) of solve_moves(depth) from targets / write_state / step_actions and a reduction in numpy"""
    n = pos[0].shape[0]
    levels, layer, boards = [], pos, 0
    for d in range(depth):
        parent, slot, kids = expand(layer)
        boards += parent.size
        mover = layer[1][parent]
        key = np.where(kids[2] == mover, 999, 0).astype(np.int64)   # a win in one: 1000 - 1
        go = np.flatnonzero(kids[2] == -1)
        levels.append((layer[0].shape[0], parent, slot, key, go, kids[2] == 2))
        layer = tuple(a[go] for a in kids)
        if go.size == 0:
            break
    below = None   # per position of the level below: the best key of the side to move there
    for d in range(len(levels) - 1, -1, -1):
        m, parent, slot, key, go, drawn = levels[d]
        if below is not None and go.size:
            key[go] = np.where(below > 0, 1 - below, np.where(below < 0, -below - 1, 0))
        if d == 0:
            break
        start = np.searchsorted(parent, np.arange(m))   # every running position has a move, parents ascend
        below = np.maximum.reduceat(key, start)
    m, parent, slot, key, go, drawn = levels[0]
    codes = np.full((n, S), SOLVE_NONE, dtype=np.int8)
    plies = np.zeros((n, S), dtype=np.int16)
    codes[parent, slot] = np.where(key > 0, SOLVE_WIN, np.where(key < 0, SOLVE_LOSS, np.where(drawn, SOLVE_DRAW, SOLVE_UNKNOWN)))
    plies[parent, slot] = np.where(key > 0, 1000 - key, np.where(key < 0, 1000 + key, np.where(drawn, 1, 0)))
    return codes.reshape(n, W, H * W), plies.reshape(n, W, H * W), boards


def composed_case(pos, depth):
    """both sides the same way: host arrays in (the roots are loaded inside the timed region), host arrays out, batches
    created and closed inside it; a warm-up, then the median of three"""
    def solver():
        b = load(pos)
        out = b.solve_moves(depth=depth, max_nodes=NO_BUDGET)
        b.close()
        return out

    def timed(fn):
        fn()   # (warm-up)
        times, out = [], None
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            times.append(time.perf_counter() - t0)
        return float(np.median(times)), out

    composed_s, (cc, cp, boards) = timed(lambda: composed(pos, depth))
    solve_s, (codes, plies) = timed(solver)
    return {"roots": pos[0].shape[0], "depth": depth, "composed_boards_materialised": int(boards),
            "composed_end_to_end_ms": round(composed_s * 1e3, 1), "solve_end_to_end_ms": round(solve_s * 1e3, 3),
            "composed_over_solve": round(composed_s / solve_s, 1),
            "answers_equal": bool(np.array_equal(codes, cc) and np.array_equal(plies, cp))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--depths", default="1,2,3,4,5")
    ap.add_argument("--roots", default="4096,16384")
    args = ap.parse_args()
    depths = [int(d) for d in args.depths.split(",")]
    sizes = [int(n) for n in args.roots.split(",")]
    big = roots(max(sizes + [n for _, n in COMPOSED]))
    res = {"tool": "tools/solve_bounce_rate.py", "device": torch.cuda.get_device_name(0), "build_id": _abi.build_id(),
           "unit_ids": {**_abi.unit_ids(), **_abi.extra_unit_ids()}, "board": "9x6 default", "root_plies": 10,
           "solve": [solve_case(tuple(a[:n] for a in big), d) for n in sizes for d in depths]}
    if not args.kernel_only:
        res["composed"] = [composed_case(tuple(a[:n] for a in big), d) for d, n in COMPOSED]
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    if not args.kernel_only and not all(c["answers_equal"] for c in res["composed"]):
        sys.exit("the composed answers differ from the solver's")


if __name__ == "__main__":
    main()
