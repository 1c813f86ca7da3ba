"""Rate of the exact Connect solver (bgs_connect_solve_actions) on 6x7 connect-4 end-games.

Workload: for every n of --n, n positions of random oracle games (uniform policy from the start) at E empty cells, still running, distinct
boards; every column of every board solved in full (depth 42) under a budget no task is meant to reach.  Reports, per E,
positions (board, column tasks) per second, nodes per second, ms per launch (device events, median of --reps launches
after one warm-up), budget hits and the codes' histogram.  Writes JSON to --out.

    python tools/solve_rate.py --n 16384 65536 --empties 10 12 14 --out profiles/solve_rate.json

The kernel trace and counters of a launch are kept apart, in profiles/solve_rate_profile.json, with the commands that
took them.
"""

import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "board-game-simulator-python_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def positions(n, empty, seed, games):
    from oracle import oracle

    h, w, k = 6, 7, 4
    orc = oracle.ConnectOracle(h, w, k, games)
    for _ in range(h * w - empty):
        orc.step_random(seed)
    keep = np.flatnonzero(orc.winner == -1)
    grid = orc.grid[keep]
    key = np.ascontiguousarray(grid.reshape(len(keep), -1)).view(f"V{h * w}").ravel()
    _, first = np.unique(key, return_index=True)
    pick = keep[np.sort(first)][:n]
    return orc.grid[pick], orc.player[pick], orc.winner[pick], orc.plies[pick]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1 << 14])
    ap.add_argument("--empties", type=int, nargs="+", default=[10, 14, 18])
    ap.add_argument("--max-nodes", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--games", type=int, default=None, help="oracle games the positions are drawn from (default 16 n)")
    ap.add_argument("--seed", type=int, default=0x501E)
    ap.add_argument("--max-seconds", type=float, default=20.0, help="skip the remaining reps of an E whose launch took longer")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from simulator.batch import ConnectBatch
    from simulator.game import _abi

    lib = _abi.lib()
    rows = []
    for want, empty in [(n_, e) for n_ in args.n for e in args.empties]:
        g, p, wn, pl = positions(want, empty, args.seed ^ empty, args.games or 16 * want)
        n = g.shape[0]
        b = ConnectBatch(6, 7, 4, n, use_torch=True)
        assert (b.write_state(g, p, wn, pl) == 0).all()
        codes = torch.empty((n, 7), dtype=torch.int8, device="cuda:0")
        plies = torch.empty((n, 7), dtype=torch.int16, device="cuda:0")
        nodes = torch.zeros(2, dtype=torch.int64, device="cuda:0")

        def launch():
            _abi.check(lib.bgs_connect_solve_actions(b._handle, 42, args.max_nodes, ctypes.c_void_p(codes.data_ptr()),
                                                     ctypes.c_void_p(plies.data_ptr()), ctypes.c_void_p(nodes.data_ptr()), 1))

        t0 = time.time()
        launch()
        torch.cuda.synchronize()
        first = time.time() - t0
        times = []
        for _ in range(args.reps if first < args.max_seconds else 0):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        ms = float(np.median(times)) if times else first * 1e3
        c = codes.cpu().numpy()
        tasks = int((c != -2).sum())
        visited = int(nodes[0].item())
        hist = {int(v): int(m) for v, m in zip(*np.unique(c, return_counts=True))}
        row = {"empty": empty, "boards": n, "tasks": tasks, "ms_per_launch": round(ms, 3), "launch_ms_all": [round(t, 3) for t in times],
               "first_launch_s": round(first, 3), "nodes": visited, "nodes_per_task": round(visited / max(tasks, 1), 1),
               "positions_per_s": tasks / (ms / 1e3), "nodes_per_s": visited / (ms / 1e3),
               "budget_hits": hist.get(3, 0), "codes": hist}
        print(json.dumps(row), flush=True)
        rows.append(row)
        b.close()
    out = {"tool": "tools/solve_rate.py", "arguments": {k: v for k, v in vars(args).items() if k != "out"}, "geometry": [6, 7, 4], "depth": 42, "max_nodes": args.max_nodes, "device": torch.cuda.get_device_name(0),
           "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
