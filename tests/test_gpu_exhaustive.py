"""Every kernel family against the oracle on every position of small game trees (tests/game_trees.py), bit for bit.

The boards are written into batches with write_state.  On every position set:
  a. every move: each position replicated once per column, plus -1 (skip) and W (out of range); full columns and ended
     boards are among them (Bounce: once per legal move, plus the skip and illegal moves) -- step_actions;
  b. the move lists: legal / action_count (Bounce: targets, targets_tensor, action_count);
  c. the exports of a policy step: step_actions_observe and env_step (auto-reset) on the running positions' moves, with
     an even and an odd batch size (the one-word fused kernel needs an even n);
  d. one ply through the rollout kernels (R replicas of each running position, capped at its ply count + 1, with the
     coverage of (position, legal move) pairs the draws reached asserted) and an uncapped rollout from every position,
     under the default plan and under each forced family that accepts loaded boards;
  e. the object API: transition, 64 boards a call and one board a call, with transition_wave on and off (Bounce:
     also on the generic kernels);
  f. flat Monte-Carlo: evaluate_actions / evaluate_moves with P = 1 and P = 7, one of them at a first game id >= 2^32;
  g. the decisive playout policy: evaluate_actions / evaluate_moves with policy="decisive", P = 2, uncapped (Bounce: 4096
     plies), twice, one of the runs at a first game id >= 2^32, against tests/policy_expected.py and
     tests/bounce_policy_expected.py.

Position sets (positions; moves of check a = positions x (W + 2) for Connect):
  Connect full trees: 2x3 k2 45, 3x3 k3 694, 3x4 k3 7 157, 4x3 k3 2 715, 4x4 k3 41 750, 4x4 k4 161 029.
  Connect depth-limited walks (every position up to the depth) plus an end-game set (the last 3 positions of 3000 oracle
  games, distinct boards):
    6x7 k4 (the bench geometry) to depth 6: 22 100 + end games; 8x8 k4 and 8x8 k5 (one word, beyond 48 cells) to depth 5:
    9 673 each + end games; 6x12 k4 (two words) to depth 4: 9 025 + end games; 12x13 k5 (the compile-time multi-word
    kernel, registers and LDS) to depth 4: 11 987 + end games; 4x20 k3 (generic) to depth 3: 5 001 + end games.
  Bounce full graphs: narrow 2, blocked_start 1, three_next_to_goal 1 476; small to depth 6: 11 267; the default 9x6
  board to depth 3: 9 670.
Check f runs on every position of the full Connect trees up to 4x4 k3 and on a fixed sample elsewhere (it replicates
each root W x P times, H x W x W x P for Bounce).  Check g runs on every position of the full Connect trees while
positions x W x P stays under 60 000 boards (2x3 k2, 3x3 k3, 4x3 k3, 3x4 k3) and on a fixed sample of 2000 elsewhere --
1000 on 8x8 k5 and 6x12 k4, 300 on 12x13 k5, where the CPU reference's long games set the size; Bounce: up to 1024
positions, 128 of the default board.  Generic Connect boards (4x20) refuse env_step's auto-reset and
evaluate_actions by design: there the tests assert the refusal.  The counts are printed (pytest -s).
"""

import functools

import numpy as np
import pytest

from oracle import oracle
from tests import game_trees as gt
from tests.bounce_policy_expected import bounce_policy_expected
from tests.knobs import knobs
from tests.mc_expected import connect_expected
from tests.policy_expected import connect_policy_expected
from tests.test_gpu_evaluate_bounce import expected as bounce_expected
from tests.test_gpu_parity import DEFAULT_BOUNCE, assert_bounce_actions, assert_same
from tests.test_spec_exhaustive import BOUNCE_CONFIGS

pytestmark = pytest.mark.gpu

SEED = 0x0E7A0577E5EED123
BIG_GAME = (1 << 32) + 5       # a first game id above 2^32

CONNECT_FULL = [(2, 3, 2), (3, 3, 3), (3, 4, 3), (4, 3, 3), (4, 4, 3), (4, 4, 4)]
CONNECT_FULL_TOTALS = {(2, 3, 2): 45, (3, 3, 3): 694, (3, 4, 3): 7157, (4, 3, 3): 2715, (4, 4, 3): 41750, (4, 4, 4): 161029}
CONNECT_DEEP = {(6, 7, 4): 6, (8, 8, 4): 5, (8, 8, 5): 5, (6, 12, 4): 4, (12, 13, 5): 4, (4, 20, 3): 3}
END_GAMES = 3000
BOUNCE_WALKS = {"narrow": (None, 2), "blocked_start": (None, 1), "three_next_to_goal": (None, 1476), "small": (6, 11267),
                "default": (3, 9670)}

# forced families that accept loaded boards ({} = the default plan); "per_ply" = the strict RNG contract
CONNECT_FAMILIES = {"default": {}, "rollout_generic": {"rollout_generic": "1"}, "force_generic": {"force_generic": "1"},
                    "per_ply": {}}
BOUNCE_FAMILIES = {"default": {}, "flat": {"bounce_group": "1", "bounce_pieces": "0"},
                   "group8": {"bounce_group": "8"}, "no_wave_pass": {"bounce_wave_pass": "0"}, "force_generic": {"force_generic": "1"}}
BOUNCE_CAP = 4096   # Bounce has games that never end


@pytest.fixture(scope="module")
def bm():
    from simulator import batch

    return batch


class forced:
    """BGS_EXPERIMENT settings for the batches created inside the block"""

    def __init__(self, settings):
        self.settings = settings

    def __enter__(self):
        self.old = {k: knobs.get(k) for k in self.settings}
        knobs.update(self.settings)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                del knobs[k]
            else:
                knobs[k] = v


def take(layer, idx):
    return tuple(a[idx].copy() for a in layer)


def concat(layers):
    return tuple(np.concatenate([l[j] for l in layers]) for j in range(4))


@functools.lru_cache(maxsize=None)
def connect_positions(h, w, k):
    if (h, w, k) in CONNECT_FULL_TOTALS:
        pos = concat([layer for _, layer in gt.connect_layers(h, w, k)])
        assert pos[0].shape[0] == CONNECT_FULL_TOTALS[(h, w, k)]
        return pos
    walk = concat([layer for _, layer in gt.connect_layers(h, w, k, max_depth=CONNECT_DEEP[(h, w, k)])])
    ends = gt.end_games(h, w, k, END_GAMES, SEED ^ h ^ (w << 8))
    return concat([walk, ends])


@functools.lru_cache(maxsize=None)
def bounce_positions(name):
    cfg = DEFAULT_BOUNCE if name == "default" else np.array(BOUNCE_CONFIGS[name], dtype=np.int8)
    max_depth, total = BOUNCE_WALKS[name]
    layers, acts = [], []
    for _, layer, a in gt.bounce_layers(cfg, max_depth=max_depth):
        layers.append(layer)
        acts += a
    pos = concat(layers)
    assert pos[0].shape[0] == total
    return cfg, pos, acts


def connect_oracle(h, w, k, layer, per_ply=False):
    o = oracle.ConnectOracle(h, w, k, layer[0].shape[0], per_ply=per_ply)
    o.grid[:], o.player[:], o.winner[:], o.plies[:] = layer
    return o


def bounce_oracle(cfg, layer):
    o = oracle.BounceOracle(cfg, layer[0].shape[0])
    o.grid[:], o.player[:], o.winner[:], o.plies[:] = layer
    return o


def loaded(dev, layer):
    assert (dev.write_state(*layer) == 0).all()
    dev.reset_steps()
    return dev


def sample(n, m, seed):
    return np.arange(n) if n <= m else np.sort(np.random.default_rng(seed).choice(n, m, replace=False))


def geom_id(g):
    return "x".join(map(str, g))


# ------------------------------------------------------------------------------------------------ Connect

ALL_CONNECT = CONNECT_FULL + list(CONNECT_DEEP)


@pytest.mark.parametrize("geom", ALL_CONNECT, ids=geom_id)
def test_connect_every_move_and_move_list(bm, geom):
    """a + b: every position x every column (and -1, W) through step_actions; legal and action_count of the loaded boards"""
    h, w, k = geom
    pos = connect_positions(h, w, k)
    cols = np.arange(-1, w + 1, dtype=np.int32)
    m = len(cols)
    rep = tuple(np.repeat(a, m, axis=0) for a in pos)
    dev = loaded(bm.ConnectBatch(h, w, k, rep[0].shape[0]), rep)
    orc = connect_oracle(h, w, k, rep)
    assert_same(dev, orc, f"{geom} loaded")
    np.testing.assert_array_equal(dev.legal, orc.legal(), err_msg=f"{geom} legal")
    np.testing.assert_array_equal(dev.action_count, orc.legal().sum(axis=1), err_msg=f"{geom} action_count")
    actions = np.tile(cols, pos[0].shape[0])
    want = orc.step_actions(actions)
    np.testing.assert_array_equal(dev.step_actions(actions), want, err_msg=f"{geom} status")
    assert_same(dev, orc, f"{geom} after every move")
    assert dev.steps == int(((want == 0) & (actions >= 0)).sum())
    assert (want == -2).any()
    print(f"Connect {geom}: {pos[0].shape[0]} positions, {actions.size} moves, {int((want == -2).sum())} refused")
    dev.close()


@pytest.mark.parametrize("geom", ALL_CONNECT, ids=geom_id)
def test_connect_policy_step_exports(bm, geom):
    """c: step_actions_observe and env_step (auto-reset) on every column of every running position, n even and odd"""
    import torch

    h, w, k = geom
    pos = connect_positions(h, w, k)
    run = take(pos, np.flatnonzero(pos[2] == -1))
    cols = np.arange(0, w + 1, dtype=np.int32)
    rep = tuple(np.repeat(a, len(cols), axis=0) for a in run)
    actions = np.tile(cols, run[0].shape[0])
    even = rep[0].shape[0] & ~1
    for n in (even, even - 1):
        part = take(rep, np.arange(n))
        d_act = torch.from_numpy(actions[:n].copy()).cuda()
        what = f"{geom} n={n}"
        # step_actions_observe
        dev = loaded(bm.ConnectBatch(h, w, k, n, use_torch=True), part)
        orc = connect_oracle(h, w, k, part)
        ended = torch.zeros(n, dtype=torch.uint8, device="cuda")
        status = torch.zeros(n, dtype=torch.int32, device="cuda")
        obs = dev.step_actions_observe(d_act, ended=ended, status=status)
        want = orc.step_actions(actions[:n])
        np.testing.assert_array_equal(status.cpu().numpy(), want, err_msg=f"{what} observe status")
        np.testing.assert_array_equal(obs.cpu().numpy(), orc.legal(), err_msg=f"{what} observe legal")
        np.testing.assert_array_equal(ended.cpu().numpy().astype(bool), orc.ended, err_msg=f"{what} observe ended")
        assert_same(dev, orc, f"{what} observe")
        # env_step, finished boards restarted in the same call (bit-packed boards only: refused on generic ones)
        dev = loaded(dev, part)
        reward = torch.zeros((n, 2), dtype=torch.int8, device="cuda")
        if dev.generic:
            with pytest.raises(ValueError, match="BGS_ENV_AUTO_RESET needs a bit-packed board"):
                dev.env_step(d_act, ended=ended, reward=reward, status=status)
            assert_same(dev, connect_oracle(h, w, k, part), f"{what} refused env_step leaves the boards")
            dev.close()
            continue
        obs = dev.env_step(d_act, ended=ended, reward=reward, status=status)
        np.testing.assert_array_equal(status.cpu().numpy(), want, err_msg=f"{what} env status")
        np.testing.assert_array_equal(ended.cpu().numpy().astype(bool), orc.ended, err_msg=f"{what} env ended")
        np.testing.assert_array_equal(reward.cpu().numpy(), orc.reward, err_msg=f"{what} env reward")
        done = orc.ended.copy()
        orc.grid[done], orc.player[done], orc.winner[done], orc.plies[done] = -1, 0, -1, 0
        assert_same(dev, orc, f"{what} env restarted")
        np.testing.assert_array_equal(obs.cpu().numpy(), orc.legal(), err_msg=f"{what} env legal")
        assert done.any()
        dev.close()


def connect_one_ply(bm, geom, pos, family, per_ply):
    """R replicas of each running position (a sample of 2048 per ply count), rollout capped at ply + 1; returns the
    fraction of (position, legal column) pairs some replica drew"""
    h, w, k = geom
    R = 8 * w
    covered = pairs = 0
    run = take(pos, np.flatnonzero(pos[2] == -1))
    for d in np.unique(run[3]):
        layer = take(run, np.flatnonzero(run[3] == d))
        layer = take(layer, sample(layer[0].shape[0], 2048, int(d)))
        rep = tuple(np.repeat(a, R, axis=0) for a in layer)
        dev = loaded(bm.ConnectBatch(h, w, k, rep[0].shape[0]), rep)
        if per_ply:
            dev.set_rng_contract("per-ply")
        dev.set_first_game(BIG_GAME)
        orc = connect_oracle(h, w, k, rep, per_ply)
        dev.rollout(SEED, max_plies=int(d) + 1)
        total = orc.rollout(SEED, first_game=BIG_GAME, max_plies=int(d) + 1)
        assert_same(dev, orc, f"{geom} {family} one ply from ply {d}")
        assert dev.steps == total == rep[0].shape[0]
        drawn = (orc.grid != rep[0]).any(axis=1).reshape(-1, R, w)   # the column each replica dropped in
        legal = connect_oracle(h, w, k, layer).legal().astype(bool)
        covered += int((drawn.any(axis=1) & legal).sum())
        pairs += int(legal.sum())
        dev.close()
    return covered / pairs


@pytest.mark.parametrize("family", list(CONNECT_FAMILIES))
@pytest.mark.parametrize("geom", ALL_CONNECT, ids=geom_id)
def test_connect_rollouts_from_every_position(bm, geom, family):
    """d: one ply (coverage asserted) and to the end from every position, under each kernel family"""
    h, w, k = geom
    pos = connect_positions(h, w, k)
    per_ply = family == "per_ply"
    settings = [dict(CONNECT_FAMILIES[family])]
    if geom == (12, 13, 5) and family == "default":
        settings.append({"rollout_no_lds": "1"})
    for s in settings:
        with forced(s):
            coverage = connect_one_ply(bm, geom, pos, family, per_ply)
            assert coverage > 0.99, f"{geom} {family}: only {coverage:.4f} of the moves were drawn"
            dev = loaded(bm.ConnectBatch(h, w, k, pos[0].shape[0]), pos)
            if per_ply:
                dev.set_rng_contract("per-ply")
            dev.set_first_game(7)
            orc = connect_oracle(h, w, k, pos, per_ply)
            dev.rollout(SEED ^ 1)
            total = orc.rollout(SEED ^ 1, first_game=7)
            assert_same(dev, orc, f"{geom} {family} {s} to the end")
            assert dev.steps == total and orc.ended.all()
            print(f"Connect {geom} {family} {s}: one-ply coverage {coverage:.4f}, {pos[0].shape[0]} rollouts")
            dev.close()


@pytest.mark.parametrize("wave", ["1", "0"])
@pytest.mark.parametrize("geom", ALL_CONNECT, ids=geom_id)
def test_connect_transition_on_a_sample(bm, geom, wave):
    """e: the object API's round trip, 64 boards a call, 16 calls over a sample of the positions"""
    h, w, k = geom
    pos = connect_positions(h, w, k)
    rng = np.random.default_rng(h * 97 + w)
    idx = sample(pos[0].shape[0], 64 * 16, h + w + k)
    with forced({} if wave == "1" else {"transition_wave": "0"}):
        for c in range(0, len(idx), 64):
            part = take(pos, idx[c : c + 64])
            n = part[0].shape[0]
            dev = bm.ConnectBatch(h, w, k, n)
            cols = rng.integers(-1, w + 1, size=n).astype(np.int32)
            status, grid, player, winner, plies, legal, reward = dev.transition(*part, actions=cols)
            orc = connect_oracle(h, w, k, part)
            np.testing.assert_array_equal(status, orc.step_actions(cols))
            for got, want in ((grid, orc.grid), (player, orc.player), (winner, orc.winner), (plies, orc.plies),
                              (legal, orc.legal()), (reward, orc.reward)):
                np.testing.assert_array_equal(got, want, err_msg=f"{geom} transition_wave={wave} call {c // 64}")
            dev.close()


@pytest.mark.parametrize("geom", ALL_CONNECT, ids=geom_id)
def test_connect_evaluate_on_every_position(bm, geom):
    """f: flat Monte-Carlo counts and env-steps, P = 1 and 7 (P = 7 at a first game above 2^32)"""
    h, w, k = geom
    pos = connect_positions(h, w, k)
    full = geom in CONNECT_FULL and pos[0].shape[0] <= 50000
    roots = pos if full else take(pos, sample(pos[0].shape[0], 6000, w))
    for playouts, first in ((1, 3), (7, BIG_GAME)):
        b = loaded(bm.ConnectBatch(h, w, k, roots[0].shape[0]), roots)
        b.set_first_game(first)
        if b.generic:   # bit-packed boards only: a generic geometry is refused, not served by a fall-back
            with pytest.raises(ValueError, match="bit-packed Connect boards only"):
                b.evaluate_actions(seed=SEED, playouts=playouts)
            b.close()
            continue
        got = b.evaluate_actions(seed=SEED, playouts=playouts)
        want, steps = connect_expected(h, w, k, roots, SEED, first, playouts, 2**31 - 1, False)
        np.testing.assert_array_equal(got, want, err_msg=f"{geom} P={playouts}")
        assert b.steps == steps
        b.close()


# the roots of check g where the tree is not walked in full: 2000, fewer where the games are long (the lock-step reference
# costs about 26 us a playout ply; both runs of a geometry together stay under about 10 s on the host)
DECISIVE_BOARDS = 60_000
DECISIVE_SAMPLE = {(8, 8, 5): 1000, (6, 12, 4): 1000, (12, 13, 5): 300}


@pytest.mark.parametrize("geom", ALL_CONNECT, ids=geom_id)
def test_connect_decisive_evaluate_on_every_position(bm, geom):
    """g: the decisive policy's counts and env-steps, P = 2, uncapped, one of the two runs at a first game above 2^32"""
    h, w, k = geom
    pos = connect_positions(h, w, k)
    playouts = 2
    full = geom in CONNECT_FULL and pos[0].shape[0] * w * playouts <= DECISIVE_BOARDS
    roots = pos if full else take(pos, sample(pos[0].shape[0], DECISIVE_SAMPLE.get(geom, 2000), w))
    for first in (3, BIG_GAME):
        b = loaded(bm.ConnectBatch(h, w, k, roots[0].shape[0]), roots)
        b.set_first_game(first)
        if b.generic:   # bit-packed boards only: a generic geometry is refused, not served by a fall-back
            with pytest.raises(ValueError, match="bit-packed Connect boards only"):
                b.evaluate_actions(seed=SEED, playouts=playouts, policy="decisive")
            b.close()
            continue
        got = b.evaluate_actions(seed=SEED, playouts=playouts, policy="decisive")
        want, steps, seen = connect_policy_expected(h, w, k, roots, SEED, first, playouts, 2**31 - 1, False)
        np.testing.assert_array_equal(got, want, err_msg=f"{geom} decisive first game {first}")
        assert b.steps == steps
        print(f"Connect {geom} decisive: {roots[0].shape[0]} roots{' (every position)' if full else ''}, {steps} env-steps, plies {seen}")
        b.close()


# ------------------------------------------------------------------------------------------------ Bounce


def bounce_moves(cfg, pos, acts):
    """(board index, move) for every legal move of every position, the skip, and illegal moves"""
    h, w = cfg.shape
    out = []
    for i, a in enumerate(acts):
        out += [(i, (sx, sy, tx, ty)) for (sx, sy), (tx, ty) in a]
        row = a[0][0][1] if a else 1
        out += [(i, (-1, 0, 0, 0)), (i, (0, 0, 0, 1)), (i, (0, row, w, row)), (i, (0, row, 0, row)), (i, (w - 1, row, 0, h - 1)),
                (i, (w, row, 0, row))]
    idx = np.array([i for i, _ in out], dtype=np.int64)
    return idx, np.array([m for _, m in out], dtype=np.int32).reshape(-1, 4)


@pytest.mark.parametrize("name", list(BOUNCE_WALKS))
def test_bounce_every_move_and_move_list(bm, name):
    """a + b: every legal move of every position and illegal ones through step_actions; targets, targets_tensor and
    action_count of the loaded boards"""
    cfg, pos, acts = bounce_positions(name)
    dev = loaded(bm.BounceBatch(cfg, pos[0].shape[0], use_torch=True), pos)
    orc = bounce_oracle(cfg, pos)
    assert_same(dev, orc, f"{name} loaded")
    np.testing.assert_array_equal(dev.action_count, orc.count_actions())
    assert [len(a) for a in acts] == orc.count_actions().tolist()
    assert_bounce_actions(dev, orc, range(pos[0].shape[0]))
    np.testing.assert_array_equal(dev.targets_tensor().cpu().numpy().view(np.uint64), dev.targets)
    dev.close()
    idx, moves = bounce_moves(cfg, pos, acts)
    rep = take(pos, idx)
    dev = loaded(bm.BounceBatch(cfg, idx.size), rep)
    orc = bounce_oracle(cfg, rep)
    want = orc.step_actions(moves)
    np.testing.assert_array_equal(dev.step_actions(moves), want, err_msg=f"{name} status")
    assert_same(dev, orc, f"{name} after every move")
    assert dev.steps == int(((want == 0) & (moves[:, 0] >= 0)).sum())
    print(f"Bounce {name}: {pos[0].shape[0]} positions, {idx.size} moves, {int((want == -2).sum())} refused")
    dev.close()


@pytest.mark.parametrize("name", list(BOUNCE_WALKS))
def test_bounce_policy_step_exports(bm, name):
    """c: step_actions_observe and env_step (auto-reset) on every legal move of every position, n even and odd"""
    import torch

    cfg, pos, acts = bounce_positions(name)
    idx, moves = bounce_moves(cfg, pos, acts)
    keep = moves[:, 0] >= 0
    idx, moves = idx[keep], moves[keep]
    if idx.size < 2:
        pytest.skip(f"{name}: {idx.size} move")   # blocked_start: settled at reset, nothing to play
    rep = take(pos, idx)
    h, w = cfg.shape
    even = idx.size & ~1
    for n in (even, even - 1):
        part = take(rep, np.arange(n))
        d_mv = torch.from_numpy(moves[:n].copy()).cuda()
        what = f"{name} n={n}"
        dev = loaded(bm.BounceBatch(cfg, n, use_torch=True), part)
        orc = bounce_oracle(cfg, part)
        ended = torch.zeros(n, dtype=torch.uint8, device="cuda")
        status = torch.zeros(n, dtype=torch.int32, device="cuda")
        obs = dev.step_actions_observe(d_mv, ended=ended, status=status)
        want = orc.step_actions(moves[:n])
        np.testing.assert_array_equal(status.cpu().numpy(), want, err_msg=f"{what} observe status")
        np.testing.assert_array_equal(ended.cpu().numpy().astype(bool), orc.ended, err_msg=f"{what} observe ended")
        assert_same(dev, orc, f"{what} observe")
        np.testing.assert_array_equal(obs.cpu().numpy().view(np.uint64), dev.targets, err_msg=f"{what} observe targets")
        assert_bounce_actions(dev, orc, range(0, n, max(1, n // 512)))
        dev = loaded(dev, part)
        reward = torch.zeros((n, 2), dtype=torch.int8, device="cuda")
        obs = dev.env_step(d_mv, ended=ended, reward=reward, status=status)
        np.testing.assert_array_equal(status.cpu().numpy(), want, err_msg=f"{what} env status")
        np.testing.assert_array_equal(ended.cpu().numpy().astype(bool), orc.ended, err_msg=f"{what} env ended")
        np.testing.assert_array_equal(reward.cpu().numpy(), orc.reward, err_msg=f"{what} env reward")
        done = orc.ended.copy()
        start = oracle.BounceOracle(cfg, 1)
        orc.grid[done], orc.player[done], orc.winner[done], orc.plies[done] = start.grid[0], 0, start.winner[0], 0
        assert_same(dev, orc, f"{what} env restarted")
        np.testing.assert_array_equal(obs.cpu().numpy().view(np.uint64), dev.targets, err_msg=f"{what} env targets")
        dev.close()


@pytest.mark.parametrize("family", list(BOUNCE_FAMILIES))
@pytest.mark.parametrize("name", list(BOUNCE_WALKS))
def test_bounce_rollouts_from_every_position(bm, name, family):
    """d: one ply from R replicas of each running position (coverage asserted) and to the end from every position"""
    cfg, pos, acts = bounce_positions(name)
    with forced(BOUNCE_FAMILIES[family]):
        run = np.flatnonzero(pos[2] == -1)
        covered = pairs = 0
        for d in np.unique(pos[3][run]):
            sel = run[pos[3][run] == d]
            sel = sel[sample(sel.size, 1024, int(d))]
            layer = take(pos, sel)
            R = max(16, 6 * max(len(acts[i]) for i in sel))
            rep = tuple(np.repeat(a, R, axis=0) for a in layer)
            dev = loaded(bm.BounceBatch(cfg, rep[0].shape[0]), rep)
            dev.set_first_game(BIG_GAME)
            orc = bounce_oracle(cfg, rep)
            dev.rollout(SEED, max_plies=int(d) + 1)
            total = orc.rollout(SEED, first_game=BIG_GAME, max_plies=int(d) + 1)
            assert_same(dev, orc, f"{name} {family} one ply from ply {d}")
            assert dev.steps == total == rep[0].shape[0]
            kids = orc.grid.reshape(len(sel), R, -1)
            for j, i in enumerate(sel):
                seen = {kids[j, r].tobytes() for r in range(R)}
                pairs += len(acts[i])
                covered += len(seen)   # distinct moves give distinct boards
            dev.close()
        if pairs:
            assert covered / pairs > 0.97, f"{name} {family}: only {covered}/{pairs} moves drawn"
        dev = loaded(bm.BounceBatch(cfg, pos[0].shape[0]), pos)
        dev.set_first_game(11)
        orc = bounce_oracle(cfg, pos)
        dev.rollout(SEED ^ 3, max_plies=BOUNCE_CAP)
        total = orc.rollout(SEED ^ 3, first_game=11, max_plies=BOUNCE_CAP)
        assert_same(dev, orc, f"{name} {family} to the end")
        assert dev.steps == total
        print(f"Bounce {name} {family}: one-ply coverage {covered}/{pairs}, {pos[0].shape[0]} rollouts")
        dev.close()


@pytest.mark.parametrize("mode", ["wave", "thread", "generic"])
@pytest.mark.parametrize("name", list(BOUNCE_WALKS))
def test_bounce_transition_on_a_sample(bm, name, mode):
    """e: transition, 64 boards a call (fewer for the tiny graphs) and 16 one-board calls (the one-wave kernel), legal and
    illegal moves; with transition_wave=0, and on the generic kernels (force_generic: wide legal records, decoded)"""
    cfg, pos, acts = bounce_positions(name)
    idx, moves = bounce_moves(cfg, pos, acts)
    pick = sample(idx.size, 64 * 16, len(name))
    calls = [pick[c : c + 64] for c in range(0, pick.size, 64)] + [pick[j : j + 1] for j in range(min(16, pick.size))]
    settings = {"wave": {}, "thread": {"transition_wave": "0"}, "generic": {"force_generic": "1"}}[mode]
    with forced(settings):
        for c, sel in enumerate(calls):
            part = take(pos, idx[sel])
            dev = bm.BounceBatch(cfg, sel.size)
            assert dev.generic == (mode == "generic")
            status, grid, player, winner, plies, masks, reward = dev.transition(*part, actions=moves[sel])
            orc = bounce_oracle(cfg, part)
            np.testing.assert_array_equal(status, orc.step_actions(moves[sel]))
            what = f"{name} {mode} call {c} ({sel.size} boards)"
            for got, want in ((grid, orc.grid), (player, orc.player), (winner, orc.winner), (plies, orc.plies),
                              (reward, orc.reward)):
                np.testing.assert_array_equal(got, want, err_msg=what)
            for i in range(sel.size):
                assert list(dev.decode_moves(masks[i], int(winner[i]))) == orc.actions(i), f"{what} board {i}"
            if mode != "generic":
                np.testing.assert_array_equal(masks, dev.targets, err_msg=what)
                assert_bounce_actions(dev, orc, range(sel.size))
            dev.close()


@pytest.mark.parametrize("name", list(BOUNCE_WALKS))
def test_bounce_evaluate_on_the_positions(bm, name):
    """f: evaluate_moves counts and env-steps, P = 1 and 7 (P = 7 at a first game above 2^32), on up to 256 positions"""
    cfg, pos, acts = bounce_positions(name)
    roots = take(pos, sample(pos[0].shape[0], 256 if name == "default" else 1024, 5))
    for playouts, first in ((1, 0), (7, BIG_GAME)):
        b = loaded(bm.BounceBatch(cfg, roots[0].shape[0]), roots)
        b.set_first_game(first)
        got = b.evaluate_moves(seed=SEED, playouts=playouts, max_plies=BOUNCE_CAP)
        want, steps = bounce_expected(cfg, roots, SEED, first, playouts, BOUNCE_CAP)
        np.testing.assert_array_equal(got, want, err_msg=f"{name} P={playouts}")
        assert b.steps == steps
        b.close()


@pytest.mark.parametrize("name", list(BOUNCE_WALKS))
def test_bounce_decisive_evaluate_on_the_positions(bm, name):
    """g: the decisive policy's counts and env-steps, P = 2, one of the two runs at a first game above 2^32, on up to 1024
    positions (128 of the default board, whose games are long)"""
    cfg, pos, acts = bounce_positions(name)
    roots = take(pos, sample(pos[0].shape[0], 128 if name == "default" else 1024, 5))
    for first in (0, BIG_GAME):
        b = loaded(bm.BounceBatch(cfg, roots[0].shape[0]), roots)
        b.set_first_game(first)
        got = b.evaluate_moves(seed=SEED, playouts=2, max_plies=BOUNCE_CAP, policy="decisive")
        want, steps, seen = bounce_policy_expected(cfg, roots, SEED, first, 2, BOUNCE_CAP)
        np.testing.assert_array_equal(got, want, err_msg=f"{name} decisive first game {first}")
        assert b.steps == steps
        print(f"Bounce {name} decisive: {roots[0].shape[0]} roots, {steps} env-steps, plies {seen}")
        b.close()
