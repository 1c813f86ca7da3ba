"""What the five agents of simulator/agents.py share and no other test pins: the cache of batches a (Config, number of
states), `close()`, ended states in a list, and that `predict_many`, `choose_many` and the one-state wrappers speak of one
and the same launch.  The values themselves are compared with the CPU models elsewhere (tests/test_gpu_evaluate*.py,
test_gpu_search*.py, test_gpu_forest.py, test_gpu_bounce_forest.py, test_gpu_solve*.py); here an agent is compared with a
fresh agent, with its own other method, or with the batch call its docstring names.

This file was written against the agents as they were before their shared parts were pulled together and passed there
unedited; it is the record that the loader and the cache did not change what an agent answers.

The smallest shapes that reach the code: Connect 4 x 5 with runs of 3 (and 5 x 4 as the second Config), the smallest
Bounce grid of tests/test_gpu_parity.py (and its "small" one as the second Config), at most 6 states a list, 4 playouts a
move, 8 iterations of 4 playouts, the least halving budget the widest root takes, a solver horizon of 2.

Everything here needs a real MI355X: `pytest -m gpu`.
"""

import functools

import numpy as np
import pytest

from simulator.batch import SOLVE_LOSS, SOLVE_WIN
from tests.test_gpu_parity import BOUNCE_GRIDS

pytestmark = pytest.mark.gpu

SEED = 0x5EED5EED
FIRST = 5                     # first_game of the calls that take one
GAMES = ("connect", "bounce")


# ---- positions: a few random plies from the start, and one ended game
def walk(config, count, seed):
    rng = np.random.default_rng(seed)
    states = []
    while len(states) < count:
        s = config.sample_initial_state()
        for _ in range(int(rng.integers(1, 5))):
            acts = s.actions
            after = acts[int(rng.integers(len(acts)))].sample_next_state()
            if after.has_ended:
                break
            s = after
        states.append(s)
    return states


def ended_state(config):
    for seed in range(16):
        rng = np.random.default_rng(seed)
        s = config.sample_initial_state()
        for _ in range(128):
            if s.has_ended:
                return s
            acts = s.actions
            s = acts[int(rng.integers(len(acts)))].sample_next_state()
    raise AssertionError("no random game of 128 plies ended")


@functools.lru_cache(maxsize=None)
def positions(game):
    """{"six": 6 states, "three": 3 others, "other": 4 states of a second Config, "ended": an ended state of the first}"""
    if game == "connect":
        from simulator.game.connect import Config

        first, second = Config(4, 5, 3), Config(5, 4, 3)
    else:
        from simulator.game.bounce import Config

        smallest = min(BOUNCE_GRIDS.values(), key=lambda grid: grid.size)
        first, second = Config(smallest), Config(BOUNCE_GRIDS["small"])
    found = {"six": walk(first, 6, 1), "three": walk(first, 3, 2), "other": walk(second, 4, 3), "ended": ended_state(first)}
    assert found["ended"].has_ended and not found["ended"].actions
    assert all(s.actions for name in ("six", "three", "other") for s in found[name])
    return found


def halving_budget(game):
    """the least budget the widest root of `positions(game)` takes: moves * max(1, ceil(log2 moves)) (a Connect batch asks
    it of its width, a Bounce batch of a root's legal moves)"""
    found = positions(game)
    if game == "connect":
        widest = max(s.config.width for s in found["six"] + found["other"])
    else:
        widest = max(len(s.actions) for s in found["six"] + found["three"] + found["other"])
    return widest * max(1, (widest - 1).bit_length())


# ---- the agents: name -> (the games it takes, how to make one)
def makers():
    from simulator.agents import BounceHalvingAgent, BounceTreeSearchAgent, MonteCarloAgent, SolverAgent, TreeSearchAgent

    tree = dict(iterations=8, leaf_playouts=4, seed=SEED)
    return {
        "flat": (GAMES, lambda game: MonteCarloAgent(playouts=4, seed=SEED)),
        "flat-decisive": (GAMES, lambda game: MonteCarloAgent(playouts=4, seed=SEED, policy="decisive")),
        "halving": (("connect",), lambda game: MonteCarloAgent(playouts=4, seed=SEED, allocation="halving", budget=halving_budget(game))),
        "tree": (("connect",), lambda game: TreeSearchAgent(**tree)),
        "tree-prove": (("connect",), lambda game: TreeSearchAgent(prove=True, **tree)),
        "tree-reuse": (("connect",), lambda game: TreeSearchAgent(reuse=True, **tree)),
        "bounce-halving": (("bounce",), lambda game: BounceHalvingAgent(budget=halving_budget(game), seed=SEED)),
        "bounce-tree": (("bounce",), lambda game: BounceTreeSearchAgent(**tree)),
        "bounce-tree-prove": (("bounce",), lambda game: BounceTreeSearchAgent(prove=True, **tree)),
        "bounce-tree-reuse": (("bounce",), lambda game: BounceTreeSearchAgent(reuse=True, **tree)),
        "solver": (GAMES, lambda game: SolverAgent(depth=2)),
    }


# a reusing agent's answers depend on the searches before: it is left out of RUNS and has tests of its own
RUNS = [("flat", "connect"), ("flat", "bounce"), ("flat-decisive", "connect"), ("flat-decisive", "bounce"), ("halving", "connect"),
        ("tree", "connect"), ("tree-prove", "connect"), ("bounce-halving", "bounce"), ("bounce-tree", "bounce"),
        ("bounce-tree-prove", "bounce"), ("solver", "connect"), ("solver", "bounce")]
REUSING = [("tree-reuse", "connect"), ("bounce-tree-reuse", "bounce")]
IDS = [f"{name}-{game}" for name, game in RUNS]


def make(name, game):
    games, maker = makers()[name]
    assert game in games
    return maker(game)


def is_solver(agent):
    return not hasattr(agent, "choose_many")


def ask(agent, states):
    """everything `agent` says about `states`, as plain comparable values"""
    if is_solver(agent):
        codes, plies = agent.solve_many(states)
        return [agent.predict_many(states), codes.tolist(), plies.tolist()]
    said = [agent.predict_many(states, first_game=FIRST), agent.choose_many(states, first_game=FIRST)]
    if hasattr(agent, "search"):
        said += [a.tolist() for a in agent.search(states, first_game=FIRST)]
    return said


def flat_slot(state, action):
    """column for Connect; for Bounce the slot of MonteCarloAgent's docstring, s = x * height * width + ty * width + tx"""
    if hasattr(action, "column"):
        return action.column
    height, width = state.grid.shape
    (sx, _), (tx, ty) = action.source.tolist(), action.target.tolist()
    return sx * height * width + ty * width + tx


def row_index(state, action):
    """where `action` sits in a root's row of a per-move output: (column,), or (x, ty * width + tx)"""
    if hasattr(action, "column"):
        return (action.column,)
    (sx, _), (tx, ty) = action.source.tolist(), action.target.tolist()
    return (sx, ty * state.grid.shape[1] + tx)


# ---- the cache
@pytest.mark.parametrize("name,game", RUNS, ids=IDS)
def test_a_used_agent_answers_as_a_fresh_one_and_holds_a_batch_a_config_and_size(name, game):
    found = positions(game)
    agent = make(name, game)
    for step, states in enumerate((found["six"], found["three"], found["six"], found["other"])):
        fresh = make(name, game)
        got, want = ask(agent, states), ask(fresh, states)
        assert got == want, step
        assert list(got[0][0]) == states[0].actions and got[0][0]          # keyed by the state's actions, in their order
        assert len(fresh._batches) == 1
        fresh.close()
    assert len(agent._batches) == 3                                         # (first Config, 6), (first Config, 3), (second Config, 4)
    agent.close()


@pytest.mark.parametrize("name", ["flat", "solver"])
def test_one_agent_takes_both_games_in_turn(name):
    agent = make(name, "connect")
    for step, game in enumerate(("connect", "bounce", "connect", "bounce")):
        fresh = make(name, game)
        assert ask(agent, positions(game)["six"]) == ask(fresh, positions(game)["six"]), step
        fresh.close()
    assert len(agent._batches) == 2
    agent.close()


# ---- close()
@pytest.mark.parametrize("name,game", RUNS, ids=IDS)
def test_close_empties_the_cache_and_the_agent_works_again(name, game):
    states = positions(game)["six"]
    agent = make(name, game)
    before = ask(agent, states)
    assert len(agent._batches) == 1
    agent.close()
    assert agent._batches == {}
    assert ask(agent, states) == before
    assert len(agent._batches) == 1
    agent.close()
    agent.close()                         # closing twice is harmless
    assert agent._batches == {}


@pytest.mark.parametrize("name,game", REUSING, ids=[name for name, _ in REUSING])
def test_close_drops_the_forests_and_the_next_search_is_search_0_of_a_new_one(name, game):
    states = positions(game)["six"]
    agent = make(name, game)
    first = [a.tolist() for a in agent.search(states, first_game=FIRST)]
    second = [a.tolist() for a in agent.search(states, first_game=FIRST)]
    assert len(first) == (5 if game == "connect" else 6)                   # ..., carried
    # the second search went on in the first's trees: it started with the nodes the first left and added to the root's visits
    assert not np.any(first[-1]) and second[-1] == first[3]
    assert np.sum(second[1]) > np.sum(first[1])
    (entry,) = agent._forests.values()
    assert entry[-1] == 2 and len(agent._batches) == 1                     # searches so far
    agent.close()
    assert agent._forests == {} and agent._batches == {}
    again = [a.tolist() for a in agent.search(states, first_game=FIRST)]
    assert again == first                                                  # seed + 0, nothing carried
    (entry,) = agent._forests.values()
    assert entry[-1] == 1
    # what a fresh reusing agent says, and what the shares of a reusing agent are: of the root's visits, carried ones included
    fresh = make(name, game)
    assert [a.tolist() for a in fresh.search(states, first_game=FIRST)] == first
    fresh.close()
    shares = agent.predict_many(states, first_game=FIRST)                  # search 1 of the new forest
    (entry,) = agent._forests.values()
    assert entry[-1] == 2
    visits = np.array(second[1])
    for k, s in enumerate(states):
        assert shares[k] == {a: float(visits[k][row_index(s, a)]) / int(visits[k].sum()) for a in s.actions}
    agent.close()


# ---- ended states
@pytest.mark.parametrize("name,game", RUNS + REUSING, ids=IDS + [name for name, _ in REUSING])
def test_an_ended_state_has_no_action_and_no_values(name, game):
    found = positions(game)
    states = [found["six"][0], found["ended"], found["six"][1]]
    agent = make(name, game)
    values = agent.predict_many(states) if is_solver(agent) else agent.predict_many(states, first_game=FIRST)
    assert values[1] == {} and list(values[0]) == states[0].actions and list(values[2]) == states[2].actions
    if is_solver(agent):
        assert agent.choose(found["ended"]) is None and agent.predict(found["ended"]) == {}
        assert agent.choose(states[0]) in states[0].actions
    else:
        chosen = agent.choose_many(states, first_game=FIRST)
        assert chosen[1] is None and chosen[0] in states[0].actions and chosen[2] in states[2].actions
        assert agent.choose(found["ended"], game=FIRST + 1) is None and agent.predict(found["ended"], game=FIRST + 1) == {}
    agent.close()


# ---- one launch for both methods, and the one-state wrappers
@pytest.mark.parametrize("name,game", [run for run in RUNS if run[0] in ("flat", "flat-decisive")], ids=lambda x: x)
def test_flat_choice_is_the_first_best_valued_action(name, game):
    states = positions(game)["six"]
    agent = make(name, game)
    values = agent.predict_many(states, first_game=FIRST)
    chosen = agent.choose_many(states, first_game=FIRST)
    for s, v, c in zip(states, values, chosen):
        best = max(v.values())
        assert c == next(a for a in s.actions if v[a] == best)
        assert all(type(x) is float and 0.0 <= x <= 1.0 for x in v.values())
    agent.close()


def test_connect_halving_choice_is_the_survivor_of_the_same_launch():
    states = positions("connect")["six"]
    agent = make("halving", "connect")
    values = agent.predict_many(states, first_game=FIRST)
    chosen = agent.choose_many(states, first_game=FIRST)
    (batch,) = agent._batches.values()                                     # it still holds the states
    v, best = agent.halving_values(batch, FIRST)
    for k, s in enumerate(states):
        assert chosen[k] == s.action_at(int(best[k]))
        assert values[k] == {a: float(v[k, a.column]) for a in s.actions}
    agent.close()


def test_bounce_halving_choice_is_the_survivor_of_the_same_launch():
    from simulator.agents import BOUNCE_MAX_PLIES

    states = positions("bounce")["six"]
    agent = make("bounce-halving", "bounce")
    values = agent.predict_many(states, first_game=FIRST)
    chosen = agent.choose_many(states, first_game=FIRST)
    (batch,) = agent._batches.values()
    counts, given, best = batch.evaluate_moves_halving(seed=SEED, budget=agent.budget, max_plies=BOUNCE_MAX_PLIES, policy="uniform")
    for k, s in enumerate(states):
        assert flat_slot(s, chosen[k]) == best[k] and chosen[k] in s.actions
        for a in s.actions:
            at = (k,) + row_index(s, a)
            assert values[k][a] == (float((counts[at][0] + 0.5 * counts[at][1]) / given[at]) if given[at] else 0.0)
    agent.close()


@pytest.mark.parametrize("name,game", [run for run in RUNS if "tree" in run[0]], ids=lambda x: x)
def test_tree_shares_and_choice_are_of_the_launch_search_returns(name, game):
    states = positions(game)["six"]
    agent = make(name, game)
    out = agent.search(states, first_game=FIRST)
    shares = agent.predict_many(states, first_game=FIRST)
    chosen = agent.choose_many(states, first_game=FIRST)
    assert len(out) == {"tree": 4, "tree-prove": 6, "bounce-tree": 5, "bounce-tree-prove": 7}[name]
    visits, best = out[1], out[2]
    for k, s in enumerate(states):
        assert flat_slot(s, chosen[k]) == best[k] and chosen[k] in s.actions
        assert abs(sum(shares[k].values()) - 1.0) < 1e-12
        if not agent.prove:
            assert shares[k] == {a: float(visits[k][row_index(s, a)]) / (8 * 4) for a in s.actions}
            assert shares[k][chosen[k]] == max(shares[k].values())          # the most visited
        else:
            proved = out[-2]
            assert proved.shape == visits.shape
            codes = {a: int(proved[k][row_index(s, a)]) for a in s.actions}
            assert SOLVE_WIN == 1 and SOLVE_LOSS == -1
            if 1 in codes.values():                                          # a proved win takes everything, and is chosen
                assert codes[chosen[k]] == 1
                assert all((v > 0) == (codes[a] == 1) for a, v in shares[k].items())
            elif any(c != -1 for c in codes.values()):                       # moves proved lost get nothing, and are not chosen
                assert codes[chosen[k]] != -1
                assert all(v == 0.0 for a, v in shares[k].items() if codes[a] == -1)
    agent.close()


@pytest.mark.parametrize("name,game", RUNS, ids=IDS)
def test_the_one_state_wrappers_are_the_list_calls_of_one_state(name, game):
    states = positions(game)["six"]
    agent = make(name, game)
    if is_solver(agent):
        many = agent.predict_many(states)
        for k in (0, 3, 5):
            assert agent.predict(states[k]) == many[k]
            assert agent.choose(states[k]) in states[k].actions
    else:
        many, chosen = agent.predict_many(states, first_game=0), agent.choose_many(states, first_game=0)
        for k in (0, 3, 5):
            assert agent.predict(states[k], game=k) == many[k] == agent.predict_many([states[k]], first_game=k)[0]
            assert agent.choose(states[k], game=k) == chosen[k]
        assert len(agent._batches) == 2                                      # 6 states, 1 state
    agent.close()
