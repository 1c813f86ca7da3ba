"""bgs_connect_guided_advance over the Connect keys of tests/guided_fuzz_cases.py -- random geometries, start grids and
roots, capacities from 2 to 33, every cpuct --: three moves a key of search, advance and step, with advance columns drawn
uniformly over [-1, width] from numpy.random.default_rng(ADVANCE_BASE + key), so that most of them meet no subtree; every
call's outputs, `kept` and the whole trees after every `finish` and every `advance` equal the CPU statement's
(tests/guided_advance_expected.py), bit for bit.  BGS_FUZZ_CASES=N widens the keys to 0 .. N - 1, as in the other fuzz
modules.  The statement's side is computed once a session.

Everything here needs a real MI355X: `pytest -m gpu`.
"""

import functools

import numpy as np
import pytest

from tests import guided_advance_expected as ga
from tests import guided_expected as ge
from tests import guided_fuzz_cases as gf
from tests import test_gpu_guided as tc
from tests import test_gpu_guided_advance as ta

pytestmark = pytest.mark.gpu

ADVANCE_BASE = 83000        # default_rng(base + key): a base of this module's own
MOVES, SIMULATIONS = 3, 24


@functools.lru_cache(maxsize=None)
def expected(key):
    case = gf.connect_key(key)
    rng = np.random.default_rng(ADVANCE_BASE + key)
    n = case.roots[0].shape[0]

    def columns_of(model, move):
        return rng.integers(-1, case.w + 1, n).astype(np.int32), ["random"] * n

    return ga.play(case.h, case.w, case.k, case.roots, case.capacity, SIMULATIONS, MOVES, cpuct=case.cpuct, columns_of=columns_of)


@pytest.mark.parametrize("key", gf.connect_keys())
def test_connect_key_equals_the_statement(key):
    case = gf.connect_key(key)
    model, script = expected(key)
    b = tc.load(case.h, case.w, case.k, case.roots)
    guided = ta.forest(b, case.capacity, case.cpuct)
    ta.replay(b, guided, script, ge.fake_network, f"key {key}")
    print(f"connect key {key}: {case.h}x{case.w}x{case.k}, C = {case.capacity}, cpuct = {case.cpuct}, columns "
          f"{[move.columns.tolist() for move in script]}, kept {[move.kept.tolist() for move in script]}")
    guided.close()
    b.close()
