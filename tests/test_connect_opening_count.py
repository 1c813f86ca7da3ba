"""The VALU count of the lock-step deferred opening in the built product library, read on the CPU
(tools/opening_valu_count.py; docs/EXPERIMENTS.md §40).

The bench kernel k_connect_rollout_opened_steps<Geo<1,6,7,4>, 3, true> is bound by VALU issue, and the opening is 43 % of
its vector instructions: 296 + 93 = 389 for the two straight-line blocks of open_games_deferred before §40, 360 after.
The ceiling of 365 is a guard against a later edit quietly putting instructions back -- a store that makes hipcc assemble
a register quad with v_mov_b32, a ply position that falls back to multiply, subtract, add -- not the measure of success:
that is the A/B on the GPU."""

import os
import sys

from tests.knobs import PRODUCT_LIB, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import opening_valu_count  # noqa: E402

CEILING = 365


def test_the_deferred_opening_stays_lean():
    name, copies = opening_valu_count.opening_blocks(PRODUCT_LIB)
    for k, (stage1, stage2) in enumerate(copies):
        print(f"{name}: opening copy {k}: {stage1} + {stage2} = {stage1 + stage2} VALU")
    stage1, stage2 = copies[0]
    assert stage1 + stage2 <= CEILING
