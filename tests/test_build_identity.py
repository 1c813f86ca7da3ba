"""The build identity (bgs_build_id) belongs to what was COMPILED: a changed compile flag rebuilds every object without a
`make clean`, and the id the library reports is folded from the ids its kernel objects were compiled with.  CPU only
(hipcc cross-compiles gfx950); three full builds and several partial ones of the library in a scratch copy of csrc/, about six minutes on 8 cores."""

import ctypes
import os
import shutil
import subprocess
import sys

from tests import kernel_units

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "board-game-simulator-python_amd")

OBJECTS = ["bgs_capi", "bgs_host", "bgs_multi", "bgs_pipeline"] + [f"{unit}_kernels" for unit in kernel_units.UNITS]


def _ids(lib_path):
    """(build id, the six kernel units' ids in kernel_units.UNITS order) of a library file, read in a child process."""
    code = (
        "import ctypes, sys; l = ctypes.CDLL(sys.argv[1]); l.bgs_build_id.restype = ctypes.c_char_p; "
        "l.bgs_kernel_unit_id.restype = ctypes.c_char_p; l.bgs_kernel_unit_id.argtypes = [ctypes.c_int]; "
        "print(l.bgs_build_id().decode(), *[l.bgs_kernel_unit_id(i).decode() for i in range(6)])"
    )
    out = subprocess.check_output([sys.executable, "-c", code, lib_path], text=True).split()
    return out[0], out[1:]


def _make(csrc, *args):
    return subprocess.run(["make", "-C", csrc, "-j8", *args], check=True, capture_output=True, text=True).stdout


def _print_id(csrc, *args):
    return subprocess.check_output(["make", "-s", "--no-print-directory", "-C", csrc, "print-id", *args], text=True).strip()


def test_a_changed_flag_rebuilds_every_object_and_changes_the_id(tmp_path):
    csrc = tmp_path / "pkg" / "csrc"
    shutil.copytree(os.path.join(PKG, "csrc"), csrc, ignore=shutil.ignore_patterns("*.o", "flags.stamp", ".pytest_cache"))
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")
    csrc = str(csrc)
    lib = str(tmp_path / "pkg" / "libbgs.so")

    _make(csrc)
    first, first_units = _ids(lib)
    assert len(first) == 16 and first != "unknown" and first == _print_id(csrc)
    assert len(set(first_units)) == 6 and all(len(u) == 16 for u in first_units)
    stamps = {o: os.stat(os.path.join(csrc, o + ".o")).st_mtime_ns for o in OBJECTS}

    # nothing changed: nothing is compiled
    assert "hipcc" not in _make(csrc)
    assert {o: os.stat(os.path.join(csrc, o + ".o")).st_mtime_ns for o in OBJECTS} == stamps

    # a flag changes, no `make clean`: EVERY object is compiled again, and the library says so
    extra = "EXTRA_CXXFLAGS=-DBGS_BUILD_IDENTITY_TEST=1"
    out = _make(csrc, extra)
    for o in OBJECTS:
        assert os.stat(os.path.join(csrc, o + ".o")).st_mtime_ns > stamps[o], f"{o}.o was not rebuilt:\n{out}"
    second, second_units = _ids(lib)
    assert second != first and second == _print_id(csrc, extra)
    assert all(a != b for a, b in zip(first_units, second_units))

    # back to the default flags: again everything, and the first id comes back (the id is a function of source + flags)
    _make(csrc)
    assert _ids(lib) == (first, first_units)

    # one kernel source changes: its unit's id and the library's change, the other units keep theirs
    with open(os.path.join(csrc, "bounce_kernels.hip"), "a") as fh:
        fh.write("\n// build identity test\n")
    _make(csrc)
    third, third_units = _ids(lib)
    assert third not in (first, second) and third == _print_id(csrc)
    assert third_units[0] == first_units[0] and third_units[2] == first_units[2] and third_units[1] != first_units[1]

    # ... and so does an edit to that unit's own header (its geometry record and launch tuning), while the host-side
    # plumbing header every unit includes (bgs_internal.h: the batch object, prototypes) moves no id at all: counters
    # under profiles/ are gated per unit (bench.py), a Bounce-only round must not invalidate the Connect counters
    with open(os.path.join(csrc, "bounce_unit.h"), "a") as fh:
        fh.write("\n// build identity test\n")
    with open(os.path.join(csrc, "bgs_internal.h"), "a") as fh:
        fh.write("\n// build identity test\n")
    _make(csrc)
    fourth, fourth_units = _ids(lib)
    assert fourth_units[0] == first_units[0] and fourth_units[2] == first_units[2]
    assert fourth_units[1] not in (first_units[1], third_units[1])
    assert [kernel_units.made_unit_ids(csrc)[unit] for unit in kernel_units.UNITS] == fourth_units

    # the board headers several units share (connect_board.h: the Connect unit and, through playout.h, the evaluate,
    # search and solve units; bounce_board.h: the Bounce unit and the same three) move the ids of the units that
    # include them, and no other
    with open(os.path.join(csrc, "connect_board.h"), "a") as fh:
        fh.write("\n// build identity test\n")
    _make(csrc)
    fifth, fifth_units = _ids(lib)
    assert fifth not in (first, second, third, fourth) and fifth == _print_id(csrc)
    assert all(fifth_units[k] != fourth_units[k] for k in (0, 3, 4, 5))
    assert fifth_units[1] == fourth_units[1] and fifth_units[2] == fourth_units[2]

    with open(os.path.join(csrc, "bounce_board.h"), "a") as fh:
        fh.write("\n// build identity test\n")
    _make(csrc)
    sixth, sixth_units = _ids(lib)
    assert sixth not in (first, second, third, fourth, fifth) and sixth == _print_id(csrc)
    assert all(sixth_units[k] != fifth_units[k] for k in (1, 3, 4, 5))
    assert sixth_units[0] == fifth_units[0] and sixth_units[2] == fifth_units[2]

    # the solve unit's own source (the cheapest unit to rebuild) moves its id and the library's, and no other unit's
    with open(os.path.join(csrc, "solve_kernels.hip"), "a") as fh:
        fh.write("\n// build identity test\n")
    _make(csrc)
    seventh, seventh_units = _ids(lib)
    assert seventh not in (first, second, third, fourth, fifth, sixth) and seventh == _print_id(csrc)
    assert seventh_units[5] != sixth_units[5] and seventh_units[:5] == sixth_units[:5]

    # what the evaluate, search and solve units share (playout.h) moves those three and none of the first three
    with open(os.path.join(csrc, "playout.h"), "a") as fh:
        fh.write("\n// build identity test\n")
    _make(csrc)
    eighth, eighth_units = _ids(lib)
    assert eighth not in (first, second, third, fourth, fifth, sixth, seventh) and eighth == _print_id(csrc)
    assert all(eighth_units[k] != seventh_units[k] for k in (3, 4, 5)) and eighth_units[:3] == seventh_units[:3]

    # ... and the first Bounce pass of the evaluation and the solver (bounce_root_moves.h) those two, not the search unit
    # (the ids the sources would give: nothing is compiled for this step)
    with open(os.path.join(csrc, "bounce_root_moves.h"), "a") as fh:
        fh.write("\n// build identity test\n")
    ninth_units = [kernel_units.made_unit_ids(csrc)[unit] for unit in kernel_units.UNITS]
    assert ninth_units[3] != eighth_units[3] and ninth_units[5] != eighth_units[5]
    assert ninth_units[:3] == eighth_units[:3] and ninth_units[4] == eighth_units[4]


def test_the_library_in_the_tree_is_the_one_its_sources_give():
    """What __graft_entry__.build() enforces: the loaded library's id equals `make print-id` of the tree."""
    lib = os.path.join(PKG, "libbgs.so")
    assert os.path.exists(lib), "build the library first (python __graft_entry__.py)"
    handle = ctypes.CDLL(lib)
    handle.bgs_build_id.restype = ctypes.c_char_p
    assert handle.bgs_build_id().decode() == _print_id(os.path.join(PKG, "csrc"))
