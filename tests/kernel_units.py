"""The kernel units of csrc/, for the CPU tests that check where a kernel lives: the ordered unit list (csrc/Makefile's
KERNEL_TUS, the index bgs_kernel_unit_id() takes), the ids `make print-unit-ids` gives, and which unit's object defines a
symbol.  A plain module, no fixtures."""

import os
import subprocess

from tests.conftest import PKG

CSRC = os.path.join(PKG, "csrc")
UNITS = ("connect", "bounce", "generic", "evaluate", "search", "solve")


def source(unit):
    return os.path.join(CSRC, f"{unit}_kernels.hip")


def kernel_files():
    """the *_kernels.hip of csrc/, sorted"""
    return sorted(name for name in os.listdir(CSRC) if name.endswith("_kernels.hip"))


def made_unit_ids(csrc=CSRC, *make_args):
    """{unit: id} as the sources under `csrc` would give them, in the Makefile's order"""
    out = subprocess.check_output(["make", "-s", "--no-print-directory", "-C", csrc, *make_args, "print-unit-ids"], text=True)
    return dict(line.split() for line in out.splitlines())


def check_six_distinct_ids(units=None):
    units = made_unit_ids() if units is None else units
    assert list(units) == list(UNITS)
    assert len(set(units.values())) == len(UNITS) and all(len(v) == 16 and int(v, 16) >= 0 for v in units.values())
    return units


def units_defining(symbol):
    """the units whose object file (csrc/<unit>_kernels.o, demangled) names `symbol`"""
    return [unit for unit in UNITS
            if symbol in subprocess.check_output(["nm", "-C", os.path.join(CSRC, f"{unit}_kernels.o")], text=True)]
