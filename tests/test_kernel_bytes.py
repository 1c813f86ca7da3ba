"""tools/kernel_bytes.py on the two libraries of the tree.  csrc/Makefile links libbgs.so and libbgs_test.so with the SAME
kernel objects (the TEST build compiles the host-side units alone once more), so every kernel of one is in the other with
the same machine code and the same descriptor figures: the tool finds nothing but identical kernels, and finds the
kernels named on its command line.  CPU only: the tool reads the code objects with the ROCm tree's binutils."""

import os
import re
import subprocess
import sys

from tests.conftest import PRODUCT_LIB, ROOT, TEST_LIB

TOOL = os.path.join(ROOT, "tools", "kernel_bytes.py")
# a kernel of each analysis unit, and one of the scan kernels that two units hold under one name
NAMES = ("k_connect_evaluate_halving", "k_bounce_search", "k_connect_solve", "k_bounce_eval_scan_totals")


def _run(*args):
    return subprocess.run([sys.executable, TOOL, PRODUCT_LIB, TEST_LIB, *args], capture_output=True, text=True)


def test_the_test_library_holds_the_product_librarys_kernels_byte_for_byte():
    res = _run(*[arg for name in NAMES for arg in ("--find", name)])
    assert res.returncode == 0, res.stdout + res.stderr
    groups = dict(re.findall(r"^(identical|differ|only in A|only in B): (\d+)$", res.stdout, re.M))
    assert int(groups["identical"]) > 100 and (groups["differ"], groups["only in A"], groups["only in B"]) == ("0", "0", "0")
    assert "not found" not in res.stdout
    # a name that two units hold (anonymous namespaces) is listed once a copy
    assert len(re.findall(r"^  \S*k_bounce_eval_scan_totals\S*  ", res.stdout, re.M)) == 2


def test_a_kernel_name_that_is_not_there_fails_the_run():
    res = _run("--quiet", "--find", "k_no_such_kernel")
    assert res.returncode == 1 and "not found in A: k_no_such_kernel" in res.stdout and "not found in B: k_no_such_kernel" in res.stdout
