"""Diagnostic (CPU): the checked set of tests/test_sensitivity.py (items 1 and 2: the numpy checker's tangent, twice, on the N = 2 and N = 3
problems) written to tests/golden/sensitivity_checked_set.npz for the GPU suite, and the `key = value` lines of the CPU part of
profiles/sensitivity.txt (floor, bound, emulator discrepancy).  test_golden_checked_set_is_what_the_checker_computes recomputes the file.
Usage: python tests/sensitivity_profile.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.test_sensitivity import GOLDEN, checked_set, measured_lines, pack_rows      # noqa: E402

np.savez_compressed(GOLDEN, **pack_rows(checked_set()))
print("\n".join(measured_lines()))
