"""Diagnostic: the lines of profiles/newton_step.txt.  CPU part (always): per case of tests/test_newton_step.py the floor of the dense reference
(its own discrepancy between the difference steps 1e-3 and 2e-3), the bound 100 x floor and the discrepancies of the C oracle and of the kernel
text on the lane emulator.  GPU part (--gpu, on an MI355X): per shape and iteration cap of tests/test_gpu_newton_step.py the CPU floor (oracle
versus emulator) and the GPU's discrepancy against the emulator and the oracle, and the restoration phase's step.  The tests recompute every one
of these figures on every run and assert on them; this script only writes them down.
Usage: python tests/newton_step_profile.py [--gpu] > profiles/newton_step.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import test_gpu_newton_step as g      # noqa: E402
from tests import test_newton_step as c          # noqa: E402

print("# one Newton direction against the dense reference (tests/test_newton_step.py); all figures relative to max |dZ|")
print("\n".join(c.measured_lines()))
if "--gpu" in sys.argv[1:]:
    print("# K iterations from a far point, GPU against emulator / oracle (tests/test_gpu_newton_step.py); x relative to the step, nu to max |nu|")
    for name in g.SHAPES:
        s = g._handle(name)
        try:
            for K in g.KS:
                print(g.line_of(g.measure(name, K, s)))
        finally:
            s.close()
    Ks, rows = g.resto_rows()
    print(f"# restoration phase's step: set A, K* = {Ks}, {len(rows)} rows")
    for waves, nw in ((1, 1), (2, "pair"), (4, 4)):
        for K in (Ks, Ks + 1):
            print(g.resto_line_of(g.measure_resto(waves, nw, K)))
