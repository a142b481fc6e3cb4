"""(GPU box) run pbf_selftest_math and pbf_selftest_divides of the library named by PBF_HIP_LIB (or the default) and print
the mismatch and visited counts.  Usage: selftest_lib.py [numerators per divisor, default 8] [--fp64]"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

import bench  # noqa: E402

pkg = bench.load_package()
args = [a for a in sys.argv[1:] if a != "--fp64"]
s = pkg.Solver(h=0.1, fp64="--fp64" in sys.argv)
bad = np.zeros(4, np.uint64)
s._chk(s.L.pbf_selftest_math(s.ctx, bad.ctypes.data_as(C.c_void_p)), "pbf_selftest_math")
print("mismatches [sqrt, (h-r)^2/r, x/poly6(0.3h), x/RHO]:", bad.tolist())
bad, seen = s.selftest_divides(int(args[0]) if args else 8)
names = ["sqrt", "(h-r)^2/r", "x/poly6(0.3h)", "x/RHO", "field a/d", "field a/d, tiny a, guarded", "radial/r",
         "field a/d, tiny a, div_ranged alone"]
for k, name in enumerate(names):
    print(f"[{k}] {name}: {int(bad[k])} mismatches of {int(seen[k])} visited")
