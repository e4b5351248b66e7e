#!/usr/bin/env python3
"""The exhaustive sweep behind the recorded bound of tanh32 (include/rex.h): every fp32 in [0, 10] -- tanh32 is exactly
odd -- through the host twin (tests/host_harness/actor_host.cpp, g++ -ffp-contract=off) against fp64 tanh, in ulp of the result.

    python profiles/actor_tanh_sweep.py [processes]

About 70 CPU-seconds in all.  tests/test_actor_host.py re-runs the slice around the worst case.
"""
import ctypes
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


def run(r):
    from host_harness import actor as host
    where = ctypes.c_float()
    worst = host.lib().actor_host_tanh_sweep(r[0], r[1], ctypes.byref(where))
    return worst, where.value


if __name__ == "__main__":
    from host_harness import actor as host
    host.lib()                                   # built once, before the workers load it
    top = int(np.float32(10.0).view(np.uint32))
    edges = np.linspace(0, top + 1, 65).astype(np.int64)
    ranges = [(int(edges[k]), int(edges[k + 1] - 1)) for k in range(64)]
    with ProcessPoolExecutor(int(sys.argv[1]) if len(sys.argv) > 1 else 4) as ex:
        worst = max(ex.map(run, ranges))
    print("tanh32: worst %.6f ulp at x = %r over %d values" % (worst[0], worst[1], top + 1))
