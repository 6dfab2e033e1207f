"""The reference's own open list, grid neighbourhood, RNG and Modulo for the tests: live from oracle/_ref/libppref.so, built
(oracle/Makefile `ref`) from the reference's utils/frontier.h, utils/grid.cpp, utils/random.h, utils/maths.h where its sources
are present, or else what that library returned for exactly the inputs below, stored in tests/golden/reference_utils.npz
(tests/golden/make_reference_utils_vectors.py writes it; tests/test_oracle_ref.py checks it whenever the library is built)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import oracle_lib as O

REF_SO = os.path.join(O.ORACLE_DIR, "_ref", "libppref.so")
if not os.path.exists(REF_SO) and os.path.isdir("/root/reference/planner/src"):
    subprocess.call(["make", "-C", O.ORACLE_DIR, "ref"])
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_utils.npz")

NEIGHBOR_GRIDS = ((5, 7), (1, 1), (2, 2), (3, 1))
RNG_SEEDS = (0, 1, 12345, 2**63 + 5)
RNG_BOUNDS = ((0.0, 1.0), (-51.2, 51.2))
RNG_DRAWS = 1000
# StateSpaceSE2::SampleUniform / SampleGaussian draws (tests/test_pyplanning_surface.py)
SE2_SEED, SE2_DRAWS = 2024, 500
SE2_LB, SE2_UB = np.array([-51.2, -20.0, -np.pi]), np.array([51.2, 30.0, np.pi])
SE2_MEAN, SE2_STD = np.array([1.0, -2.0, 0.3]), np.array([40.0, 0.5, 2.5])


def _random_ops(rng, n, levels):
    costs = rng.randint(0, levels, size=n).astype(np.float64) / 4.0
    ops, pushed, inq = [], 0, 0
    while pushed < n or inq > 0:
        if pushed < n and (inq == 0 or rng.rand() < 0.55):
            ops.append(pushed)
            pushed += 1
            inq += 1
        else:
            ops.append(-1)
            inq -= 1
    return np.array(ops, dtype=np.int32), costs


def frontier_cases():
    rng = np.random.RandomState(7)
    return [_random_ops(rng, 300, levels=3 + trial % 9) for trial in range(40)]


def neighbor_cases():
    return [(r, c, rows, cols) for rows, cols in NEIGHBOR_GRIDS for r in range(-1, rows + 1) for c in range(-1, cols + 1)]


def modulo_values():
    return np.random.RandomState(3).uniform(-20, 20, 200)


class LiveReference:
    """The reference's functions, called in oracle/_ref/libppref.so."""

    def __init__(self, path):
        L = C.CDLL(path)
        L.ref_modulo.restype = C.c_double
        L.ref_modulo.argtypes = [C.c_double, C.c_double]
        L.ref_rng_uniform.argtypes = [C.c_ulonglong, C.c_longlong, C.c_double, C.c_double, C.POINTER(C.c_double)]
        L.ref_rng_se2.argtypes = [C.c_ulonglong, C.c_longlong] + [C.POINTER(C.c_double)] * 6
        self.L = L

    def frontier_pops(self, case, ops, costs):
        popped = np.empty(len(ops), dtype=np.int32)
        n = self.L.ref_frontier_replay(C.c_int(len(ops)), O.iptr(ops), O.dptr(costs), O.iptr(popped))
        return popped[:n]

    def neighbors(self, case, r, c, rows, cols):
        n = C.c_int()
        rc = np.empty((8, 2), dtype=np.int32)
        self.L.ref_neighbors(C.c_int(r), C.c_int(c), C.c_int(rows), C.c_int(cols), C.byref(n), O.iptr(rc))
        return rc[:n.value]

    def rng_uniform(self, case, seed, n, lb, ub):
        out = np.empty(n)
        self.L.ref_rng_uniform(C.c_ulonglong(seed), C.c_longlong(n), C.c_double(lb), C.c_double(ub), O.dptr(out))
        return out

    def modulo(self, case, v, m):
        return self.L.ref_modulo(float(v), m)

    def rng_se2(self, seed, n, lb, ub, mean, std):
        """(uniform [n, 3], gaussian [n, 3] before the clamp to the bounds) from the reference's global mt19937_64"""
        uni, gau = np.empty((n, 3)), np.empty((n, 3))
        self.L.ref_rng_se2(C.c_ulonglong(seed), C.c_longlong(n), O.dptr(lb), O.dptr(ub), O.dptr(mean), O.dptr(std), O.dptr(uni), O.dptr(gau))
        return uni, gau


class RecordedReference:
    """The same answers, as the library returned them for the inputs of this module (tests/golden/reference_utils.npz).  Every call
    also checks that the inputs it is asked about are the recorded ones."""

    def __init__(self, path):
        self.z = np.load(path)

    def _split(self, key, i):
        off = self.z[key + "_offsets"]
        return self.z[key][off[i]:off[i + 1]]

    def frontier_pops(self, case, ops, costs):
        assert np.array_equal(self._split("frontier_ops", case), ops) and np.array_equal(self._split("frontier_costs", case), costs)
        return self._split("frontier_popped", case)

    def neighbors(self, case, r, c, rows, cols):
        assert tuple(self.z["neighbor_cases"][case]) == (r, c, rows, cols)
        return self._split("neighbor_rc", case).reshape(-1, 2)

    def rng_uniform(self, case, seed, n, lb, ub):
        assert self.z["rng_seeds"][case] == np.uint64(seed) and tuple(self.z["rng_bounds"][case]) == (lb, ub)
        return self.z["rng_uniform"][case][:n]

    def modulo(self, case, v, m):
        assert self.z["modulo_in"][case] == v and m == 2 * math.pi
        return float(self.z["modulo_out"][case])

    def rng_se2(self, seed, n, lb, ub, mean, std):
        assert (seed, n) == (SE2_SEED, SE2_DRAWS)
        assert all(np.array_equal(a, b) for a, b in ((lb, SE2_LB), (ub, SE2_UB), (mean, SE2_MEAN), (std, SE2_STD)))
        return self.z["se2_uniform"], self.z["se2_gaussian"]


def reference():
    """the live library where it is built, its recorded answers otherwise"""
    return LiveReference(REF_SO) if os.path.exists(REF_SO) else RecordedReference(GOLDEN)
