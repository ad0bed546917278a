"""Host-side launch shape of the training march, queried through the C ABI without a GPU: mi3d_march_train_plan reports
what mi3d_march_rays_train launches (csrc/raymarching.hip march_train_plan, the one function both call).  The rays per
wave start at 64 and are halved while N > 64, more than 16 are left and ceil(N / rays per wave) < 1024; at most 4096
single-wave workgroups are launched, and a wave walks batches w, w + 4096, ...  tests/test_march_variants_gpu.py asserts
from this query which variant each of its ray counts runs."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "make-it-3d_amd"))

RESIDENT = 4096


@pytest.fixture(scope="module")
def lib():
    from mi3d import _lib as L
    return L


def plan(lib, N):
    out = (C.c_uint32 * 3)(9, 9, 9)
    lib.call("mi3d_march_train_plan", N, out)
    return tuple(out)


def cdiv(a, b):
    return -(-a // b)


# N, rays per wave, rounds of the busiest wave: both sides of every switch of the launch heuristic
BOUNDARIES = [
    (1, 64, 1), (37, 64, 1), (64, 64, 1),                      # one wave's worth of rays stays one wave
    (65, 16, 1), (32_736, 16, 1),                              # 32 736 = 1023 x 32: 32 rays per wave would be 1023 waves
    (32_737, 32, 1), (65_472, 32, 1),                          # 65 472 = 1023 x 64
    (65_473, 64, 1), (262_144, 64, 1),                         # 262 144 = 4096 x 64: the last launch of one round
    (262_145, 64, 2), (262_353, 64, 2), (524_288, 64, 2), (524_289, 64, 3),
]


@pytest.mark.parametrize("N,rpw,rounds", BOUNDARIES)
def test_plan_on_both_sides_of_every_boundary(lib, N, rpw, rounds):
    got = plan(lib, N)
    batches = cdiv(N, rpw)
    assert got == (rpw, batches, min(batches, RESIDENT)), (N, got)
    assert cdiv(got[1], got[2]) == rounds


def test_plan_rows_of_the_table(lib):
    """The table as ranges: every N of a sample of each row lands in it, and workgroups == min(batches, 4096)."""
    rows = [(1, 64, 64), (65, 32_736, 16), (32_737, 65_472, 32), (65_473, 262_144, 64), (262_145, 2_000_000, 64)]
    for lo, hi, rpw in rows:
        for N in sorted({lo, lo + 1, (lo + hi) // 2, hi - 1, hi} | set(range(lo, hi + 1, max(1, (hi - lo) // 97)))):
            r, batches, wgs = plan(lib, N)
            assert (r, batches) == (rpw, cdiv(N, rpw)), (N, r, batches)
            assert wgs == min(batches, RESIDENT), (N, wgs)
    assert plan(lib, 32_736)[1] == 2046 and plan(lib, 65_472)[1] == 2046 and plan(lib, 32_737)[1] == 1024
    assert plan(lib, 65_473)[1] == 1024 and plan(lib, 262_144)[1:] == (4096, 4096)
    assert plan(lib, 262_353) == (64, 4100, 4096)              # batches 4096..4099: the second round of waves 0..3


def test_plan_invalid_arguments(lib):
    assert plan(lib, 0) == (0, 0, 0)                           # no rays: nothing is launched
    with pytest.raises(lib.Mi3dError):
        lib.call("mi3d_march_train_plan", 64, None)
    with pytest.raises(lib.Mi3dError):
        lib.call("mi3d_march_train_plan", 0, None)
