"""Generates tests/golden/grid_plans.npz: the raw integer outputs of the hash grid's host-side planning queries
(mi3d_grid_encode_plan, mi3d_grid_scatter_plan, mi3d_grid_scatter_binned_workspace, mi3d_grid_level_routes,
mi3d_hashgrid_levels) over the matrix of tests/plan_matrix.py, and the return codes of their invalid-argument cases.

    python tests/golden/make_golden_plans.py [path/to/libmi3d.so]

The file in the repository was recorded from the library as it stood BEFORE the planners moved into
csrc/mi3d_grid_plan.h (the launches and the queries then each derived their plans on their own); tests/test_plan_cpu.py
holds every later library to it.  Rerun it only when a plan is meant to change.  No GPU is involved: the queries are host
arithmetic.  The file is written with fixed zip timestamps, so a rerun reproduces it byte for byte."""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, HERE)
    import plan_matrix
    from make_golden_pointcloud import save_npz

    so = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "make-it-3d_amd", "csrc", "libmi3d.so")
    rec = plan_matrix.record(ctypes.CDLL(so))
    for name, rc in zip(rec["invalid_case"], rec["invalid_rc"]):
        print(f"{name}: {rc}")
    path = os.path.join(HERE, "grid_plans.npz")
    save_npz(path, rec)
    print(f"{path}: {os.path.getsize(path)} bytes from {so}")


if __name__ == "__main__":
    main()
