#!/usr/bin/env python3
"""commit_states.py - the walk of tests/commit_walk.py (every source of csrc/host/commit_plan.hpp's table: a new value, the same value again, back) with
the tuner off, the general layout and the pooled pipeline forced: what each commit makes the next frames LAUNCH - a schedule sorted again, a block list
rebuilt, a clear pass, a shadow lattice built - is only visible from outside:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/commit_states.py

once with this tree's library and once with another build's (OVR_HIP_LIBRARY=...), then `python tools/commit_states.py --compare DIR_A DIR_B`: the two
traces must agree line for line, in dispatch order, on kernel name, grid size, workgroup size and LDS size (tools/launch_states.py's comparison)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        from launch_states import compare
        return compare(sys.argv[2], sys.argv[3])
    os.environ["OVR_HIP_TUNE"] = "0"  # the rules alone: nothing a step launches depends on a measured time
    import ovr_amd as ovr
    from commit_walk import Walk
    walk = Walk(ovr, layout=0, pipeline=2)
    try:
        bad = walk.run()
    finally:
        walk.close()
    for row in bad:
        print("MISSED", row)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
