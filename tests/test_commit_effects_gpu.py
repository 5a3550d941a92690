"""What a setter invalidates, as an application sees it (csrc/host/commit_plan.hpp): for every source of the commit plan's table, with a
new value and with the same value again, ovr_hip_stats.frame_index of the frame after the commit - 1 where the accumulation starts over, 4 where it goes
on - and, in shadow mode CACHED, whether ovr_hip_shadow_cache.builds grew - exactly where the lattice is stale.  The walk and its literals are
tests/commit_walk.py; the setters go through the C binding."""
import pytest

from commit_walk import Walk

pytestmark = pytest.mark.gpu


def test_every_source_resets_and_stales_what_the_table_says(ovr):
    walk = Walk(ovr)
    try:
        bad = walk.run()
    finally:
        walk.close()
    assert not bad, bad
