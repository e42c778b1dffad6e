"""Every forward makes the C-ABI calls ``tests/golden/launch_records.json`` recorded for it: same entry points, same order,
same scalar arguments, same operand descriptors, same streams (``tests/launch_record.py``).  The library behind the ABI being
the same, that is the same computation - the check under which the Python orchestration (``graph_weather_amd/layers.py``,
``analysis.py``, ``regional.py``) may be rearranged."""
import functools

import pytest

pytestmark = pytest.mark.gpu

from . import launch_record as lr  # noqa: E402


@functools.lru_cache(maxsize=None)
def _golden():
    return lr.load_golden()


def test_the_golden_records_reach_every_route_the_block_call_serves():
    missing = [route for route, seen in lr.coverage(_golden()).items() if not seen]
    assert not missing, "the golden launch records never take: %s" % ", ".join(missing)


def test_the_golden_holds_exactly_the_cases():
    assert sorted(_golden()) == sorted(lr.CASES)


@pytest.mark.parametrize("case", sorted(lr.CASES))
def test_a_forward_makes_the_recorded_calls(case):
    want, got = _golden()[case], lr.record_case(case)
    for i, (w, g) in enumerate(zip(want, got)):
        if w != g:
            around = [c[0] for c in got[max(0, i - 3):i]]
            pytest.fail("%s: call %d differs (after %s)\n  recorded: %s\n  made:     %s" % (case, i, around, w, g))
    assert len(got) == len(want), "%s: %d calls made, %d recorded; first surplus / missing: %s" % (
        case, len(got), len(want), (got[len(want):] or want[len(got):])[0][0])
