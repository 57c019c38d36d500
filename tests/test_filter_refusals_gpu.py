"""Every refusal of the filtered search calls, and of the unfiltered range calls that share their scaffold, held to the record: status and
vers_last_error() text byte for byte, and what the call left in *out_total (tests/refusal_cases.py: the list; tests/golden/filter_refusals.json:
the record, written by scripts/record_refusals.py before the host paths were folded into one check and one scaffold).  Where several refusals
apply at once the record says which one is reported; the b == 0 cases pin that the top-k calls check first and the range calls return first."""
import json
import os

import pytest

from tests import refusal_cases as rc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "filter_refusals.json")


def test_every_refusal_is_the_recorded_one():
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(want) == sorted(rc.case_ids()), "the case list and the record differ: a case was added or dropped without the other"
    env = rc.Env()
    try:
        got = env.run()
    finally:
        env.close()
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, "\n".join(f"{k}: got {g}, recorded {w}" for k, (g, w) in wrong.items())
    # what the list is for: everything but the range calls' b == 0 return is a refusal
    assert all(v[0] != 0 for k, v in want.items() if not k.endswith(":b_0_and_nprobe_0"))


def test_the_list_covers_every_filtered_entry_point():
    from vers_amd import capi
    named = {e.name for e in rc.entries()}
    for name in capi.SIGNATURES:
        if ("_filtered" in name or "_prepared_dev" in name) and name.startswith(("vers_ivf_search", "vers_ivf_range_search")):
            assert name in named, name
