"""Runs every case of tests/refusal_cases.py against the library as built and writes status + vers_last_error() text of each to
tests/golden/filter_refusals.json, which tests/test_filter_refusals_gpu.py holds later builds to.  Run ONCE, on the commit whose refusals are
the contract (the parent of a refactor of the filtered host paths); a later run would only record what the code does then."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import refusal_cases as rc

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "filter_refusals.json")
env = rc.Env()
got = env.run()
env.close()
assert list(got) == rc.case_ids()
with open(out, "w") as f:
    json.dump(got, f, indent=0, sort_keys=True)
    f.write("\n")
accepted = [k for k, v in got.items() if v[0] == 0]
print(f"{len(got)} cases recorded to {out}; returned VERS_OK: {accepted}")
