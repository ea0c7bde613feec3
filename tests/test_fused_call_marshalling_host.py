"""CPU test of the Python mirror's fused flux calls (lw_fluxes*, sw_fluxes*): every case of
tests/golden/fused_call_marshalling.json -- the arguments each ``ecckd_*_fluxes*`` entry point is handed, argument by
argument, and the answer to every refused call, as message or as exception -- is replayed against this tree and compared
for equality.  The fixture was recorded at the commit before the marshalling of these calls was gathered into one helper and
has not been regenerated since; tests/golden/make_golden_fused_calls.py describes the recording and holds the cases."""
import json
import os
import re
import sys

import pytest

import __graft_entry__ as entry

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)

import make_golden_fused_calls as gen   # noqa: E402


@pytest.fixture(scope="module")
def fixture():
    with open(gen.PATH) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def replayed(pkg):
    models = gen.load_models(pkg)
    return [gen.run(pkg, models, c) for c in gen.cases(pkg, models)]


def test_every_recorded_case_replays_equal(fixture, replayed):
    assert re.fullmatch(r"[0-9a-f]{40}", fixture["recorded_at"])
    assert fixture["shape"] == {"nlay": gen.NLAY, "ncol": gen.NCOL}
    assert [r[0] for r in replayed] == [r[0] for r in fixture["cases"]]
    # (through JSON once, as the fixture went: tuples and lists, float text)
    differ = [(want, got) for want, got in zip(fixture["cases"], json.loads(json.dumps(replayed))) if want != got]
    for want, got in differ[:10]:
        print("recorded:", json.dumps(want))
        print("replayed:", json.dumps(got))
    assert not differ, "%d of %d cases differ from the recording, e.g. %s" % (len(differ), len(replayed), differ[0][0][0])


def test_no_entry_point_is_left_unrecorded(pkg, fixture):
    """The entry points seen over the recorded calls are all the ``ecckd_*_fluxes*`` symbols the binding calls."""
    seen = {r[2] for r in fixture["cases"] if r[1] == "called"}
    fused = {s for s in entry.exported_symbols() if "_fluxes" in s and not s.endswith("_bytes")}
    source = open(os.path.join(os.path.dirname(pkg.__file__), "__init__.py")).read()
    bound = set(re.findall(r"\becckd_[a-z0-9_]*_fluxes[a-z0-9_]*", source))
    called = {s for s in fused if s in bound}
    assert seen == called, (sorted(called - seen), sorted(seen - called))
