"""CPU test of the refusals of the fused flux entry points of the C ABI: every case of the host section of
tests/golden/capi_refusals.json -- one fault or two at once, through ctypes straight to the library on host-only models --
is replayed against this build and compared for equality, return value and message.  The fixture was recorded at the
commit before the fused calls of rte-ecckd_amd/csrc/capi.cpp were gathered into Columns + Particles + outputs;
tests/golden/make_golden_capi_refusals.py describes the recording and holds the cases."""
import json
import os
import re
import sys

import pytest

import __graft_entry__ as entry

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)

import make_golden_capi_refusals as gen   # noqa: E402


@pytest.fixture(scope="module")
def fixture():
    with open(gen.PATH) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def models(pkg):
    return gen.Models(pkg, -1)


def test_every_recorded_refusal_replays_equal(pkg, fixture, models):
    assert re.fullmatch(r"[0-9a-f]{40}", fixture["recorded_at"])
    assert fixture["shape"] == {"ncol": gen.NCOL, "nlay": gen.NLAY}
    want, got = gen.expand(fixture, "host"), gen.record(pkg, models)
    assert len(want) > 5000
    differ = [(key, want[key], got[key]) for key in want if key in got and want[key] != got[key]]
    for key, w, g in differ[:10]:
        print(key, "\n  recorded:", w, "\n  replayed:", g)
    assert not differ, "%d of %d cases differ from the recording, e.g. %s" % (len(differ), len(want), differ[0][0])
    assert set(want) == set(got)


def test_no_entry_point_and_no_case_is_left_unrecorded(fixture, models):
    """Every exported fused flux call has cases in both sections, and every case id of the generator is in the file."""
    fused = {s for s in entry.exported_symbols()
             if ("_fluxes" in s or "_flux_bands" in s or "_flux_scaled" in s) and not s.endswith("_bytes")}
    assert len(fused) == 26
    for section, device in (("host", False), ("device", True)):
        assert set(fixture[section]) == fused, (section, sorted(fused ^ set(fixture[section])))
        recorded = set(gen.expand(fixture, section))
        for name, (ids, changes, pairs) in gen.case_ids(models, device).items():
            expected = {(name, i) for i in ids} | {(name, ids[i] + "+" + ids[j]) for i, j in pairs}
            assert expected == {key for key in recorded if key[0] == name}, (section, name)
            assert len(ids) >= 7 and (device or len(pairs) > len(ids))   # (the plain clear-sky calls have the fewest)
