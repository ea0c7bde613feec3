"""GPU test of the refusals that the fused flux entry points of the C ABI answer only with a model on a device (a null
required array, a bad memory space, bad ncol / nlay, no columns, a cloud mask on a model of 65 g-points): the device section
of tests/golden/capi_refusals.json replayed for equality.  No case launches a kernel.  The recording:
tests/golden/make_golden_capi_refusals.py."""
import json
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)

import make_golden_capi_refusals as gen   # noqa: E402


@pytest.mark.gpu
def test_every_recorded_device_refusal_replays_equal(pkg, gpu):
    with open(gen.PATH) as f:
        fixture = json.load(f)
    want, got = gen.expand(fixture, "device"), gen.record(pkg, gen.Models(pkg, 0), device=True)
    assert len(want) > 250
    differ = [(key, want[key], got[key]) for key in want if key in got and want[key] != got[key]]
    for key, w, g in differ[:10]:
        print(key, "\n  recorded:", w, "\n  replayed:", g)
    assert not differ, "%d of %d cases differ from the recording, e.g. %s" % (len(differ), len(want), differ[0][0])
    assert set(want) == set(got)
