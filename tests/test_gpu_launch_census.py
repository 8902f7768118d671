"""GPU: which forms the decoder walks select, as launch counts per profile class (tests/decoder_cases.py).

tests/golden/decoder_launch_census.json is a recorded result: tools/decoder_census.py --golden, run on the commit before the
decoder walks were folded into one per arithmetic (the V and C cases: on the commit before the three forward pipelines were
folded into one, where the same run reproduced the older entries).  A refactor of the walks keeps every count: the bias decoder must not
start taking the short-input or fused forms, the ASR decoder must keep its three-launch layer, the int8 bias decoder its
two passes.  The streaming seam is not in the census: that fold gave its non-GEMM launches the brackets of the bias
decoder, so its counts changed by design; tools/decoder_census.py reports its bit identity."""
import json
import os

import pytest

import decoder_cases as DC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decoder_launch_census.json"),
              encoding="utf-8") as f:
        return json.load(f)


@pytest.mark.parametrize("case", DC.OFFLINE, ids=[c.name for c in DC.OFFLINE])
def test_decoder_launch_census(case, golden):
    got = DC.launch_census(case)                      # asserts the case's side of the 512-row threshold itself
    want = golden[case.name]
    print("%s: B * L = %d (recorded %d)" % (case.name, got["rows"], want["rows"]))
    assert got["rows"] == want["rows"]
    assert got["launches"] == want["launches"], {
        c: (got["launches"].get(c, 0), want["launches"].get(c, 0))
        for c in set(got["launches"]) | set(want["launches"])
        if got["launches"].get(c, 0) != want["launches"].get(c, 0)}
