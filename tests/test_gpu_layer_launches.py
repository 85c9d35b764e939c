"""The layer modules launch what they launched before their host idioms moved into _lib (pack_codes,
gemm_wonly_rows, backward_ops): for every case of tests/layer_launch_trace.py the ordered wrapper calls with their
bound arguments, the bits of the output and of every gradient (small tensors verbatim, larger ones by the sha256 of
their bytes), and the M == 0 outcomes equal tests/golden/layer_launches_parent.json, recorded on an MI355X at the
parent commit. Exact: the same kernels with the same arguments."""
import json

import pytest

import layer_launch_trace as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(L.GOLDEN) as f:
        return json.load(f)["cases"]


def test_the_golden_file_holds_every_case(golden):
    assert sorted(golden) == sorted(L.CASES)


@pytest.mark.parametrize("name", list(L.CASES))
def test_launches_and_bits_equal_the_parent(dev, golden, name):
    want = golden[name]
    got = json.loads(json.dumps(L.run_case(dev, name)))   # tuples as the lists the file holds
    assert got["outcome"] == want["outcome"]
    assert [l[0] for l in got["launches"]] == [l[0] for l in want["launches"]]
    for i, (g, w) in enumerate(zip(got["launches"], want["launches"])):
        assert g == w, f"launch {i} ({g[0]})"
    assert sorted(got["tensors"]) == sorted(want["tensors"])
    for key, w in want["tensors"].items():
        assert got["tensors"][key] == w, key
