"""The executor's launch sites switched every way a caller can switch them (tests/net_site_trace.py), step by step against the snapshots
recorded in tests/golden/net_site_trace.json: op names, choice words, launch counts, selected stages / tails / heads and unwritten edges
are what they were before the sites' decisions and the state derived from them were separated (net_resolve, api_net_optimize.hip)."""
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from anakin_amd import lib as L  # noqa: E402
from tests import net_site_trace as NT  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _device():
    L.require_device()


@pytest.fixture(scope="module")
def golden():
    return NT.load_golden()


@pytest.mark.parametrize("walk", sorted(NT.WALKS))
def test_every_step_of_the_walk_equals_the_recorded_trace(walk, golden):
    want = golden[walk]
    got = NT.WALKS[walk]()
    assert [label for label, _ in got] == [label for label, _ in want]
    for (label, g), (_, w) in zip(got, want):
        for key in w:
            assert g[key] == w[key], (walk, label, key, [(i, a, b) for i, (a, b) in enumerate(zip(g[key], w[key])) if a != b]
                                      if isinstance(w[key], list) and len(w[key]) == len(g[key]) else (g[key], w[key]))
        assert g == w, (walk, label)
