"""Create-time sizes, pinned: device_bytes and the capacities right after create equal the values recorded in
golden/create_sizes.json, for one-GPU, row-sharded and slot-sharded handles and one with SWIM_CAPS lowered: a buffer
added to, dropped from or resized in the allocation table (create.hip) shows here. The sizes are far below where free HBM decides
anything except the 8-bit shadow plane (allocated last, if it fits): each case is also created with SWIM_NO_K8, so the
fixture holds the bytes with and without the plane and a change of its presence shows as such."""
import json
from pathlib import Path

import pytest

from swimhip import ClusterConfig, SimConfig, _abi
from swimhip.cluster import SimulatedCluster

from test_gpu_fallbacks import TINY

GOLDEN = Path(__file__).resolve().parent / "golden" / "create_sizes.json"

pytestmark = pytest.mark.gpu

# name: (config, shards, SWIM_CAPS)
CASES = {
    "full300": (SimConfig(n_members=300), 1, None),
    "full300_cold_dormant8": (SimConfig(n_members=300, cluster=ClusterConfig(seedMembers=[0]),
                                        init_mode=_abi.INIT_COLD_JOIN, n_dormant=8), 1, None),
    "full300_delay_emcounters": (SimConfig(n_members=300, delay_cap_ms=500, emulator_counters=True), 1, None),
    "rumor4000_churn40": (SimConfig(n_members=4000, mode=_abi.MODE_RUMOR, churn_per_period=40), 1, None),
    "full300_2shards": (SimConfig(n_members=300), 2, None),
    "rumor4000_churn40_2shards": (SimConfig(n_members=4000, mode=_abi.MODE_RUMOR, churn_per_period=40), 2, None),
    "full300_tiny_caps": (SimConfig(n_members=300), 1, TINY),
}


def measure(engine, name, monkeypatch):
    """[{device_bytes, device_bytes_no_k8, caps}] per shard handle of the case, right after create."""
    cfg, shards, caps = CASES[name]
    out = []
    for no_k8 in (False, True):
        if caps:
            monkeypatch.setenv("SWIM_CAPS", caps)
        if no_k8:
            monkeypatch.setenv("SWIM_NO_K8", "1")
        try:
            if shards == 1:
                c = SimulatedCluster(engine, cfg)
                handles = [c]
            else:
                from swimhip.shard import ThreadShardGroup
                c = ThreadShardGroup(engine, cfg, shards)
                handles = c.shards
        finally:
            monkeypatch.delenv("SWIM_CAPS", raising=False)
            monkeypatch.delenv("SWIM_NO_K8", raising=False)
        for i, s in enumerate(handles):
            b = int(s.counters()["device_bytes"])
            if no_k8:
                out[i]["device_bytes_no_k8"] = b
            else:
                out.append({"device_bytes": b, "caps": {k: int(v) for k, v in _abi.debug_caps(engine, s._h).items()}})
        c.close()
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_create_sizes_pinned(engine, monkeypatch, name):
    want = json.loads(GOLDEN.read_text())[name]
    got = measure(engine, name, monkeypatch)
    print(f"{name}: {got}", flush=True)
    assert got == want
