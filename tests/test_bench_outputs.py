"""bench.py's plain run, --full and --dump-outputs: the options, the dumped arrays (on the oracle, the same C ABI), and one
small run of the script itself on the GPU."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from swimhip import SimConfig, SimulatedCluster

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402

NAMES = {"state_hash", "counters", "row_observers", "row_incarnation", "row_status", "row_has_metadata",
         "row_suspicion_deadline"}


def check_dump(d, n):
    files = {p.stem: np.load(p) for p in Path(d).glob("*.npy")}
    assert set(files) == NAMES
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    rows = min(bench.DUMP_ROWS, n)
    assert files["state_hash"].shape == (n, 12) and files["counters"].shape == (len(bench.DUMP_COUNTERS),)
    assert files["row_observers"].shape == (rows,)
    assert all(files[k].shape == (rows, n) for k in NAMES if k.startswith("row_") and k != "row_observers")
    return files


def test_plain_run_is_the_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"


def test_dump_outputs_carries_the_state_exactly(oracle, tmp_path):
    n = 300
    dumps = []
    for k in range(2):  # the same arguments give the same arrays
        with SimulatedCluster(oracle, SimConfig(n_members=n)) as c:
            c.update_incarnation(5)
            c.run_periods(4)
            bench.dump_outputs(c, n, tmp_path / str(k))
            f = check_dump(tmp_path / str(k), n)
            h = c.state_hash()
            assert np.array_equal(f["state_hash"][:, 0::2].astype(np.uint64) << np.uint64(32)
                                  | f["state_hash"][:, 1::2].astype(np.uint64), h)
            ctr = c.counters()
            assert [int(v) for v in f["counters"]] == [ctr[k2] for k2 in bench.DUMP_COUNTERS]
            for i, o in enumerate(f["row_observers"].astype(int)):
                row = c.row(int(o))
                back = (f["row_incarnation"][i].astype(np.uint64) | f["row_status"][i].astype(np.uint64) << np.uint64(32)
                        | f["row_has_metadata"][i].astype(np.uint64) << np.uint64(34)
                        | f["row_suspicion_deadline"][i].astype(np.uint64) << np.uint64(35))
                assert np.array_equal(back, row)
            dumps.append(f)
    assert all(np.array_equal(dumps[0][k], dumps[1][k]) for k in NAMES)
    assert dumps[0]["row_incarnation"].max() == 1  # the bumped member's record reached a sampled row


@pytest.mark.gpu
def test_bench_plain_run_on_gpu(tmp_path):
    n = 2000
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--members", str(n), "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["cpu_baseline"] is None and line["higher_is_better"] is True
    assert line["unit"] == "member·periods/s" and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(n * 1e3 / line["ms_per_step"])
    assert line["run_totals"]["ticks"] == (3 + 1) * line["config"]["ticks_per_period"]
    f = check_dump(tmp_path / "out", n)
    assert int(f["counters"][0]) == line["run_totals"]["ticks"]
