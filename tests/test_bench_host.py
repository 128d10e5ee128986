"""Host-side pieces of bench.py that need no GPU: the amdgpu sysfs telemetry parser and the source digest."""
import importlib.util
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent


def _bench():
    spec = importlib.util.spec_from_file_location("bench", REPO / "bench.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_sysfs_telemetry_parser(tmp_path):
    """The three files rocm-smi itself reads: the starred level of pp_dpm_sclk / pp_dpm_mclk and hwmon power in microwatts (power1_average, or
    power1_input where the average is not exported — the MI355X boxes of this pool)."""
    b = _bench()
    d = tmp_path / "device"
    (d / "hwmon" / "hwmon3").mkdir(parents=True)
    (d / "pp_dpm_sclk").write_text("0: 500Mhz\n1: 1931Mhz *\n2: 2400Mhz\n")
    (d / "pp_dpm_mclk").write_text("0: 900Mhz\n1: 2000Mhz *\n")
    (d / "hwmon" / "hwmon3" / "power1_input").write_text("1399000000\n")
    assert b._read_sysfs_telemetry(str(d)) == (1931, 2000, 1399.0)
    (d / "hwmon" / "hwmon3" / "power1_average").write_text("1250000000\n")
    assert b._read_sysfs_telemetry(str(d))[2] == 1250.0
    (d / "pp_dpm_sclk").write_text("0: 500Mhz\n1: 2400Mhz\n")           # no starred level: unknown, not a guess
    assert b._read_sysfs_telemetry(str(d))[0] is None
    assert b._read_sysfs_telemetry(str(tmp_path / "missing")) == (None, None, None)


def test_source_digest_is_stable_and_covers_the_kernel_sources():
    b = _bench()
    a = b.source_digest()
    assert a == b.source_digest() and len(a) == 16
    import inspect
    src = inspect.getsource(b.source_digest)
    assert "*.hip" in src and "*.hpp" in src and "cmx.h" in src


def test_dump_outputs_names_dtypes_and_seeded_sample(tmp_path, monkeypatch):
    """--dump-outputs: every floating-point array of the result by field name, as computed (f32 / f64); above the budget the same seeded
    sample of positions of every array, identical from call to call."""
    import collections

    import numpy as np
    import torch
    b = _bench()
    R = collections.namedtuple("R", ["a", "b", "count"])
    res = (R(torch.arange(10, dtype=torch.float32), torch.arange(10, dtype=torch.float64).reshape(2, 5), torch.zeros(3, dtype=torch.int64)), None)
    snap, info = b.snapshot_outputs(res)
    assert set(snap) == {"0.a", "0.b"} and not info["sampled"]
    lengths = b.write_outputs(tmp_path / "full", snap)
    assert lengths == {"0.a": 10, "0.b": 10}
    a = np.load(tmp_path / "full" / "0.a.npy")
    assert a.dtype == np.float32 and np.array_equal(a, np.arange(10))
    assert np.load(tmp_path / "full" / "0.b.npy").dtype == np.float64

    monkeypatch.setattr(b, "DUMP_BUDGET_BYTES", 4000)
    big = {"x": torch.arange(10_000, dtype=torch.float32), "y": -torch.arange(10_000, dtype=torch.float32)}
    s1, i1 = b.snapshot_outputs(big)
    s2, _ = b.snapshot_outputs(big)
    assert i1["sampled"] and sum(t.numel() * 4 for t in s1.values()) <= 4000
    assert torch.equal(s1["x"], s2["x"]) and torch.equal(s1["x"], -s1["y"])          # same positions in every array and every call
    assert torch.all(s1["x"][1:] >= s1["x"][:-1])


def test_dump_outputs_refused_in_the_dry_run(tmp_path):
    import subprocess
    import sys
    r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--dry-run-scaffolding", "--dump-outputs", str(tmp_path / "d")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--dump-outputs" in r.stderr and not (tmp_path / "d").exists()
