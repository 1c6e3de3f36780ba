"""bench.py's command line: a plain run does what its headline figure needs and nothing else, --full adds
the extras, --dump-outputs writes the last timed step's outputs, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--width", "96", "--height", "72", "--world", "64", "--steps", "3", "--warmup", "2"]
EXTRAS = ("cpu_baseline", "roofline_chain_alone", "hbm_copy_gbs", "primary_hit_frac", "band_diag", "band_parity")


def run_bench(*args):
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + list(args), cwd=REPO, timeout=240,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_dump_outputs_whole_arrays(tmp_path):
    import bench
    rng = np.random.default_rng(1)
    out, depth = rng.random((9, 7, 4)), rng.random((9, 7)).astype(np.float32)
    assert bench.dump_outputs(str(tmp_path / "d"), {"OUTPUT": out, "DEPTH": depth}) == ["depth", "output"]
    assert sorted(os.listdir(tmp_path / "d")) == ["depth.npy", "output.npy"]
    got = np.load(tmp_path / "d" / "output.npy")
    assert got.dtype == np.float32 and got.shape == out.shape
    np.testing.assert_array_equal(got, out.astype(np.float32))
    np.testing.assert_array_equal(np.load(tmp_path / "d" / "depth.npy"), depth)


def test_dump_outputs_samples_over_the_limit(tmp_path, monkeypatch):
    """Over the byte limit every array keeps the same seeded pixels: the files fit, name their pixels and
    are the same on a second call."""
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4000)
    rng = np.random.default_rng(2)
    out, depth = rng.random((40, 30, 4)).astype(np.float32), rng.random((40, 30)).astype(np.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"OUTPUT": out, "DEPTH": depth})
    a = {f: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    b = {f: np.load(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")}
    assert sorted(a) == ["depth.npy", "output.npy", "sample_pixels.npy"] == sorted(b)
    assert sum(v.nbytes for v in a.values()) <= 4000
    px = a["sample_pixels.npy"].astype(np.int64)
    assert len(px) == 4000 // 28 and (np.diff(px) > 0).all() and px[0] >= 0 and px[-1] < 40 * 30
    np.testing.assert_array_equal(a["output.npy"], out.reshape(-1, 4)[px])
    np.testing.assert_array_equal(a["depth.npy"], depth.reshape(-1, 1)[px])
    for f in a:
        assert a[f].dtype in (np.float32, np.float64)
        np.testing.assert_array_equal(a[f], b[f])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_same_outputs_twice(tmp_path):
    """Two plain runs with the same arguments: no extra in the line, --steps is the number of timed steps
    behind ms_per_step and value, and the dumped last frame is the same, bit for bit."""
    lines = [run_bench(*SMALL, "--dump-outputs", str(tmp_path / d)) for d in ("a", "b")]
    for ln in lines:
        assert ln["full"] is False and ln["steps"] == 3 and ln["warmup"] == 2
        assert all(ln[k] is None for k in EXTRAS), {k: ln[k] for k in EXTRAS}
        assert ln["unit"] == "Mpaths/s" and ln["higher_is_better"] is True and ln["dtype"] == "f32"
        assert ln["ms_per_step"] > 0
        # value = W * H * spp paths per step / the step's time
        assert ln["value"] == pytest.approx(96 * 72 * 4 / (ln["ms_per_step"] * 1e-3) / 1e6, rel=1e-2)
        assert ln["dumped_outputs"] == ["depth", "output"]
    a, b = (np.load(tmp_path / d / "output.npy") for d in ("a", "b"))
    assert a.dtype == np.float32 and a.shape == (72, 96, 4) and np.isfinite(a).all() and a[..., :3].max() > 0
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    da, db = (np.load(tmp_path / d / "depth.npy") for d in ("a", "b"))
    assert da.shape == (72, 96) and (da < 1e26).any()
    np.testing.assert_array_equal(da.view(np.uint32), db.view(np.uint32))


@pytest.mark.gpu
def test_full_run_keeps_the_extras(tmp_path):
    """--full (here without the CPU baseline, which takes its seconds): the chain alone, the copy
    bandwidth and the hit fraction are measured after the timed steps, and the dumped frame is the timed
    steps' last one, not a later one."""
    full = run_bench(*SMALL, "--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "f"))
    assert full["full"] is True and full["cpu_baseline"] is None
    assert full["roofline_chain_alone"]["frames"] == 4 and full["roofline_chain_alone"]["avg_duration_ms"] > 0
    assert full["hbm_copy_gbs"] > 0 and 0 < full["primary_hit_frac"] <= 1
    plain = run_bench(*SMALL, "--dump-outputs", str(tmp_path / "p"))
    assert plain["dumped_outputs"] == full["dumped_outputs"]
    for name in plain["dumped_outputs"]:
        a, b = (np.load(tmp_path / d / (name + ".npy")) for d in ("f", "p"))
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
