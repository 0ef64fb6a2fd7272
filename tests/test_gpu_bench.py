"""bench.py's plain run and --dump-outputs: the plain line carries the headline fields and none of the legs of --full, and two
runs with the same arguments (seeded inputs; --deterministic: Gamma reduced in source order) dump the same outputs bit for bit."""
import json
import os
import subprocess
import sys
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 128^3 has more cells than bench.DUMP_SAMPLE_CELLS: the grids are dumped as the seeded sample
ARGS = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--mesh", "128", "--sources", "64", "--deterministic"]
FULL_LEGS = {"other_sweep_mode", "configs1_128_1src", "one_gpu_share_of_8", "configs", "share_504", "dropin_128_1src", "cpu_baseline", "parity"}
DUMPED = {"xh_av", "xh_intermed", "phih_grid", "conv_flag", "sum_xh1", "photon_loss", "sum_nbox"}


def line(out):
    return json.loads([l for l in out.strip().split("\n") if l.startswith("{")][-1])


def test_bench_plain_line_and_dumped_outputs(tmp_path):
    lines = []
    for run in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + ["--dump-outputs", str(tmp_path / run)],
                           capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append(line(r.stdout))
    a = lines[0]
    assert a["steps"] == 2 and a["unit"] == "cells-traced/s" and a["higher_is_better"] is True and a["dtype"] == "f64"
    assert abs(a["value"] * a["ms_per_step"] * 1e-3 / (128 ** 3 * 64) - 1) < 1e-9
    assert not FULL_LEGS & set(a) and a["roofline"]["mix_ceiling_this_box"] is None
    files = {run: sorted((tmp_path / run).iterdir()) for run in ("a", "b")}
    assert {p.stem for p in files["a"]} == DUMPED and all(p.suffix == ".npy" for p in files["a"])
    assert sum(p.stat().st_size for p in files["a"]) <= 64 << 20
    for pa, pb in zip(files["a"], files["b"]):
        x, y = np.load(pa), np.load(pb)
        assert x.dtype in (np.float32, np.float64) and x.shape == y.shape, pa.name
        assert np.array_equal(x, y), pa.name
    assert np.load(tmp_path / "a" / "xh_av.npy").shape == (1 << 20,)
    assert np.load(tmp_path / "a" / "sum_nbox.npy")[0] == a["check"]["sum_nbox_last_step"]
