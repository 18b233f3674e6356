"""bench.py's stdout carries ONE line, the JSON (the driver reads it); whatever a library prints on stdout while the legs run -- this image's RCCL prints a banner
from C when a communicator is created -- must end up on stderr."""
import json
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_only_the_line_reaches_stdout():
    code = textwrap.dedent(f'''
        import sys, ctypes
        sys.path.insert(0, {ROOT!r})
        import bench
        t = bench._OnlyTheLineOnStdout()
        print("noise from python")
        ctypes.CDLL(None).puts(b"noise from C")
        t.line('{{"metric": "correlators/s"}}')
        ctypes.CDLL(None).puts(b"late noise from C")
    ''')
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == '{"metric": "correlators/s"}\n'
    for noise in ("noise from python", "noise from C", "late noise from C"):
        assert noise in r.stderr


def test_dump_outputs_layout(tmp_path):
    """--dump-outputs: every bank's outputs, the first `taps` columns, as float32 [banks, jobs, taps, 2 (re, im)]."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench

    class Bank:
        def __init__(self, seed):
            rng = np.random.default_rng(seed)
            self.out = (rng.standard_normal((7, 8)) + 1j * rng.standard_normal((7, 8))).astype(np.complex64)

        def read_outputs(self):
            return self.out

    banks = [Bank(1), Bank(2)]
    bench.dump_outputs(str(tmp_path / "d"), banks, 3)
    a = np.load(tmp_path / "d" / "correlator_outputs.npy")
    assert a.dtype == np.float32 and a.shape == (2, 7, 3, 2)
    for k, b in enumerate(banks):
        assert np.array_equal(a[k, ..., 0], b.out[:, :3].real) and np.array_equal(a[k, ..., 1], b.out[:, :3].imag)


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only_and_dumps(gpu, tmp_path):
    """A plain run (no --full): the contract keys, none of the --full legs, --steps honoured, and the dump of both banks' last launches -- the
    same job table over copies of one block, so the two banks' arrays are equal."""
    import numpy as np
    d = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--settle-steps", "0",
                        "--blocks-per-step", "4", "--epochs", "40", "--ring-blocks", "2", "--dump-outputs", str(d)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["metric"] == "correlators/s" and res["unit"] == "correlators/s" and res["higher_is_better"] is True and res["dtype"] == "f32"
    assert res["steps"] == 3 and res["value"] > 0 and res["ms_per_step"] > 0
    assert res["ms_per_step"] == pytest.approx(res["config"]["timed_region_s"] / 3 * 1e3)
    for leg in ("roofline", "spot_check", "value_single_stream", "acquisition", "closed_loop", "dropin", "cpu_baseline", "summary"):
        assert leg not in res, leg
    a = np.load(d / "correlator_outputs.npy")
    assert a.dtype == np.float32 and a.shape == (2, 32 * 40, 3, 2) and np.all(np.isfinite(a)) and np.any(a != 0)
    assert np.array_equal(a[0], a[1])
