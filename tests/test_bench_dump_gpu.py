"""A plain `bench.py` run (no `--full`): the headline steps and nothing else in its line, `--steps` honoured, and what
`--dump-outputs` writes is what the timed call returned -- scales and zero points against the digests of what the reference
returned for the same matrix (tests/golden/digests.json, config2_asym), the sampled blob bytes against the oracle's blob."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oq_oracle as O
from conftest import ROOT, load_json


def _sha16(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 7 and line["warmup"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "M-param/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["roofline"]["launch_us"] > 0
    for extra in ("gptq", "model_file_7b", "model_rtn", "seam", "calibration", "awq", "searches", "rccl_selftest", "cpu_baseline"):
        assert line[extra] is None, extra

    files = {f: np.load(out / f) for f in sorted(os.listdir(out))}
    assert sorted(files) == ["q_sample.npy", "scales.npy", "zero_points.npy"]
    assert all(a.dtype == np.float32 for a in files.values())
    assert sum(os.path.getsize(out / f) for f in files) <= 64 * 2**20
    d = load_json("digests.json")["config2_asym"]
    assert _sha16(files["scales.npy"]) == d["s_sha"]
    assert _sha16(files["zero_points.npy"].astype(np.uint8)) == d["z_sha"]

    w = np.random.default_rng(0).standard_normal((4096, 11008), dtype=np.float32)
    assert _sha16(w) == d["w_sha"]
    blob = np.asarray(O.seam_arrays(w, "rtn", "uint4", "group", 128, nbits=True)[0]).reshape(-1)
    idx = np.sort(np.random.default_rng(0).choice(blob.size, 1 << 23, replace=False))
    assert np.array_equal(files["q_sample.npy"], blob[idx].astype(np.float32))
