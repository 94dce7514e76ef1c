"""bench.py on one GPU at a small size: a plain run reports the headline figures only, --dump-outputs writes what the
timed path returned (the same waveforms the engine gives for the same seeded batch), --full adds the per-kernel pass,
the power-cap ceiling, the golden comparison and the CPU legs."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

ARGV = ["--gpus", "1", "--clips-per-gpu", "3", "--seconds", "1", "--steps", "2", "--warmup", "1"]


def _line(capsys):
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_bench_plain_and_full_lines_and_dumped_outputs(lib_built, tmp_path, capsys, monkeypatch):
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    sys.path.insert(0, ROOT)
    import bench
    out = str(tmp_path / "out")
    assert bench.main(ARGV + ["--dump-outputs", out]) == 0
    line = _line(capsys)
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["status_flags"] == 0
    audio_per_step = 3 * (98 * 160 + 240) / 16000.0                       # three 1 s clips trimmed to 98 frames
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 - audio_per_step) < 1e-6 * audio_per_step
    for k in ("metric", "unit", "higher_is_better", "dtype"):
        assert k in line
    for k in ("roofline", "hbm_kernels", "kernel_ms_per_step", "cpu_baseline", "device_state", "rms_vs_golden_10s"):
        assert k not in line, k
    assert sorted(os.listdir(out)) == ["denoised_wav.npy", "denoised_wav_clips.npy"]
    wav = np.load(os.path.join(out, "denoised_wav.npy"))
    assert wav.dtype == np.float32 and np.load(os.path.join(out, "denoised_wav_clips.npy")).tolist() == [0, 1, 2]
    from nhans_amd import engine, weights
    mixes, ca, cb, _ = bench.make_batch("denoiser", 0, 3, 1.0, 0)
    eng = engine.Engine("denoiser", weights.synthetic_weights("denoiser", 7), precision="f16x3")
    ref = np.concatenate(eng.enhance(mixes, ca, cb, want_mixed=False)["denoised_wav"])
    eng.close()
    assert wav.shape == ref.shape and np.abs(wav - ref).max() < 1e-6

    assert bench.main(ARGV + ["--full", "--ceiling-seconds", "0.2", "--cpu-frames", "2"]) == 0
    line = _line(capsys)
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    assert line["roofline"]["kernel"] and line["roofline"]["per_kernel"] and line["kernel_ms_per_step"]
    assert line["roofline"]["peak_at_power_cap"] > 0 and "stft_features_GBs" in line["hbm_kernels"]
    assert "device_state" in line and line["rms_vs_golden_10s"] is None              # (the golden clip is 10 s)
    assert line["cpu_baseline"]["frames_per_s"] > 0 and line["rms_check"]["rms"] < line["rms_check"]["tolerance"]
