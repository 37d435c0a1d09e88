"""bench.py's plain / --full split and --dump-outputs.

CPU: a plain command line leaves every side line out and --full brings them
back, each still switched off by its own --no-... option.  GPU: one small
plain run with --dump-outputs, its line and its files checked against the
oracle's `fse_compress2` (lib.rs:146-183)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE_FLAGS = ("no_cpu", "no_c3", "no_serial", "no_onestate", "no_sweep", "no_host_calls", "no_gather")
SIDE_LINES = ("c3_decode_only", "sidecar_less_decode", "one_state", "c5_sweep", "cpu_baseline", "host_call_latency",
              "c4_exchange")


def _parse(monkeypatch, *argv):
    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_command_line_leaves_side_lines_out(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    assert all(getattr(a, f) for f in SIDE_FLAGS)


def test_full_command_line_keeps_side_lines_and_their_switches(monkeypatch):
    a = _parse(monkeypatch, "--full")
    assert a.full and not any(getattr(a, f) for f in SIDE_FLAGS)
    a = _parse(monkeypatch, "--full", "--no-sweep", "--no-cpu")
    assert a.no_sweep and a.no_cpu and not a.no_c3 and not a.no_host_calls


def test_steps_must_be_positive(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--steps", "0")


@pytest.mark.gpu
def test_plain_run_dumps_last_step_outputs(tmp_path):
    """9 blocks (the last one short) through a plain run: the line carries the
    timed step only, and the dumped arrays are the step's outputs: every
    block's compressed bytes equal the oracle's for the decoded block."""
    from oracle import oracle as O

    block, n = 65536, 8 * 65536 + 4321
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--bytes", str(n), "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["verified_roundtrip"] is True and line["dtype"] == "u8" and line["unit"] == "GiB/s"
    assert not [k for k in SIDE_LINES if k in line]

    arrays = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    nb = -(-n // block)
    decoded = arrays["decoded"]
    assert decoded.shape == (n,)  # fewer bytes than the sample size: written whole
    src = decoded.astype(np.uint8)
    assert np.array_equal(src.astype(decoded.dtype), decoded)
    assert not arrays["encode_status"].any() and not arrays["decode_status"].any()
    assert np.array_equal(arrays["compressed_block_index"], np.arange(nb))
    blocks = arrays["compressed_blocks"]
    weight = np.arange(blocks.shape[1]) % 251 + 1
    for b in range(nb):
        want, bits = O.compress2(src[b * block:(b + 1) * block])
        ln = int(arrays["comp_len"][b])
        got = blocks[b].astype(np.uint8)
        assert got[:ln].tobytes() == want and not got[ln:].any()
        assert int(arrays["payload_bits"][b]) == bits
        assert arrays["compressed_block_sums"][b].tolist() == [int(got.sum(dtype=np.int64)),
                                                               int((got.astype(np.int64) * weight).sum())]
    assert arrays["sidecar_lo32"].shape == arrays["sidecar_hi32"].shape and arrays["sidecar_lo32"].any()
