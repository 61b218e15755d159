"""--live-weights through the CLI on the device: the per-epoch line, a stream that decodes to the input in both containers,
and a run without the option that is what it was.  `-m gpu`."""
import lzma
import os
import re
import subprocess

import pytest

from megalania_amd import build, corpus

pytestmark = pytest.mark.gpu

DATA = corpus.enwik_like(6000, 0x71)
BASE = ["--epochs", "1", "--phases", "1", "--steps", "40", "--neighbours", "256", "--greedy-seed", "8"]
LINE = r"^live-weights: every (\d+) steps, floor (\d+|mean), refreshes (\d+), skipped (\d+), (\d+\.\d\d) ms$"


def cli(tmp_path, extra, env=None):
    f = tmp_path / "in.bin"
    f.write_bytes(DATA)
    r = subprocess.run([build.CLI] + BASE + extra + [str(f)], capture_output=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr.decode()[-600:]
    return r.stdout, r.stderr.decode()


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    out, err = cli(tmp_path_factory.mktemp("plain"), [])
    assert "live-weights" not in err and lzma.decompress(out, format=lzma.FORMAT_ALONE) == DATA
    return out


@pytest.mark.parametrize("fmt", ["lzma", "xz"])
def test_live_weights_run_decodes(tmp_path, fmt):
    """--accept auto, the default, with a bulk threshold no step of this input meets: the first block of four steps goes the
    bulk route without weights, the rest the single route -- refreshed before step 4 (due since 0), 5, 10 .. 35"""
    out, err = cli(tmp_path, ["--live-weights", "5:0,single", "--format", fmt], dict(os.environ, MGL_BULK_THRESHOLD="100000"))
    rows = re.findall(LINE, err, re.M)
    assert len(rows) == 1, err[-600:]
    every, floor, refreshes, skipped, ms = rows[0]
    assert (every, floor, skipped) == ("5", "0", "0") and int(refreshes) == 8 and float(ms) > 0
    assert lzma.decompress(out, format=lzma.FORMAT_ALONE if fmt == "lzma" else lzma.FORMAT_XZ) == DATA


def test_mean_floor_under_single_steps_and_a_window(tmp_path, plain):
    out, err = cli(tmp_path, ["--live-weights", "8:mean", "--accept", "single", "--focus", "1000:4000"])
    rows = re.findall(LINE, err, re.M)
    assert len(rows) == 1 and rows[0][:4] == ("8", "mean", "5", "0"), err[-600:]  # steps 0, 8, .. 32 of 40
    assert lzma.decompress(out, format=lzma.FORMAT_ALONE) == DATA


def test_without_the_option_nothing_changed(tmp_path, plain):
    again, err = cli(tmp_path, [])
    assert again == plain and "live-weights" not in err
