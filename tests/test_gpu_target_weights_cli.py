"""--target-weights through the CLI on a device: cost weights per epoch, a map written by one run steering the next, a weights
file of the wrong size, and the x86 filter.  The input is the 8 277-byte file of tests/test_gpu_focus.py.  `-m gpu`."""
import lzma
import re
import subprocess

import numpy as np
import pytest

import test_gpu_focus as tf
from megalania_amd import build

pytestmark = pytest.mark.gpu

DATA, N = tf.DATA, tf.N
BASE = ["--epochs", "2", "--phases", "1", "--neighbours", "64"]


def cli(args):
    return subprocess.run([build.CLI] + args, capture_output=True, timeout=600)


@pytest.fixture()
def infile(tmp_path):
    f = tmp_path / "in.bin"
    f.write_bytes(DATA)
    return str(f)


@pytest.mark.parametrize("value", ["cost", "cost:0"])
def test_cost_weights_per_epoch(tmp_path, infile, value):
    out = tmp_path / "out.lzma"
    r = cli(["--target-weights", value] + BASE + ["-o", str(out), infile])
    assert r.returncode == 0 and r.stdout == b"", r.stderr.decode()[-600:]
    assert lzma.decompress(out.read_bytes(), format=lzma.FORMAT_ALONE) == DATA
    rows = re.findall(r"^target-weights: cost map \+ (\d+) per byte, total (\d+), [\d.]+ ms$", r.stderr.decode(), re.M)
    assert len(rows) == 2  # made again before every epoch's run
    floor, total = int(rows[0][0]), int(rows[0][1])
    if value == "cost":  # the mean cost of a byte: the floor weighs as much as the map, short of the division's remainder
        cost = total - floor * N
        assert floor == cost // N and 0 <= cost - floor * N < N
    else:
        assert floor == 0


def test_a_cost_map_steers_the_next_run(tmp_path, infile):
    m, out = tmp_path / "m.bin", tmp_path / "out.lzma"
    r = cli(BASE + ["--cost-map", str(m), "-o", str(tmp_path / "first.lzma"), infile])
    assert r.returncode == 0, r.stderr.decode()[-600:]
    assert m.stat().st_size == 4 * N
    r = cli(BASE + ["--target-weights", "file:" + str(m), "--focus", "1000:8000", "-o", str(out), infile])
    assert r.returncode == 0 and b"target-weights:" not in r.stderr, r.stderr.decode()[-600:]
    assert lzma.decompress(out.read_bytes(), format=lzma.FORMAT_ALONE) == DATA
    # the weights matter: the same run without them ends elsewhere
    plain = cli(BASE + ["--focus", "1000:8000", infile])
    assert plain.returncode == 0 and lzma.decompress(plain.stdout, format=lzma.FORMAT_ALONE) == DATA
    # one entry short, one entry long, missing: 255, an `Error:` line, no output file
    for name, raw in (("short", m.read_bytes()[:-4]), ("long", m.read_bytes() + b"\0\0\0\0"), ("ragged", m.read_bytes()[:-1]), ("missing", None)):
        bad, gone = tmp_path / (name + ".bin"), tmp_path / (name + ".lzma")
        if raw is not None:
            bad.write_bytes(raw)
        r = cli(BASE + ["--target-weights", "file:" + str(bad), "-o", str(gone), infile])
        assert r.returncode == 255 and r.stdout == b"" and not gone.exists(), name
        assert len(re.findall(rb"^Error: ", r.stderr, re.M)) == 1 and str(bad).encode() in r.stderr and b"usage:" not in r.stderr, name


def test_all_zero_weights_are_the_plain_run(tmp_path, infile):
    z = tmp_path / "zero.bin"
    z.write_bytes(np.zeros(N, dtype="<u4").tobytes())
    a = cli(BASE + ["--target-weights", "file:" + str(z), infile])
    b = cli(BASE + [infile])
    assert a.returncode == 0 and b.returncode == 0 and a.stdout == b.stdout and lzma.decompress(a.stdout, format=lzma.FORMAT_ALONE) == DATA


def test_x86_filter(tmp_path, infile):
    out = tmp_path / "out.xz"
    r = cli(["--format", "xz", "--filter", "x86", "--target-weights", "cost"] + BASE + ["-o", str(out), infile])
    assert r.returncode == 0, r.stderr.decode()[-600:]
    assert lzma.decompress(out.read_bytes(), format=lzma.FORMAT_XZ) == DATA
    assert len(re.findall(rb"^target-weights: ", r.stderr, re.M)) == 2
