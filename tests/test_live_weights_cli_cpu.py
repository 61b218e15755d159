"""--live-weights at the CLI's front end, in the manner of tests/test_target_weights_cli_cpu.py: what the parser and the
combination rules refuse and with which line -- exit status 255, the `Error:` line and the usage text, before the input is
opened and before a device is looked for."""
import subprocess

import pytest

from megalania_amd import build

MALFORMED = "--live-weights takes R, R:N, R:mean (R from 1, N from 0 to 4293918719), optionally followed by ,single"
TWICE = "--live-weights given twice"
BOTH = "--live-weights and --target-weights exclude each other"
BARE = None

TABLE = [
    (["--live-weights", ""], MALFORMED), (["--live-weights", "0"], MALFORMED), (["--live-weights", "x"], MALFORMED),
    (["--live-weights", "-5"], MALFORMED), (["--live-weights", " 5"], MALFORMED), (["--live-weights", "4294967296"], MALFORMED),
    (["--live-weights", "25:"], MALFORMED), (["--live-weights", "25:x"], MALFORMED), (["--live-weights", "25:-1"], MALFORMED),
    (["--live-weights", "25:4293918720"], MALFORMED), (["--live-weights", "25:means"], MALFORMED), (["--live-weights", "25:mean:2"], MALFORMED),
    (["--live-weights", "25,"], MALFORMED), (["--live-weights", "25,singles"], MALFORMED), (["--live-weights", "25,single,single"], MALFORMED),
    (["--live-weights", "25:0:single"], MALFORMED), (["--live-weights", "single"], MALFORMED), (["--live-weights", "mean"], MALFORMED),
    (["--live-weights", "25x"], MALFORMED), (["--live-weights", "0:mean"], MALFORMED), (["--live-weights", "cost"], MALFORMED),
    (["--live-weights", "25", "--live-weights", "25"], TWICE), (["--live-weights", "5:mean", "--live-weights", "7,single"], TWICE),
    (["--live-weights", "x", "--live-weights", "7"], MALFORMED),
    (["--live-weights", "25", "--target-weights", "cost"], BOTH), (["--target-weights", "file:w.bin", "--live-weights", "25:0,single"], BOTH),
    # the parser goes along the command line; the combination rules come behind it, in their order
    (["--live-weights", "25", "--target-weights", "costs"], "--target-weights takes cost, cost:mean, cost:N (N from 0 to 4293918719) or file:PATH"),
    (["--focus", "rank", "--live-weights", "25", "--target-weights", "cost"], "--focus rank needs --chains N with N at least 2"),
]


def run(args):
    return subprocess.run([build.CLI] + args, capture_output=True, timeout=60)


@pytest.fixture(scope="module")
def usage():
    text = run([]).stderr
    assert text.startswith(b"usage: " + build.CLI.encode() + b" [--neighbours K]") and text.endswith(b"(auto, default)\n")
    assert b"          [--live-weights R[:N|:mean][,single]]\n" in text and b"\n  --live-weights R[:N|:mean][,single]  " in text
    assert text.index(b"[--target-weights") < text.index(b"[--live-weights") < text.index(b"[--cost-map FILE]")
    return text


def refused(r, message, usage):
    assert r.returncode == 255 and r.stdout == b"" and b"no HIP device" not in r.stderr
    assert r.stderr == (b"Error: " + message.encode() + b"\n" if message else b"") + usage


@pytest.mark.parametrize("args,message", TABLE, ids=[" ".join(t[0]) or "empty" for t in TABLE])
def test_refusal(usage, tmp_path, args, message):
    # the input does not exist: a line that got as far as opening it would say so instead
    refused(run(args + [str(tmp_path / "never_opened.bin")]), message, usage)


def test_missing_value(usage, tmp_path):
    f = tmp_path / "in.txt"
    f.write_bytes(b"hello hello hello")
    refused(run([str(f), "--live-weights"]), BARE, usage)
    refused(run(["--live-weights", str(f)]), MALFORMED, usage)  # takes the file name as its value


@pytest.mark.parametrize("value", ["1", "25", "4294967295", "25:0", "25:4293918719", "25:mean", "25,single", "5:0,single", "16:mean,single"])
def test_accepted_values_reach_the_input(usage, tmp_path, value):
    """a well-formed value passes the parser: the run gets as far as the input, which does not exist"""
    for more in ([], ["--focus", "10:20"], ["--accept", "auto", "--format", "xz"]):
        r = run(["--live-weights", value] + more + [str(tmp_path / "missing.bin")])
        assert r.returncode == 255 and r.stdout == b"" and usage not in r.stderr and b"--live-weights" not in r.stderr
