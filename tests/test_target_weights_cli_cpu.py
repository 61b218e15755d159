"""--target-weights at the CLI's front end: what the parser refuses and with which line, as tests/test_cli_args_cpu.py checks the
other options -- exit status 255, the `Error:` line and the usage text, before the input is opened and before a device is
looked for."""
import subprocess

import pytest

from megalania_amd import build

MALFORMED = "--target-weights takes cost, cost:mean, cost:N (N from 0 to 4293918719) or file:PATH"
TWICE = "--target-weights given twice"
BARE = None

TABLE = [
    (["--target-weights", ""], MALFORMED), (["--target-weights", "cost:"], MALFORMED), (["--target-weights", "cost:x"], MALFORMED),
    (["--target-weights", "file:"], MALFORMED), (["--target-weights", "costs"], MALFORMED), (["--target-weights", "map"], MALFORMED),
    (["--target-weights", "cost:12x"], MALFORMED), (["--target-weights", "cost:-1"], MALFORMED), (["--target-weights", "cost: 5"], MALFORMED),
    (["--target-weights", "cost:4293918720"], MALFORMED), (["--target-weights", "cost:mean:2"], MALFORMED), (["--target-weights", "FILE:x"], MALFORMED),
    (["--target-weights", "cost", "--target-weights", "cost"], TWICE), (["--target-weights", "cost:0", "--target-weights", "file:w.bin"], TWICE),
    (["--target-weights", "file:w.bin", "--target-weights", "cost:mean"], TWICE),
    # the parser goes along the command line; the combination rules come behind it
    (["--target-weights", "cost:x", "--focus", "5:5"], MALFORMED), (["--focus", "rank", "--target-weights", "cost"], "--focus rank needs --chains N with N at least 2"),
]


def run(args):
    return subprocess.run([build.CLI] + args, capture_output=True, timeout=60)


@pytest.fixture(scope="module")
def usage():
    text = run([]).stderr
    assert text.startswith(b"usage: " + build.CLI.encode() + b" [--neighbours K]") and text.endswith(b"(auto, default)\n")
    assert b"[--target-weights cost[:mean|:N]|file:PATH]" in text and b"\n  --target-weights cost[:mean|:N] | file:PATH  " in text
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
    refused(run([str(f), "--target-weights"]), BARE, usage)
    refused(run(["--target-weights", str(f)]), MALFORMED, usage)  # takes the file name as its value


@pytest.mark.parametrize("value", ["cost", "cost:mean", "cost:0", "cost:4293918719", "file:w.bin"])
def test_accepted_values_reach_the_input(usage, tmp_path, value):
    """a well-formed value passes the parser: the run gets as far as the input, which does not exist"""
    r = run(["--target-weights", value, str(tmp_path / "missing.bin")])
    assert r.returncode == 255 and r.stdout == b"" and usage not in r.stderr and b"--target-weights" not in r.stderr
