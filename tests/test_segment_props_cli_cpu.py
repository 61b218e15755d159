"""--segment-props at the CLI's front end, in the manner of tests/test_live_weights_cli_cpu.py: what the parser and the
combination rules refuse and with which line -- exit status 255, the `Error:` line and the usage text, nothing on stdout,
before the input is opened and before a device is looked for."""
import subprocess

import pytest

from megalania_amd import build

MALFORMED = "--segment-props takes a number of bytes, at least 1, or auto"
NEEDS_XZ = "--segment-props needs --format xz: an .lzma stream cannot reset its state or change lc/lp/pb"
ONE_TRIPLE = "--segment-props cannot be combined with --cost-map, --cost-report or --cost-bucket: they describe a stream under one triple"
BARE = None
XZ = ["--format", "xz"]

TABLE = [
    (["--segment-props", ""], MALFORMED), (["--segment-props", "0"], MALFORMED), (["--segment-props", "x"], MALFORMED),
    (["--segment-props", "-5"], MALFORMED), (["--segment-props", " 5"], MALFORMED), (["--segment-props", "64k"], MALFORMED),
    (["--segment-props", "autos"], MALFORMED), (["--segment-props", "Auto"], MALFORMED), (["--segment-props", "4096:2"], MALFORMED),
    (XZ + ["--segment-props", "0x"], MALFORMED),
    (["--segment-props", "auto"], NEEDS_XZ), (["--segment-props", "65536"], NEEDS_XZ), (["--segment-props", "auto", "--format", "lzma"], NEEDS_XZ),
    (XZ + ["--segment-props", "auto", "--format", "lzma"], NEEDS_XZ),  # the last --format wins
    (["--segment-props", "auto", "--cost-report"], NEEDS_XZ),         # two rules broken: the first one answers
    (XZ + ["--segment-props", "auto", "--cost-report"], ONE_TRIPLE), (XZ + ["--cost-map", "m.bin", "--segment-props", "4096"], ONE_TRIPLE),
    (XZ + ["--segment-props", "auto", "--cost-bucket", "4096"], ONE_TRIPLE),
    (XZ + ["--segment-props", "auto", "--cost-map", "m.bin", "--cost-report", "--filter", "x86"], ONE_TRIPLE),
    # rules that come earlier in the order keep their answers
    (XZ + ["--segment-props", "auto", "--props", "auto", "--lc", "3"], "--props auto cannot be combined with --lc/--lp/--pb or with --chains above 1"),
    (["--segment-props", "auto", "--filter", "x86"], "--filter x86 / auto need --format xz: an .lzma stream has no place to declare a filter"),
]


def run(args):
    return subprocess.run([build.CLI] + args, capture_output=True, timeout=60)


@pytest.fixture(scope="module")
def usage():
    build.build_all()
    text = run([]).stderr
    assert text.startswith(b"usage: " + build.CLI.encode() + b" [--neighbours K]") and text.endswith(b"(auto, default)\n")
    assert b" [--segment-props GRAIN|auto] filename\n" in text and b"\n  --segment-props GRAIN|auto  " in text
    assert b"segment-props: grain G cuts C spans S single" in text and b"segment: offset O bytes N" in text
    return text


def refused(r, message, usage):
    assert r.returncode == 255 and r.stdout == b"" and b"no HIP device" not in r.stderr
    assert r.stderr == (b"Error: " + message.encode() + b"\n" if message else b"") + usage


@pytest.mark.parametrize("args,message", TABLE, ids=[" ".join(t[0]) or "empty" for t in TABLE])
def test_refusal(usage, tmp_path, args, message):
    # the input does not exist, and -o names a file: a line that got as far as either would show
    out = tmp_path / "never_written.xz"
    refused(run(args + ["-o", str(out), str(tmp_path / "never_opened.bin")]), message, usage)
    assert not out.exists()


def test_missing_value(usage, tmp_path):
    f = tmp_path / "in.txt"
    f.write_bytes(b"hello hello hello")
    refused(run(XZ + [str(f), "--segment-props"]), BARE, usage)
    refused(run(XZ + ["--segment-props", str(f)]), MALFORMED, usage)  # takes the file name as its value


@pytest.mark.parametrize("value", ["auto", "1", "1024", "65536", "0x10000", "18446744073709551615"])
def test_accepted_values_reach_the_input(usage, tmp_path, value):
    """a well-formed value passes the parser and the rules, with the options it is meant to work with: the run gets as far as the
    input, which does not exist"""
    for more in ([], ["--filter", "x86"], ["--dict-size", "65536"], ["--props", "auto"], ["--lc", "3", "--pb", "2"],
                 ["--chains", "2", "--rank", "1", "--comm-file", str(tmp_path / "comm")], ["--adaptive-seed", "3", "--match-finder", "frontier"]):
        r = run(XZ + ["--segment-props", value] + more + [str(tmp_path / "missing.bin")])
        assert r.returncode == 255 and r.stdout == b"" and usage not in r.stderr and b"--segment-props" not in r.stderr
