"""The CLI's argument front end as a whole: every refusal of the parser and of the combination rules, with its message,
and the order in which a doubly wrong command line is answered.  All of it happens before the input is opened and before a
device is looked for, so it is the same with and without a GPU.  The expected lines were taken from the driver as it was
before its options moved into one struct and its rules into one pass (host/main.c: parse_args, check_args)."""
import subprocess

import pytest

from megalania_amd import build

S = "stream.lzma"  # never opened: every line below is refused first

SEED_STREAM = "--seed-stream cannot be combined with --load-slab or --greedy-seed"
OPTIMAL = "--optimal-seed cannot be combined with --greedy-seed, --seed-stream or --load-slab"
ADAPTIVE = "--adaptive-seed cannot be combined with --optimal-seed, --greedy-seed, --seed-stream or --load-slab"
FINDER = "--match-finder / --mf-depth need --optimal-seed, --adaptive-seed or --props auto"
SWEEP_FINDER = "--parse-sweep runs both match finders; --match-finder cannot be combined with it"
PROPS_AUTO = "--props auto cannot be combined with --lc/--lp/--pb or with --chains above 1"
PROPS_JOINT = "--props-joint needs --props auto --adaptive-seed P --parse-sweep"
CROSS_GRAIN = "--cross-grain needs --exchange cross or --exchange cross-all"
FILTER_XZ = "--filter x86 / auto need --format xz: an .lzma stream has no place to declare a filter"
FILTER_AUTO = "--filter auto cannot be combined with --seed-stream, --load-slab or --chains above 1"
FOCUS_RANK = "--focus rank needs --chains N with N at least 2"
DICT_SIZE = "--dict-size takes a number of bytes from 4096 to 4294967295 (0 = 4 MiB)"
FOCUS = "--focus takes LO:HI, byte positions with LO < HI, or `rank`"
FOCUS_TWICE = "--focus given twice"
COST_BUCKET = "--cost-bucket takes a number of bytes, at least 1"
BARE = None  # the usage text alone
TWO_CHAINS = "--chains 2 --rank 0 --comm-file c"

# (command line in front of the input's name, the `Error:` line or BARE)
RULES = [  # the combination rules, in the order they are applied
    ("--seed-stream %s --load-slab x" % S, SEED_STREAM), ("--seed-stream %s --greedy-seed 8" % S, SEED_STREAM),
    ("--optimal-seed 2 --greedy-seed 8", OPTIMAL), ("--optimal-seed 2 --seed-stream %s" % S, OPTIMAL), ("--optimal-seed 2 --load-slab x", OPTIMAL),
    ("--adaptive-seed 2 --optimal-seed 2", ADAPTIVE), ("--adaptive-seed 2 --greedy-seed 4", ADAPTIVE),
    ("--adaptive-seed 2 --seed-stream %s" % S, ADAPTIVE), ("--adaptive-seed 2 --load-slab x", ADAPTIVE),
    ("--match-finder frontier", FINDER), ("--match-finder nearest", FINDER), ("--mf-depth 8", FINDER),
    ("--parse-sweep", BARE), ("--parse-sweep --optimal-seed 3", BARE), ("--adaptive-seed 3 --parse-sweep-table", BARE),
    ("--parse-sweep --adaptive-seed 3 --match-finder frontier", SWEEP_FINDER), ("--parse-sweep --adaptive-seed 3 --match-finder nearest", SWEEP_FINDER),
    ("--optimal-seed 2 --mf-depth 8", BARE), ("--optimal-seed 2 --match-finder nearest --mf-depth 8", BARE),
    ("--clip-window", BARE),
    ("--props auto --lc 1", PROPS_AUTO), ("--props auto --lp 0", PROPS_AUTO), ("--props auto --pb 2", PROPS_AUTO), ("--props auto " + TWO_CHAINS, PROPS_AUTO),
    ("--props-table", BARE),
    ("--props-joint 2", PROPS_JOINT), ("--props auto --props-joint 2", PROPS_JOINT), ("--props auto --adaptive-seed 2 --props-joint 2", PROPS_JOINT),
    ("--cross-grain 8", CROSS_GRAIN), ("--exchange best --cross-grain 8", CROSS_GRAIN), ("--exchange cross --exchange best --cross-grain 8", CROSS_GRAIN),
    ("--filter x86", FILTER_XZ), ("--filter auto", FILTER_XZ), ("--format xz --format lzma --filter x86", FILTER_XZ),
    ("--format xz --filter auto --seed-stream %s" % S, FILTER_AUTO), ("--format xz --filter auto --load-slab x", FILTER_AUTO),
    ("--format xz --filter auto " + TWO_CHAINS, FILTER_AUTO),
    ("--focus rank", FOCUS_RANK), ("--focus rank --chains 1", FOCUS_RANK),
    ("--chains 0", BARE), ("--rank -1", BARE), ("--rank 1", BARE), ("--chains 2 --rank 2 --comm-file c", BARE), ("--chains 2", BARE),
]
VALUES = [  # what the parser refuses of a single option
    ("--dict-size 100", DICT_SIZE), ("--dict-size 4096x", DICT_SIZE), ("--dict-size 4294967296", DICT_SIZE),
    ("--focus 5:5", FOCUS), ("--focus 7", FOCUS), ("--focus 1:", FOCUS), ("--focus 1:2 --focus 3:4", FOCUS_TWICE), ("--focus rank --focus 3:4", FOCUS_TWICE),
    ("--cost-bucket 0", COST_BUCKET), ("--cost-bucket 12x", COST_BUCKET),
    ("--mf-depth 0", BARE), ("--mf-depth 4097", BARE),
    ("--props manual", BARE), ("--props-rounds 0", BARE), ("--props-joint 0", BARE), ("--props-joint 5", BARE),
    ("--optimal-seed 0", BARE), ("--adaptive-seed 0", BARE),
    ("--transport tcp", BARE), ("--exchange worst", BARE), ("--format zip", BARE), ("--filter arm", BARE), ("--match-finder far", BARE), ("--accept some", BARE),
    ("--bogus", BARE), ("--bogus 1", BARE), ("-x", BARE),
]
ORDER = [  # two rules broken at once: the one that stands first answers
    ("--seed-stream %s --greedy-seed 8 --optimal-seed 2" % S, SEED_STREAM), ("--adaptive-seed 2 --optimal-seed 2 --greedy-seed 4", OPTIMAL),
    ("--match-finder frontier --parse-sweep", FINDER), ("--parse-sweep --match-finder frontier --optimal-seed 2", BARE),
    ("--props auto --lc 1 --props-table", PROPS_AUTO), ("--props-table --props-joint 2", BARE), ("--props-joint 2 --cross-grain 8", PROPS_JOINT),
    ("--filter x86 --cross-grain 8", CROSS_GRAIN), ("--filter auto --load-slab x", FILTER_XZ), ("--focus rank --chains 0", FOCUS_RANK),
    ("--format xz --filter auto --load-slab x --focus rank", FILTER_AUTO),
    # the parser goes first, along the command line
    ("--seed-stream %s --load-slab x --dict-size 100" % S, DICT_SIZE), ("--focus 5:5 --dict-size 100", FOCUS), ("--dict-size 100 --focus 5:5", DICT_SIZE),
    ("--cost-bucket 0 --bogus", COST_BUCKET), ("--bogus --cost-bucket 0", BARE),
]
TABLE = RULES + VALUES + ORDER


def run(args):
    return subprocess.run([build.CLI] + args, capture_output=True, timeout=60)


@pytest.fixture(scope="module")
def usage():
    text = run([]).stderr  # no file name: the first rule, which has no message
    assert text.startswith(b"usage: " + build.CLI.encode() + b" [--neighbours K]") and text.endswith(b"(auto, default)\n")
    return text


@pytest.fixture(scope="module")
def infile(tmp_path_factory):
    f = tmp_path_factory.mktemp("cli_args") / "in.txt"
    f.write_bytes(b"hello hello hello")
    return str(f)


def refused(r, message, usage):
    assert r.returncode == 255 and r.stdout == b"" and b"no HIP device" not in r.stderr
    assert r.stderr == (b"Error: " + message.encode() + b"\n" if message else b"") + usage


@pytest.mark.parametrize("line,message", TABLE, ids=[t[0] for t in TABLE])
def test_refusal(usage, infile, line, message):
    refused(run(line.split() + [infile]), message, usage)


@pytest.mark.parametrize("line", ["--cross-grain 8", "--props-table", "--filter x86", "--epochs 1"])
def test_no_file_name_comes_first(usage, line):
    refused(run(line.split()), BARE, usage)


@pytest.mark.parametrize("option", ["--epochs", "--dict-size", "--focus", "--props", "--seed-stream", "-o", "--accept", "--cost-bucket"])
def test_missing_value(usage, infile, option):
    """an option that takes a value, at the end of the line; in front of the file name it takes that as its value and no
    file name is left, except where the value is refused first"""
    refused(run([infile, option]), BARE, usage)
    taken = {"--dict-size": DICT_SIZE, "--focus": FOCUS, "--cost-bucket": COST_BUCKET}.get(option, BARE)
    refused(run([option, infile]), taken, usage)


def test_empty_and_missing_input(tmp_path):
    empty, out = tmp_path / "empty", tmp_path / "out.lzma"
    empty.write_bytes(b"")
    r = run(["-o", str(out), "--epochs", "1", str(empty)])
    assert (r.returncode, r.stdout, r.stderr) == (0, b"", b"") and not out.exists()
    missing = str(tmp_path / "missing")
    r = run(["-o", str(out), missing])
    assert (r.returncode, r.stdout, r.stderr) == (255, b"", b"Error: could not open " + missing.encode() + b"\n") and not out.exists()
