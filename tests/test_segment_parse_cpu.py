"""Segment re-parse without a GPU (mgl_segment_reparse, CLI --segment-reparse): what ties the
restatement of tests/_segment_parse.py to the pieces it is made of and to the host's code -- with one segment at 0/0/0 its
pass is adaptive_rule's, its result is a valid parse whose segment costs the host confirms and whose .xz liblzma decodes --
and what the CLI's front end refuses, in the manner of tests/test_segment_props_cli_cpu.py.  tests/test_gpu_segment_parse.py
holds the device against `segment_rule`."""
import lzma
import subprocess

import pytest

import _segment_parse as R
import _segments as S
import _validity
from megalania_amd import binding, build, corpus
from test_adaptive_rule_cpu import adaptive_rule

DICT = 0x400000


def small_mixed(seed=0x51):
    """1 280 B of prose, then 1 280 B of 4-byte records"""
    return corpus.prose_like(1280, seed) + S.records(1280, seed)


def cut_at(slab, want):
    """the first packet start at or above `want`"""
    return next(p for p in S.walk_starts(slab) if p >= want)


@pytest.fixture(scope="module")
def mixed():
    data = small_mixed()
    return data, S.xz_parse(data)


@pytest.fixture(scope="module")
def two_segments(mixed):
    """from the all-literal slab, cut off the chunk grid: every position is a packet start, and any copy the DP takes is a gain"""
    data = mixed[0]
    slab = binding.literal_slab(len(data))
    segs = [(0, 1300, (3, 0, 0)), (1300, len(data), (0, 2, 2))]
    return slab, segs, R.segment_rule(data, slab, segs, passes=2, chunk=1000)


@pytest.mark.parametrize("segment,ahead", [(64, 128), (1000, 0)])
def test_one_segment_at_000_is_the_adaptive_rule(mixed, segment, ahead):
    """[0, n) at 0/0/0: nothing is re-expressed, the grid starts at 0, and the pass is adaptive_rule's entry for entry"""
    data, slab = mixed
    n = len(data)
    want, objective, _ = adaptive_rule(data, slab, 16, 1000, segment, ahead)
    cost, starts = R.coder_walk(data, S.reexpress(slab, 0, n)[0], 0, n, (0, 0, 0), 1000)
    got = [None] * n
    assert R.segment_pass(data, got, starts, 0, n, (0, 0, 0), 16, 1000, segment, ahead, DICT) == objective
    assert got == want
    assert cost == binding.host_segment_cost(data, slab, 0, n, (0, 0, 0))[0]


def test_two_segments_give_a_valid_parse_the_host_confirms(mixed, two_segments):
    data = mixed[0]
    slab, segs, (out, stats, taken) = two_segments
    print([(st["start_cost"], st["pass_cost"], st["best_pass"], st["final_cost"]) for st in stats], taken)
    assert _validity.violations(data, out, DICT) == []
    starts = S.walk_starts(out)
    for (lo, hi, props), st in zip(segs, stats):
        assert lo in starts and hi in starts
        assert st["start_cost"] == binding.host_segment_cost(data, slab, lo, hi, props)[0]
        assert st["final_cost"] == binding.host_segment_cost(data, out, lo, hi, props)[0]
        assert len(st["pass_cost"]) == len(st["objective"]) == 2
    # the rule's own promises: a strict gain or the input handed back
    total = lambda key: sum(st[key] for st in stats)
    if taken:
        assert total("final_cost") < total("start_cost") and any(st["best_pass"] is not None for st in stats)
    else:
        assert (out == slab).all() and total("final_cost") == total("start_cost")
    # prose that repeats its words offers copies at a fraction of what its literals cost: a shortest path that may take them
    # and may take the literals cannot end above the literals alone, up to what the model learns on the way
    assert taken and stats[0]["best_pass"] is not None
    stream = binding.emit_xz_segments(data, data, out, [dict(lo=lo, hi=hi, props=pr) for lo, hi, pr in segs])
    assert lzma.decompress(stream) == data


def test_join_of_the_input_alone_is_a_valid_parse_of_the_same_cost(mixed):
    """every segment keeping its packets: the join names the same distances again, and no segment's cost moves"""
    data, slab = mixed
    c = cut_at(slab, 700)
    segs = [(0, c, (0, 0, 0)), (c, len(data), (0, 0, 0))]
    out = R.join(slab, segs, [None, None])
    assert _validity.violations(data, out, DICT) == []
    for lo, hi, props in segs:
        assert R.segment_cost(data, out, lo, hi, props) == binding.host_segment_cost(data, slab, lo, hi, props)[0]


# ---- the CLI's front end
NEEDS_SEGMENTS = "--segment-reparse needs --segment-props: it parses the segments that option chooses"
MALFORMED = "--segment-reparse takes a number of passes from 1 to 16"
XZ = ["--format", "xz"]
TABLE = [
    (XZ + ["--segment-reparse", "2"], NEEDS_SEGMENTS), (["--segment-reparse", "16"], NEEDS_SEGMENTS),
    (XZ + ["--segment-reparse", "2", "--match-finder", "frontier"], NEEDS_SEGMENTS),
    (XZ + ["--segment-props", "auto", "--segment-reparse", "0"], MALFORMED), (XZ + ["--segment-props", "auto", "--segment-reparse", "17"], MALFORMED),
    (XZ + ["--segment-reparse", "0"], MALFORMED), (XZ + ["--segment-props", "auto", "--segment-reparse", "x"], MALFORMED),
    (XZ + ["--segment-props", "auto", "--segment-reparse", "-1"], MALFORMED), (XZ + ["--segment-props", "auto", "--segment-reparse", ""], MALFORMED),
    # rules that come earlier keep their answers
    (["--segment-props", "auto", "--segment-reparse", "2"], "--segment-props needs --format xz: an .lzma stream cannot reset its state or change lc/lp/pb"),
]


def run(args):
    return subprocess.run([build.CLI] + args, capture_output=True, timeout=60)


@pytest.fixture(scope="module")
def usage():
    build.build_all()
    text = run([]).stderr
    assert b" [--segment-reparse P] " in text and b"\n  --segment-reparse P  " in text
    assert b"segment-reparse: passes P segments M reparsed R taken 0|1 was X B exact C now X B exact C T ms" in text
    assert b"segment-parse: offset O bytes N lc=.. lp=.. pb=.. start X B exact C best X B exact C pass p|- final X B exact C" in text
    return text


@pytest.mark.parametrize("args,message", TABLE, ids=[" ".join(t[0]) for t in TABLE])
def test_refusal(usage, tmp_path, args, message):
    out = tmp_path / "never_written.xz"
    r = run(args + ["-o", str(out), str(tmp_path / "never_opened.bin")])
    assert r.returncode == 255 and r.stdout == b"" and b"no HIP device" not in r.stderr
    assert r.stderr == b"Error: " + message.encode() + b"\n" + usage
    assert not out.exists()


@pytest.mark.parametrize("value", ["1", "3", "16", "0x10"])
def test_accepted_values_reach_the_input(usage, tmp_path, value):
    for more in ([], ["--match-finder", "frontier", "--mf-depth", "64"], ["--filter", "x86"], ["--adaptive-seed", "1"]):
        r = run(XZ + ["--segment-props", "1024", "--segment-reparse", value] + more + [str(tmp_path / "missing.bin")])
        assert r.returncode == 255 and r.stdout == b"" and usage not in r.stderr and b"--segment-reparse" not in r.stderr
