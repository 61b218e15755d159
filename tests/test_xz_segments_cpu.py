"""The .xz writer with a triple per segment (mgl_emit_xz_segments) without a device: on an input whose
halves want different lc/lp/pb, the partition found with the host functions is written, decoded by the standard library and
by xz, and compared with the best single-triple stream."""
import lzma
import os
import shutil
import subprocess

import pytest

import _segments as S
from conftest import ROOT
from megalania_amd import binding, build

GRAIN = 1024


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build_hip()
    build.build_host()


@pytest.fixture(scope="module")
def case():
    """input, slab, cuts, the host's span table, the partition and the best single triple"""
    data = S.mixed_input()
    slab = S.xz_parse(data)
    cuts = S.grain_cuts(slab, GRAIN)
    tab = S.host_table(data, slab, cuts)
    segs, total = binding.segment_partition(tab, cuts)
    m = len(cuts) - 1
    whole = [int(c) for c in tab[S.span_index(0, m, m)]]
    single = min(whole)
    return dict(data=data, slab=slab, cuts=cuts, tab=tab, segs=segs, total=total, single=single,
                single_props=binding.PROPS_TRIPLES[whole.index(single)])


def test_the_input_pays_for_segments(case):
    """what the other tests rely on: two segments at least, cheaper than the best one triple even with the overheads"""
    assert len(case["segs"]) >= 2 and case["total"] < case["single"]
    assert (S.as_tuples(case["segs"]), case["total"]) == S.partition(case["tab"], case["cuts"], binding.SEG_OVERHEAD)
    assert len({tuple(s["props"]) for s in case["segs"]}) >= 2
    for s in case["segs"]:  # each segment's figure is the host's exact cost under its triple
        assert s["cost"] == binding.host_segment_cost(case["data"], case["slab"], s["lo"], s["hi"], s["props"])[0]


def test_segmented_stream_decodes_and_is_shorter(case):
    data, slab, segs = case["data"], case["slab"], case["segs"]
    stream = binding.emit_xz_segments(data, data, slab, segs)
    assert lzma.decompress(stream) == data
    if shutil.which("xz"):
        r = subprocess.run(["xz", "-dc"], input=stream, capture_output=True, timeout=60)
        assert r.returncode == 0 and r.stdout == data, r.stderr
    one = binding.emit_xz(data, data, slab, *case["single_props"])
    assert lzma.decompress(one) == data
    assert len(stream) < len(one)
    # the estimate holds: the chunks' coded bytes are the exact cost, give or take each chunk's 5 flush bytes and the 1 % that
    # a price table of 1/2048 bit over 11-bit probabilities can be off by against the coder's 32-bit range
    chunks = S.lzma2_chunks(stream)
    coded = sum(c[3] for c in chunks)
    exact = sum(s["cost"] for s in segs)
    assert abs(coded - exact / 16384) <= 5 * len(chunks) + coded // 100
    # the importer reads it back as a parse of the same bytes, and counts the props changes
    back, st = binding.stream_import(stream, data)
    assert st["props_changes"] == sum(tuple(s["props"]) != tuple(segs[0]["props"]) for s in segs[1:])
    assert binding.emit_xz(data, data, back, *case["single_props"]) is not None


def test_chunk_walk_shows_the_resets(case):
    data, slab, segs = case["data"], case["slab"], case["segs"]
    chunks = S.lzma2_chunks(binding.emit_xz_segments(data, data, slab, segs))
    pos, k = 0, 0
    for idx, (ctl, props, usize, csize) in enumerate(chunks):
        if idx == 0:
            assert ctl == 0xE0 and props == S.props_byte(segs[0]["props"]) and pos == segs[0]["lo"] == 0
        elif pos == segs[k]["hi"]:
            k += 1
            assert ctl == 0xC0 and props == S.props_byte(segs[k]["props"]) and pos == segs[k]["lo"]
        else:
            assert ctl == 0x80 and props is None
        pos += usize
        assert pos <= segs[k]["hi"]  # a chunk never crosses a segment's end
    assert pos == len(data) and k == len(segs) - 1


def test_reset_chunk_is_written_where_the_triple_repeats_and_chunks_split_inside_segments(case):
    """every leaf its own segment under one triple: 0xC0 at every cut all the same; random bytes make chunks end inside segments"""
    data, slab, cuts = case["data"], case["slab"], case["cuts"]
    segs = [dict(lo=a, hi=b, props=(0, 0, 0)) for a, b in zip(cuts, cuts[1:])]
    stream = binding.emit_xz_segments(data, data, slab, segs)
    assert lzma.decompress(stream) == data
    chunks = S.lzma2_chunks(stream)
    assert [c[0] for c in chunks] == [0xE0] + [0xC0] * (len(segs) - 1) and all(c[1] == 0 for c in chunks)
    assert [c[2] for c in chunks] == [b - a for a, b in zip(cuts, cuts[1:])]
    from conftest import rand_bytes
    big = rand_bytes(150_000, 5) + data
    lit = binding.literal_slab(len(big))
    lit[150_000:] = slab  # the mixed input's parse behind 150 000 literals: its copies stay inside it
    cut = 150_000 + cuts[2]
    segs = [dict(lo=0, hi=cut, props=(0, 0, 0)), dict(lo=cut, hi=len(big), props=(0, 2, 2))]
    stream = binding.emit_xz_segments(big, big, lit, segs)
    assert lzma.decompress(stream) == big
    ctl = [c[0] for c in S.lzma2_chunks(stream)]
    assert ctl[0] == 0xE0 and ctl.count(0xC0) == 1 and ctl.count(0x80) >= 2 and ctl[-1] == 0xC0


def test_one_segment_is_mgl_emit_xz_byte_for_byte(case):
    data, slab = case["data"], case["slab"]
    for pr in [(0, 0, 0), (3, 0, 2), (0, 2, 2), (1, 3, 4)]:
        for kw in (dict(), dict(check=0), dict(dict_size=1 << 16)):
            assert binding.emit_xz_segments(data, data, slab, [dict(lo=0, hi=len(data), props=pr)], **kw) == \
                binding.emit_xz(data, data, slab, *pr, **kw)


def test_filtered_bytes_check_is_over_the_original(case):
    """--filter x86: the LZMA layer sees the filtered bytes, the block check covers the original ones"""
    code = bytearray(case["data"])
    for at in range(16, 4000, 64):  # calls whose operands the filter changes
        code[at:at + 5] = bytes([0xE8, at & 0xFF, (at >> 8) & 0xFF, 0, 0])
    original = bytes(code)
    coded = binding.bcj_x86(original)
    assert coded != original
    slab = S.xz_parse(coded)
    cuts = S.grain_cuts(slab, 2048)
    segs = [dict(lo=a, hi=b, props=pr) for (a, b), pr in zip(zip(cuts, cuts[1:]), [(3, 0, 2), (0, 0, 0), (0, 2, 2), (1, 1, 1)])]
    stream = binding.emit_xz_segments(original, coded, slab, segs, filter=binding.FILTER_X86)
    assert lzma.decompress(stream) == original  # liblzma verifies the CRC32 against what it hands out
    assert binding.stream_info_x(stream)["filter"] == 4
    assert len(S.lzma2_chunks(stream)) == len(segs)
    with pytest.raises(binding.MglError):  # without a filter the coded bytes must be the original ones
        binding.emit_xz_segments(original, coded, slab, segs)


def test_segments_that_do_not_tile_are_refused(case):
    data, slab, cuts = case["data"], case["slab"], case["cuts"]
    n = len(data)
    starts = set(S.walk_starts(slab))
    off = next(p for p in range(cuts[1], n) if p not in starts)
    a = cuts[1]
    for segs in ([dict(lo=0, hi=a, props=(0, 0, 0))],                                                     # stops short
                 [dict(lo=0, hi=a, props=(0, 0, 0)), dict(lo=a + 0, hi=n - 1, props=(0, 0, 0))],         # ends before n
                 [dict(lo=0, hi=a, props=(0, 0, 0)), dict(lo=cuts[2], hi=n, props=(0, 0, 0))],           # a gap
                 [dict(lo=0, hi=cuts[2], props=(0, 0, 0)), dict(lo=a, hi=n, props=(0, 0, 0))],           # an overlap
                 [dict(lo=a, hi=n, props=(0, 0, 0)), dict(lo=0, hi=a, props=(0, 0, 0))],                 # out of order
                 [dict(lo=0, hi=off, props=(0, 0, 0)), dict(lo=off, hi=n, props=(0, 0, 0))],             # a cut inside a packet
                 [dict(lo=0, hi=a, props=(0, 0, 0)), dict(lo=a, hi=a, props=(0, 0, 0)), dict(lo=a, hi=n, props=(0, 0, 0))],  # empty
                 [dict(lo=0, hi=a, props=(0, 0, 0)), dict(lo=a, hi=n, props=(3, 2, 0))],                 # lc + lp > 4
                 []):
        with pytest.raises(binding.MglError):
            binding.emit_xz_segments(data, data, slab, segs)
    assert binding.emit_xz_segments(b"", b"", binding.literal_slab(0), []) == binding.emit_xz(b"", b"", binding.literal_slab(0))


def test_segment_paths_under_sanitizers(tmp_path):
    """tests/segments_sanitizer_main.c with the host library's source under AddressSanitizer and UBSan, as a child process."""
    cc = os.environ.get("CC", "gcc")
    flags = ["-std=gnu11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-static-libasan", "-static-libubsan"]
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    if subprocess.run([cc] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler cannot link the sanitizer runtimes")
    exe = tmp_path / "segments_sanitizer"
    subprocess.run([cc] + flags + ["-Wall", "-Wextra", "-o", str(exe), os.path.join(ROOT, "tests", "segments_sanitizer_main.c"),
                                   os.path.join(ROOT, "megalania_amd", "host", "mgl_host.c")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0 and r.stdout.strip() == "ok", tail
    assert "AddressSanitizer" not in tail and "runtime error" not in tail, tail
