"""The .xz writer of the host library (mgl_emit_xz), the dictionary size of both containers and the opt-in import of
[x86, LZMA2] streams, without a GPU: the parses come out of liblzma's own streams through binding.stream_import, and
liblzma (the standard library's `lzma` module, and /usr/bin/xz where it exists) is the decoder of what is written."""
import lzma
import os
import shutil
import subprocess
import zlib

import pytest

from conftest import ROOT, rand_bytes
from megalania_amd import binding, build, corpus

MIB = 1 << 20
XZ = shutil.which("xz") or ("/usr/bin/xz" if os.path.exists("/usr/bin/xz") else None)


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build_host()


def alone(data, preset, dict_size=1 << 22):
    return lzma.compress(data, format=lzma.FORMAT_ALONE,
                         filters=[dict(id=lzma.FILTER_LZMA1, preset=preset, dict_size=dict_size, lc=0, lp=0, pb=0)])


def elf_slice(at=512 << 10, n=16384) -> bytes:
    return corpus.elf1m()[0][at:at + n]


def same_slab(a, b):
    return all((a[f] == b[f]).all() for f in ("type", "dist", "len"))


def varint(x, at):
    v = shift = 0
    while True:
        b = x[at]
        at += 1
        v |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            return v, at


def walk_xz(x: bytes) -> dict:
    """Every field of a one-stream, at most one-block .xz, each checked on the way; the chunks as (control, usize, csize)."""
    le = lambda p, k=4: int.from_bytes(x[p:p + k], "little")  # noqa: E731
    assert x[:6] == b"\xFD7zXZ\x00" and x[6] == 0 and x[7] in (0, 1)
    check = x[7]
    assert le(8) == zlib.crc32(x[6:8])
    at, out = 12, dict(check=check, chunks=[], filter_flags=None, usize=0)
    if x[at] != 0:
        hsize = (x[at] + 1) * 4
        h = x[at:at + hsize]
        assert le(at + hsize - 4) == zlib.crc32(h[:-4])
        assert h[1] in (0, 1)  # number of filters - 1, no size fields
        flags = h[2:2 + (5 if h[1] else 3)]
        assert not any(h[2 + len(flags):-4])  # zero padding
        out.update(filter_flags=bytes(flags), header=hsize)
        p = at + hsize
        while x[p] != 0:
            c = x[p]
            assert c >= 0x80
            usize = ((c & 0x1F) << 16 | x[p + 1] << 8 | x[p + 2]) + 1
            csize = (x[p + 3] << 8 | x[p + 4]) + 1
            out["chunks"].append((c, usize, csize))
            p += 5 + (1 if c >= 0xC0 else 0) + csize
        p += 1
        data_size = p - (at + hsize)
        while (p - at) % 4:
            assert x[p] == 0
            p += 1
        out.update(unpadded_seen=hsize + data_size + 4 * check, crc=le(p) if check else None)
        at = p + 4 * check
    istart = at
    assert x[at] == 0
    nrec, at = varint(x, at + 1)
    assert nrec == len(out["chunks"][:1])
    if nrec:
        out["unpadded"], at = varint(x, at)
        out["usize"], at = varint(x, at)
    while (at - istart) % 4:
        assert x[at] == 0
        at += 1
    assert le(at) == zlib.crc32(x[istart:at])
    at += 4
    assert le(at) == zlib.crc32(x[at + 4:at + 10])
    assert (le(at + 4) + 1) * 4 == at - istart  # backward size
    assert x[at + 8:at + 12] == bytes([0, check]) + b"YZ"
    assert at + 12 == len(x)
    return out


_CASES = {}


def case(name):
    """(original, coded, slab, filter) of the larger inputs, each made once."""
    if name not in _CASES:
        if name == "rand":  # incompressible: the chunks close on their compressed size
            d = rand_bytes(160 << 10, 0x5A7)
            _CASES[name] = (d, d, binding.literal_slab(len(d)), 0)
        elif name == "rep":  # 273-byte block repeated: liblzma tiles it with rep matches, which the 2 MiB marks do not divide
            block = rand_bytes(273, 0x111)
            d = (block * (5 * MIB // 273 + 1))[:5 * MIB]
            _CASES[name] = (d, d, binding.stream_import(alone(d, 1), d)[0], 0)
        elif name == "small":
            d = elf_slice()[4000:4300]
            _CASES[name] = (d, d, binding.stream_import(alone(d, 6), d)[0], 0)
        elif name == "elf-x86":
            d = elf_slice()
            c = binding.bcj_x86(d)
            _CASES[name] = (d, c, binding.stream_import(alone(c, 6), c)[0], 4)
        elif name == "far":  # tests/test_stream_import.py's: the key comes back from 5 MiB away
            key = rand_bytes(64 << 10, 0x6B)
            d = key + corpus.enwik_like(5 << 20, 0x5A) + key
            _CASES[name] = (d, d, binding.stream_import(alone(d, 1, dict_size=8 * MIB), d, window=8 * MIB)[0], 0)
    return _CASES[name]


def xz_accepts(tmp_path, x: bytes, want: bytes):
    if XZ is None:
        pytest.skip("no xz program")
    f = tmp_path / "t.xz"
    f.write_bytes(x)
    assert subprocess.run([XZ, "-t", str(f)], capture_output=True, timeout=60).returncode == 0
    r = subprocess.run([XZ, "-dc", str(f)], capture_output=True, timeout=60)
    assert r.returncode == 0 and r.stdout == want


def test_xz_roundtrip_small(tmp_path):
    src = elf_slice()[4000:4300]  # holds calls: the filter changes bytes of it
    assert binding.bcj_x86(src) != src
    for n in (0, 1, 5, 300):
        d = src[:n]
        for flt in (0, 4):
            coded = binding.bcj_x86(d) if flt else d
            slabs = [binding.literal_slab(n)]
            if n == 300:
                slabs.append(binding.stream_import(alone(coded, 6), coded)[0])
                assert (slabs[1]["type"] != binding.LITERAL).any()
            for slab in slabs:
                for check in (0, 1):
                    x = binding.emit_xz(d, coded, slab, filter=flt, check=check)
                    assert lzma.decompress(x) == d, (n, flt, check)
                    xz_accepts(tmp_path, x, d)
    # lc/lp/pb travel in the first chunk
    d = src
    x = binding.emit_xz(d, d, binding.literal_slab(len(d)), lc=3, lp=0, pb=2)
    assert lzma.decompress(x) == d and binding.stream_info(x)["lc"] == 3 and binding.stream_info(x)["pb"] == 2
    with pytest.raises(binding.MglError):
        binding.emit_xz(d, d, binding.literal_slab(len(d)), filter=3)
    with pytest.raises(binding.MglError):  # without a filter the coded bytes are the original
        binding.emit_xz(d, binding.bcj_x86(d), binding.literal_slab(len(d)), filter=0)


def test_xz_layout():
    for name, check in (("small", 1), ("small", 0), ("elf-x86", 1), ("rand", 1), ("rep", 1)):
        d, c, slab, flt = case(name)
        x = binding.emit_xz(d, c, slab, filter=flt, check=check)
        w = walk_xz(x)
        assert w["check"] == check
        assert w["filter_flags"] == (b"\x04\x00" if flt else b"") + b"\x21\x01\x14"  # 0x14 = 20: 2 << (10 + 11) = 4 MiB
        ctl = [k[0] for k in w["chunks"]]
        assert ctl[0] >= 0xE0 and all(0x80 <= k < 0xA0 for k in ctl[1:])
        assert all(u <= 2 * MIB and cs <= 64 << 10 for _, u, cs in w["chunks"])
        assert sum(u for _, u, _ in w["chunks"]) == w["usize"] == len(d)
        assert w["unpadded"] == w["unpadded_seen"]  # header + chunks + end byte + check
        if check:
            assert w["crc"] == zlib.crc32(d)
    w = walk_xz(binding.emit_xz(b"", b"", binding.literal_slab(0)))
    assert w["chunks"] == [] and w["filter_flags"] is None  # no block


def test_compressed_chunk_limit():
    d, c, slab, _ = case("rand")
    x = binding.emit_xz(d, c, slab)
    w = walk_xz(x)
    assert len(w["chunks"]) > 2 and all(cs <= 64 << 10 for _, _, cs in w["chunks"])
    # a packet's worst case is 70 bytes: no chunk was closed earlier than that before the limit
    assert all(cs > (64 << 10) - 70 - 5 for _, _, cs in w["chunks"][:-1])
    assert lzma.decompress(x) == d
    # only the first chunk resets anything, so the model ran on across the cuts
    got, st = binding.stream_import(x, d)
    assert same_slab(got, slab) and st["props_changes"] == 0 and st["reexpressed"] == 0


def test_uncompressed_chunk_limit():
    d, c, slab, _ = case("rep")
    assert (slab["type"] == binding.LONG_REP).sum() > 1000
    x = binding.emit_xz(d, c, slab)
    w = walk_xz(x)
    us = [u for _, u, _ in w["chunks"]]
    assert len(us) >= 3 and max(us) <= 2 * MIB and sum(us) == len(d)
    assert any(u < 2 * MIB for u in us[:-1])  # a packet straddled a 2 MiB mark and was kept whole
    assert lzma.decompress(x) == d


def test_xz_size_against_lzma():
    """len(xz) <= len(lzma) + 53 + 11 * (chunks - 1).

    The .lzma stream is 13 header bytes, the range coder's bytes and its 5 flush bytes.  The .xz stream with a CRC32
    check holds, around the first chunk's range coder bytes (flush included): stream header 12, block header 12 (size,
    flags, at most 7 bytes of filter flags, padded to 8, CRC32), first chunk header 6, end byte 1, block padding at most
    3, check 4, index at most 16 (indicator, count, at most 3 + 4 bytes of sizes for these inputs, padded to 12, CRC32),
    footer 12: 66 in all, against the 13 it replaces: + 53.  (The issue's "- 13 + 53" counts the 13 twice: its own list of
    parts sums to 66.)  Every further chunk costs its 5-byte header and a range coder of its own, whose first byte is
    the zero it starts with and whose flush is 5 bytes: 11.  A fresh coder starts from the full range, which is never
    smaller than the running one's, so the cut itself adds no byte beyond those."""
    for name in ("small", "elf-x86", "rand", "rep"):
        d, c, slab, flt = case(name)
        x = binding.emit_xz(d, c, slab, filter=flt, check=1)
        chunks = len(walk_xz(x)["chunks"])
        ref = binding.emit_stream(c, slab)
        assert len(x) <= len(ref) + 53 + 11 * (chunks - 1), (name, len(x), len(ref), chunks)


def test_dict_size_declared_and_enforced():
    d, c, slab, _ = case("far")
    far = slab["dist"][slab["type"] == binding.MATCH].max()
    assert 4 * MIB <= far < 8 * MIB
    s = binding.emit_stream_dict(d, slab, 8 * MIB)
    assert binding.stream_info(s)["dict_size"] == 8 * MIB and lzma.decompress(s, format=lzma.FORMAT_ALONE) == d
    x = binding.emit_xz(d, c, slab, dict_size=8 * MIB)
    assert binding.stream_info(x)["dict_size"] == 8 * MIB and lzma.decompress(x) == d
    for refuse in (lambda: binding.emit_stream(d, slab), lambda: binding.emit_xz(d, c, slab),
                   lambda: binding.emit_stream_dict(d, slab, 0), lambda: binding.emit_stream_dict(d, slab, 4 * MIB),
                   lambda: binding.emit_stream_dict(d, slab, int(far))):  # a 0-based distance `far` reaches far + 1 bytes back
        with pytest.raises(binding.MglError):
            refuse()
    assert lzma.decompress(binding.emit_stream_dict(d, slab, int(far) + 1), format=lzma.FORMAT_ALONE) == d
    # with everything inside 4 MiB, emit_stream_dict at the default is emit_stream
    sd, _, ss, _ = case("small")
    assert binding.emit_stream_dict(sd, ss, 0) == binding.emit_stream(sd, ss) == binding.emit_stream_dict(sd, ss, 4 * MIB)
    assert binding.stream_info(binding.emit_stream_dict(sd, ss, 4096))["dict_size"] == 4096
    # .xz names 2^n and 3 * 2^(n-1) only: the next one up, and never below 4 KiB
    for ask, get in ((6 * MIB, 6 * MIB), (5 * MIB, 6 * MIB), (4 * MIB + 1, 6 * MIB), (0, 4 * MIB), (4096, 4096), (1, 4096),
                     (4097, 6144), (64 * MIB, 64 * MIB)):
        x = binding.emit_xz(sd, sd, ss, dict_size=ask)
        assert binding.stream_info(x)["dict_size"] == get, ask
        assert lzma.decompress(x) == sd


def test_import_x86_stream():
    d = elf_slice()
    f = binding.bcj_x86(d)
    xs = lzma.compress(d, format=lzma.FORMAT_XZ, filters=[dict(id=lzma.FILTER_X86), dict(id=lzma.FILTER_LZMA2, preset=6)])
    with pytest.raises(binding.MglError) as e:
        binding.stream_import(xs, d)
    assert e.value.rc == -1 and "BCJ" in e.value.error
    with pytest.raises(binding.MglError) as e:
        binding.stream_import(xs, f)  # the filtered bytes do not help without the flag
    assert "BCJ" in e.value.error
    with pytest.raises(binding.MglError):
        binding.stream_info(xs)
    slab, st = binding.stream_import(xs, f, x86=True)
    assert st["matches"] > 0
    assert lzma.decompress(binding.emit_xz(d, f, slab, filter=4)) == d
    info = binding.stream_info_x(xs)
    assert info["filter"] == 4 and info["declared_size"] == len(d) and info["container"] == binding.CONTAINER_XZ
    with pytest.raises(binding.MglError) as e:
        binding.stream_import(xs, d, x86=True)
    assert "decoded byte differs" in e.value.error
    # a plain chain and an .lzma stream report no filter, and the flag changes nothing for them
    plain = lzma.compress(d, format=lzma.FORMAT_XZ, preset=6)
    assert binding.stream_info_x(plain)["filter"] == 0 and binding.stream_info_x(alone(d, 6))["filter"] == 0
    assert same_slab(binding.stream_import(plain, d, x86=True)[0], binding.stream_import(plain, d)[0])
    # every other chain stays refused: a start offset, another BCJ filter, delta
    for chain in ([dict(id=lzma.FILTER_X86, start_offset=16)], [dict(id=lzma.FILTER_ARM)], [dict(id=lzma.FILTER_DELTA, dist=1)],
                  [dict(id=lzma.FILTER_DELTA, dist=1), dict(id=lzma.FILTER_X86)]):
        other = lzma.compress(d, format=lzma.FORMAT_XZ, filters=chain + [dict(id=lzma.FILTER_LZMA2, preset=6)])
        with pytest.raises(binding.MglError):
            binding.stream_import(other, f, x86=True)
        with pytest.raises(binding.MglError):
            binding.stream_info_x(other)


def test_host_paths_under_sanitizers(tmp_path):
    """tests/xz_sanitizer_main.c with the host library's source under AddressSanitizer and UBSan, as a child process."""
    cc = os.environ.get("CC", "gcc")
    flags = ["-std=gnu11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-static-libasan", "-static-libubsan"]
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    if subprocess.run([cc] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler cannot link the sanitizer runtimes")
    exe = tmp_path / "xz_sanitizer"
    subprocess.run([cc] + flags + ["-Wall", "-Wextra", "-o", str(exe), os.path.join(ROOT, "tests", "xz_sanitizer_main.c"),
                                   os.path.join(ROOT, "megalania_amd", "host", "mgl_host.c")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0 and r.stdout.strip() == "ok", tail
    assert "AddressSanitizer" not in tail and "runtime error" not in tail, tail


@pytest.mark.parametrize("args,why", [
    (["--filter", "x86"], b"--format xz"),
    (["--filter", "auto"], b"--format xz"),
    (["--format", "xz", "--filter", "auto", "--load-slab", "some.slab"], b"--filter auto cannot be combined"),
    (["--format", "xz", "--filter", "auto", "--seed-stream", "some.xz"], b"--filter auto cannot be combined"),
    (["--format", "xz", "--filter", "auto", "--chains", "2", "--rank", "0", "--comm-file", "some.comm"], b"--filter auto cannot be combined"),
    (["--dict-size", "4095"], b"--dict-size"),
    (["--dict-size", "4k"], b"--dict-size"),
    (["--format", "7z"], b"usage:"),
    (["--format", "xz", "--filter", "arm"], b"usage:"),
])
def test_cli_refuses_before_it_touches_a_device(args, why, tmp_path):
    build.build_all()
    f = tmp_path / "in.bin"
    f.write_bytes(corpus.prose_like(64, 1))
    r = subprocess.run([build.CLI] + args + [str(f)], capture_output=True, timeout=60, cwd=str(tmp_path))
    assert r.returncode != 0 and r.stdout == b""
    assert why in r.stderr and b"usage:" in r.stderr and b"no HIP device" not in r.stderr
    assert not os.path.exists(tmp_path / "some.comm")
    usage = subprocess.run([build.CLI], capture_output=True, timeout=60).stderr
    assert b"--format lzma|xz" in usage and b"--filter none|x86|auto" in usage and b"--dict-size BYTES" in usage and b"same filter" in usage
