"""Stream import on the host (no GPU): megalania_amd/host/mgl_host.c reads the parse out of an existing LZMA-alone or
.xz stream of the same input (mgl_stream_import) as a starting slab for the search.  Every stream here is made at
test time -- by the reference's own emission (tests/golden), by ours, or by liblzma through the standard library's
`lzma` module -- so no stream is committed."""
import lzma
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, rand_bytes, sha, slab_from_rle
from megalania_amd import binding, build, corpus

EXTREME = 9 | lzma.PRESET_EXTREME
CHILD_ENV = "MGL_STREAM_IMPORT_ASAN_CHILD"  # set in the sanitizer child: it must not start another one


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.environ.get("MGL_NO_AUTOBUILD"):
        build.build_host()


def alone(data, preset, lc=0, lp=0, pb=0, dict_size=1 << 22):
    return lzma.compress(data, format=lzma.FORMAT_ALONE,
                         filters=[dict(id=lzma.FILTER_LZMA1, preset=preset, dict_size=dict_size, lc=lc, lp=lp, pb=pb)])


def same_slab(a, b):
    return all((a[f] == b[f]).all() for f in ("type", "dist", "len"))


def walk_packets(slab):
    t, d, ln = slab["type"].tolist(), slab["dist"].tolist(), slab["len"].tolist()
    pos, out = 0, []
    while pos < len(ln):
        out.append((t[pos], d[pos], ln[pos]))
        pos += ln[pos]
    return out


_INPUTS = {}


def inp(name) -> bytes:
    if name not in _INPUTS:
        if name == "c5":
            _INPUTS[name] = corpus.config_input("c5")[0][: 256 << 10]
        else:
            _INPUTS[name] = corpus.config_input(name)[0]
    return _INPUTS[name]


def test_reference_streams_import_to_their_walks(golden, golden_input):
    """The reference's own streams (size declared, no end marker) give back exactly the slab they were coded from,
    with nothing re-expressed.  Entries without a stored stream are pinned by its hash."""
    for w in golden["walks"]:
        data = golden_input(w["input"])
        want = slab_from_rle(len(data), w["packets"]).astype(binding.PACKET)
        if "stream_hex" in w:
            stream = bytes.fromhex(w["stream_hex"])
        else:
            stream = binding.emit_stream(data, want)
            assert sha(np.frombuffer(stream, dtype=np.uint8)) == w["stream_sha256"], w["name"]
        info = binding.stream_info(stream)
        assert info == dict(container=binding.CONTAINER_LZMA, lc=0, lp=0, pb=0, dict_size=0x400000,
                            declared_size=len(data)), w["name"]
        slab, st = binding.stream_import(stream, data)
        assert same_slab(slab, want), w["name"]
        assert st["reexpressed"] == 0 and st["clipped"] == 0, (w["name"], st)
        assert st["packets"] == int(w["npackets"]), w["name"]


def test_emit_import_round_trip_covers_every_packet_kind(golden, golden_input):
    seen = set()
    slabs = [(golden_input(w["input"]), slab_from_rle(len(golden_input(w["input"])), w["packets"])) for w in golden["walks"]]
    slabs += [(golden_input(k), slab_from_rle(len(golden_input(k)), v)) for k, v in golden["evolved_walks"].items()]
    for data, slab in slabs:
        slab = slab.astype(binding.PACKET)
        for lc, lp, pb in ((0, 0, 0), (3, 0, 2)):
            got, st = binding.stream_import(binding.emit_stream(data, slab, lc, lp, pb), data)
            assert walk_packets(got) == walk_packets(slab)
            assert st["reexpressed"] == 0
        for t, d, _ in walk_packets(slab):
            seen.add((t, d if t == binding.LONG_REP else None))
    assert {(binding.LONG_REP, j) for j in range(4)} | {(binding.SHORT_REP, None)} <= seen


@pytest.mark.parametrize("name", ["c1", "c2", "c5"])
@pytest.mark.parametrize("preset", [0, 6, EXTREME], ids=["p0", "p6", "p9e"])
@pytest.mark.parametrize("lc,lp,pb", [(0, 0, 0), (3, 0, 2), (0, 4, 4)])
def test_liblzma_alone_streams(name, preset, lc, lp, pb):
    """liblzma's parse re-emitted at the stream's properties is liblzma's stream up to the final flush (ours has no
    end marker), so the seed is never longer than what xz wrote."""
    data = inp(name)
    xs = alone(data, preset, lc, lp, pb)
    info = binding.stream_info(xs)
    assert info == dict(container=binding.CONTAINER_LZMA, lc=lc, lp=lp, pb=pb, dict_size=1 << 22, declared_size=None)
    slab, st = binding.stream_import(xs, data)
    assert st["reexpressed"] == 0 and st["clipped"] == 0
    assert st["packets"] == st["literals"] + st["matches"] + st["short_reps"] + sum(st["long_reps"])
    ours = binding.emit_stream(data, slab, lc, lp, pb)
    assert lzma.decompress(ours, format=lzma.FORMAT_ALONE) == data
    k = len(ours) - 5
    while k > 13 and ours[k - 1] == 0xFF:
        k -= 1
    assert ours[13:k] == xs[13:k]
    assert len(ours) <= len(xs)


@pytest.mark.parametrize("check", [lzma.CHECK_NONE, lzma.CHECK_CRC32, lzma.CHECK_CRC64, lzma.CHECK_SHA256])
def test_xz_checks(check):
    data = inp("c2")
    xs = lzma.compress(data, format=lzma.FORMAT_XZ, check=check, preset=EXTREME)
    info = binding.stream_info(xs)
    assert info["container"] == binding.CONTAINER_XZ and info["declared_size"] == len(data)
    assert (info["lc"], info["lp"], info["pb"]) == (3, 0, 2) and info["dict_size"] == 64 << 20
    slab, st = binding.stream_import(xs, data)
    assert st["props_changes"] == 0
    for lc, lp, pb in ((0, 0, 0), (3, 0, 2)):
        assert lzma.decompress(binding.emit_stream(data, slab, lc, lp, pb), format=lzma.FORMAT_ALONE) == data
    # one block, one stream: the same parse as liblzma's LZMA-alone coder at the same settings
    ref, _ = binding.stream_import(alone(data, EXTREME, 3, 0, 2, 64 << 20), data)
    assert same_slab(slab, ref)


def test_xz_concatenated_streams():
    data = inp("c2")
    xs = lzma.compress(data, format=lzma.FORMAT_XZ, preset=EXTREME)
    both = xs + b"\0" * 8 + xs  # stream padding between the two
    assert binding.stream_info(both)["declared_size"] == 2 * len(data)
    slab, st = binding.stream_import(both, data + data)
    assert lzma.decompress(binding.emit_stream(data + data, slab), format=lzma.FORMAT_ALONE) == data + data
    # the second stream starts a fresh dictionary: none of its copies reach into the first half
    for pos in range(len(data), 2 * len(data)):
        if slab[pos]["type"] == binding.MATCH:
            assert int(slab[pos]["dist"]) < pos - len(data)
    with pytest.raises(binding.MglError):
        binding.stream_import(both, data)  # more stream than input
    with pytest.raises(binding.MglError):
        binding.stream_import(xs, data + data)  # less


def test_xz_uncompressed_and_several_lzma_chunks():
    """A random middle makes liblzma write uncompressed LZMA2 chunks (after which an LZMA chunk resets the state, so
    that the stream's rep stack and ours differ); text that codes to more than 64 KiB on either side, LZMA chunks that
    carry the state over."""
    text = corpus.enwik_like(600_000, 0x302)
    data = text[:300_000] + rand_bytes(300 << 10, 0x301) + text[250_000:]
    xs = lzma.compress(data, format=lzma.FORMAT_XZ, preset=EXTREME)
    # the chunk kinds this is about are really there
    ctl, at = [], 12 + (xs[12] + 1) * 4
    while xs[at] != 0:
        c = xs[at]
        ctl.append(c)
        at += 3 + ((xs[at + 1] << 8 | xs[at + 2]) + 1) if c < 0x80 else 5 + (c >= 0xC0) + ((xs[at + 3] << 8 | xs[at + 4]) + 1)
    assert any(c in (1, 2) for c in ctl) and any(0x80 <= c < 0xA0 for c in ctl) and any(0xA0 <= c < 0xC0 for c in ctl), ctl
    slab, st = binding.stream_import(xs, data)
    assert lzma.decompress(binding.emit_stream(data, slab), format=lzma.FORMAT_ALONE) == data
    assert st["literals"] >= 300 << 10 and st["clipped"] == 0


def test_xz_bcj_is_refused():
    data = inp("c5")
    xs = lzma.compress(data, format=lzma.FORMAT_XZ, filters=[dict(id=lzma.FILTER_X86), dict(id=lzma.FILTER_LZMA2, preset=6)])
    with pytest.raises(binding.MglError) as e:
        binding.stream_import(xs, data)
    assert e.value.rc == -1 and "BCJ" in e.value.error
    with pytest.raises(binding.MglError):
        binding.stream_info(xs)


def _far_input():
    key = rand_bytes(64 << 10, 0x6B)
    return key + corpus.enwik_like(5 << 20, 0x5A) + key


def test_window():
    """Copies beyond the 4 MiB window: an error, or literals under clipping.  (The text itself repeats from farther
    than 4 MiB, so the first such copy lies inside it, past 4 MiB; the key's second copy is one of them.)"""
    data = _far_input()
    xs = alone(data, 1, dict_size=8 << 20)
    with pytest.raises(binding.MglError) as e:
        binding.stream_import(xs, data)
    assert e.value.rc == -4 and e.value.error_pos >= 0x400000
    slab, st = binding.stream_import(xs, data, clip=True)
    assert st["clipped"] > 0
    assert walk_packets(slab)[-1] == (binding.LITERAL, 0, 1)  # the key's second copy came back as literals
    stream = binding.emit_stream(data, slab)  # refuses any distance outside the window
    assert lzma.decompress(stream, format=lzma.FORMAT_ALONE) == data
    # a smaller window clips more; nothing out of window: clipping changes nothing
    _, st2 = binding.stream_import(xs, data, window=1 << 20, clip=True)
    assert st2["clipped"] > st["clipped"]
    c2 = inp("c2")
    x2 = alone(c2, EXTREME)
    a, sa = binding.stream_import(x2, c2)
    b, sb = binding.stream_import(x2, c2, clip=True)
    assert same_slab(a, b) and sa == sb


def test_bad_input():
    data = inp("c2")
    xs = alone(data, EXTREME)
    # a byte of the input that the stream does not reproduce: named by position
    for at in (0, 777, 50_000, len(data) - 1):
        other = bytearray(data)
        other[at] ^= 0x20
        with pytest.raises(binding.MglError) as e:
            binding.stream_import(xs, bytes(other))
        assert e.value.rc == -1 and e.value.error_pos == at, (at, e.value.error, e.value.error_pos)
    for cut in (1, 5, 13, len(xs) // 2, len(xs) - 1):
        with pytest.raises(binding.MglError) as e:
            binding.stream_import(xs[:cut], data)
        assert e.value.rc == -1, cut
    for off in np.linspace(13, len(xs) - 1, 8).astype(int):
        bad = bytearray(xs)
        bad[off] ^= 0x10
        with pytest.raises(binding.MglError) as e:
            binding.stream_import(bytes(bad), data)
        assert e.value.rc == -1 and 0 <= e.value.error_pos <= len(data), off
    for props in (225, 255):
        with pytest.raises(binding.MglError):
            binding.stream_import(bytes([props]) + xs[1:], data)
        with pytest.raises(binding.MglError):
            binding.stream_info(bytes([props]) + xs[1:])
    # a declared size other than the input's
    ref = binding.emit_stream(data, binding.literal_slab(len(data)))
    with pytest.raises(binding.MglError):
        binding.stream_import(ref, data[:-1])
    with pytest.raises(binding.MglError):
        binding.stream_import(ref, data + b"x")
    # trailing bytes after the declared size / the end marker are ignored
    assert binding.stream_import(ref + b"\x01\x02\x03", data)[1]["packets"] == len(data)
    binding.stream_import(xs + b"trailing", data)
    # the .xz container: truncations and flips anywhere
    xz = lzma.compress(data[:20_000], format=lzma.FORMAT_XZ, preset=6)
    for cut in (1, 6, 12, 20, len(xz) // 2, len(xz) - 12, len(xz) - 1):
        with pytest.raises(binding.MglError):
            binding.stream_import(xz[:cut], data[:20_000])
    for off in np.linspace(0, len(xz) - 1, 24).astype(int):
        bad = bytearray(xz)
        bad[off] ^= 0x41
        try:
            binding.stream_import(bytes(bad), data[:20_000])
        except binding.MglError:
            pass  # refused, or (a flipped check / CRC) accepted: never a crash


def test_under_asan_and_ubsan():
    """This file once more in a child interpreter against the sanitizer build of the host library (the way
    tests/test_sanitizers.py runs the golden walks)."""
    if os.environ.get(CHILD_ENV):
        return  # the child itself: nothing to nest
    rt = {}
    for name in ("libasan.so", "libubsan.so"):
        p = subprocess.run(["gcc", "-print-file-name=" + name], capture_output=True, text=True).stdout.strip()
        rt[name] = p if os.path.isabs(p) and os.path.exists(p) else None
    if not all(rt.values()):
        pytest.skip("gcc's sanitizer runtimes are not installed")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "sanitizers"], stdout=sys.stderr)
    env = dict(os.environ,
               LD_PRELOAD=":".join(p for p in (rt["libasan.so"], rt["libubsan.so"], os.environ.get("LD_PRELOAD")) if p),
               ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1",
               MGL_HOST_SO=os.path.join(ROOT, "oracle", "_build", "libmegalania_host_asan.so"),
               MGL_NO_AUTOBUILD="1", **{CHILD_ENV: "1"})
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", "-m", "not gpu",
                        "--deselect", "tests/test_stream_import.py::test_under_asan_and_ubsan",
                        os.path.join(ROOT, "tests", "test_stream_import.py")],
                       env=env, capture_output=True, text=True, timeout=1500, cwd=ROOT)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "passed" in r.stdout and "AddressSanitizer" not in tail and "runtime error" not in tail, tail
