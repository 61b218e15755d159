"""The x86 branch/call/jump filter of the host library (mgl_bcj_x86, no GPU) against liblzma's.  The standard library's
raw coder needs a compressor as the last filter, so liblzma's filtered bytes are what an LZMA2-only raw decoder gives
back from an [x86, LZMA2] raw stream."""
import lzma

import numpy as np
import pytest

from conftest import rand_bytes
from megalania_amd import binding, build, corpus

_LZMA2 = [dict(id=lzma.FILTER_LZMA2, preset=0)]


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build_host()


def liblzma_x86(d: bytes) -> bytes:
    raw = lzma.compress(d, format=lzma.FORMAT_RAW, filters=[dict(id=lzma.FILTER_X86)] + _LZMA2)
    return lzma.decompress(raw, format=lzma.FORMAT_RAW, filters=_LZMA2)


def elf_slice(at: int, n: int = 16384) -> bytes:
    return corpus.elf1m()[0][at:at + n]


def _inputs():
    dense = np.array([0xE8, 0xE9, 0x00, 0xFF, 0x12], dtype=np.uint8)[np.frombuffer(rand_bytes(4096, 0xBC), dtype=np.uint8) % 5]
    return {
        "n0": b"", "n4": b"\xE8\x00\x00\x00", "n5": b"\xE8\x00\x00\x00\x00", "n6": b"\xE9\xFF\xFF\xFF\xFF\xE8",
        "opcode in the last four bytes": b"A" * 10 + b"\xE8\x00\x00\x00\x00" + b"\xE8\x00\x00",
        "dense": dense.tobytes(),
        "prose": corpus.prose_like(4096, 0x51),
        "elf@0": elf_slice(0), "elf@256K": elf_slice(256 << 10), "elf@512K": elf_slice(512 << 10),
    }


def test_bcj_matches_liblzma():
    for name, d in _inputs().items():
        f = binding.bcj_x86(d)
        assert len(f) == len(d), name
        assert f == liblzma_x86(d), name
        assert binding.bcj_x86(f, encode=False) == d, name
    # the dense mix is really about the filter's masks: most of its opcodes sit inside another one's operand
    d = _inputs()["dense"]
    assert binding.bcj_x86(d) != d


def test_bcj_changes_code_not_prose():
    p = corpus.prose_like(65536, 0x51)
    assert binding.bcj_x86(p) == p
    e = elf_slice(512 << 10)
    changed = sum(a != b for a, b in zip(e, binding.bcj_x86(e)))
    assert changed > 0
    if corpus.elf1m()[1].startswith("first 1 MiB of"):
        assert changed == 2009
