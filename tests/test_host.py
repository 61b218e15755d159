"""CPU-side product checks (no GPU): the C host emission path against the reference's
fixtures, and the C-ABI library's load/export contract.  No compute entry point of
libmegalania_hip.so is called here."""
import ctypes as C
import json
import lzma
import os
import re
import subprocess

import numpy as np
import pytest

from _libs import Oracle, literal_slab
from conftest import ROOT, sha, slab_from_rle
from megalania_amd import binding, build


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build_hip()
    build.build_host()


def test_c_abi_exports_every_declared_symbol():
    """Every function include/megalania_hip.h declares is exported by the library, and the
    library loads without a GPU."""
    hdr = open(os.path.join(ROOT, "include", "megalania_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mgl_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(binding.HIP_SYMBOLS), declared ^ set(binding.HIP_SYMBOLS)
    lib = C.CDLL(binding.HIP_SO)
    for name in sorted(declared):
        assert hasattr(lib, name), name
    lib.mgl_version.restype = C.c_char_p
    assert b"gfx950" in lib.mgl_version()
    # the code object inside is for gfx950 only
    out = subprocess.run(["strings", "-a", binding.HIP_SO], capture_output=True, text=True).stdout
    assert "gfx950" in out and "gfx90a" not in out and "sm_" not in out


def test_host_library_exports():
    hdr = open(os.path.join(ROOT, "megalania_amd", "host", "mgl_host.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mgl_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(binding.HOST_SYMBOLS), declared ^ set(binding.HOST_SYMBOLS)
    lib = C.CDLL(binding.HOST_SO)
    for name in sorted(declared):
        assert hasattr(lib, name), name


def test_rng_matches_oracle():
    lib = binding.hip_lib()
    o = Oracle.lib()
    for seed, step, j, n in [(0, 0, 0, 0), (1673551, 5, 17, 3), (2**63 + 9, 10**9, 0xFFFFFFFF, 40), (7, 99, 4095, 31)]:
        assert lib.mgl_rng_draw_at(seed, step, j, n) == o.orc_draw(seed, step, j, n) < 2**31


def test_bit_cost_table_is_the_reference_table():
    """csrc/mgl_cost_table.inc (exact integer arithmetic) == the oracle's libm table == the
    reference's perplexity_table.h (its hash, recorded in tests/golden/oracle_vs_ref.json)."""
    txt = open(os.path.join(ROOT, "megalania_amd", "csrc", "mgl_cost_table.inc")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    mine = np.array([int(x) for x in re.findall(r"\d+", txt)], dtype=np.uint16)
    assert len(mine) == 2048 and (mine == Oracle.cost_table()).all()
    with open(os.path.join(ROOT, "tests", "golden", "oracle_vs_ref.json")) as f:
        assert sha(mine) == json.load(f)["perplexity_table_sha256"]


def test_host_emission_matches_reference_streams(golden, golden_input):
    """mgl_emit_stream (C, over EncoderInterface/OutputInterface) reproduces the byte streams
    the reference's range_encoder.c + lzma_header_encoder.c produced for the same slabs."""
    for w in golden["walks"]:
        data = golden_input(w["input"])
        slab = slab_from_rle(len(data), w["packets"]).astype(binding.PACKET)
        stream = binding.emit_stream(data, slab)
        assert len(stream) == w["stream_len"], w["name"]
        assert sha(np.frombuffer(stream, dtype=np.uint8)) == w["stream_sha256"], w["name"]
        if "stream_hex" in w:
            assert stream.hex() == w["stream_hex"]


@pytest.mark.parametrize("lc,lp,pb", [(0, 0, 2), (3, 0, 2), (0, 2, 0), (1, 1, 1), (4, 0, 4)])
def test_host_emission_lc_lp_pb_roundtrip(lc, lp, pb):
    """lc/lp/pb != 0 has no reference implementation (lzma_packet_encoder.c:17,44,113): cost
    parity is unpinned there; the stream itself is pinned by liblzma decoding it, and the
    oracle's estimate must agree with the real stream length to within a few bytes."""
    from megalania_amd import corpus
    data = corpus.enwik_like(6000, 0x42)
    o = Oracle(data, lc, lp, pb)
    slab = literal_slab(len(data))
    # a non-trivial valid parse: let the oracle's batched SA run a little
    best = slab.copy()
    o.sa_batched(slab, best, 0, 0, seed=3, K=6, phase=0, iters_per_epoch=len(data), step_begin=0, step_end=40)
    stream = binding.emit_stream(data, slab.astype(binding.PACKET), lc, lp, pb)
    assert stream[0] == (pb * 5 + lp) * 9 + lc
    assert lzma.decompress(stream, format=lzma.FORMAT_ALONE) == data
    assert stream == o.emit(slab)
    est = 18 + o.cost_slab(slab)["total"] / 16384
    assert abs(est - len(stream)) <= 4, (est, len(stream))


def test_host_emission_rejects_broken_slab():
    data = b"hello hello"
    slab = binding.literal_slab(len(data))
    slab[6] = (binding.MATCH, 5, 9)  # runs past the end
    with pytest.raises(binding.MglError):
        binding.emit_stream(data, slab)


def test_cli_without_gpu_fails_loudly(tmp_path):
    """No CPU fallback: on a box without a GPU the driver must refuse, not silently search
    on the CPU."""
    if binding.hip_lib().mgl_device_count() > 0:
        pytest.skip("a GPU is visible")
    f = tmp_path / "in.txt"
    f.write_bytes(b"hello hello hello")
    r = subprocess.run([build.CLI, str(f)], capture_output=True)
    assert r.returncode != 0 and b"no HIP device" in r.stderr and r.stdout == b""
    with pytest.raises(binding.MglError):
        binding.SA(b"hello hello")


def test_probability_update_form_is_exact(tmp_path):
    """mgl_prob_update is written branch-free ((c - v) >> 5 with an arithmetic shift); it must be the
    reference's update (probability_model.c:5-15) for every probability and both bits, as compiled by
    the host compiler (the device compiler sees the same header; the GPU parity tests cover it there)."""
    src = tmp_path / "pu.c"
    src.write_text('#include <stdint.h>\n#include "mgl_model.h"\n'
                   "int main(void) { for (uint32_t v = 0; v <= 2048; v++) for (uint32_t b = 0; b < 2; b++) {\n"
                   "  uint32_t ref = b ? v - (v >> 5) : v + ((2048u - v) >> 5);\n"
                   "  if (mgl_prob_update(v, b) != ref) return 1; }\n  return 0; }\n")
    exe = tmp_path / "pu"
    inc = os.path.join(ROOT, "megalania_amd", "csrc")
    subprocess.run([os.environ.get("CC", "gcc"), "-O2", "-I", inc, str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0
