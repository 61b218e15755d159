"""Seeding the search from the parse of an existing .lzma / .xz stream (mgl_stream_import + SA.seed_stream, CLI
--seed-stream): the device costs the imported slab exactly as the host coder does, the search continues from it and
never ends above it, and what comes out still decodes and is never longer than the stream it started from.
Streams are made at test time by liblzma (the standard library's `lzma` module).  `-m gpu`."""
import ctypes as C
import lzma
import subprocess

import numpy as np
import pytest

from conftest import rand_bytes
from megalania_amd import binding, build, corpus

pytestmark = pytest.mark.gpu

EXTREME = 9 | lzma.PRESET_EXTREME
CONFIGS = {"c2": dict(), "c5": dict(pb=2, max_bucket_scan=4096)}  # bench.py's per-config settings


def alone(data, preset, lc=0, lp=0, pb=0, dict_size=1 << 22):
    return lzma.compress(data, format=lzma.FORMAT_ALONE,
                         filters=[dict(id=lzma.FILTER_LZMA1, preset=preset, dict_size=dict_size, lc=lc, lp=lp, pb=pb)])


class _Packet(C.Structure):
    _fields_ = [("type", C.c_uint8), ("dist", C.c_uint32), ("len", C.c_uint16)]


class _Encoder(C.Structure):
    _fields_ = [("encode_bit", C.c_void_p), ("encode_direct_bits", C.c_void_p), ("private_data", C.c_void_p)]


def host_cost(data: bytes, slab, lc=0, lp=0, pb=0) -> int:
    """The slab's cost by the host coder: mgl_lzma_encode_packet over mgl_perplexity_encoder, packet by packet."""
    L = binding.host_lib()
    L.mgl_lzma_state_init.restype = C.c_bool
    L.mgl_lzma_state_init.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, binding.Properties]
    L.mgl_lzma_encode_packet.argtypes = [C.c_void_p, C.POINTER(_Encoder), _Packet]
    L.mgl_perplexity_encoder_new.argtypes = [C.POINTER(_Encoder), C.POINTER(C.c_uint64)]
    L.mgl_lzma_state_free.argtypes = [C.c_void_p]
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    state = C.create_string_buffer(512)  # mgl_lzma_state is well under this
    assert L.mgl_lzma_state_init(state, buf.ctypes.data, len(buf), binding.Properties(lc, lp, pb))
    total, enc = C.c_uint64(0), _Encoder()
    L.mgl_perplexity_encoder_new(C.byref(enc), C.byref(total))
    t, d, ln = slab["type"].tolist(), slab["dist"].tolist(), slab["len"].tolist()
    pos = 0
    while pos < len(ln):
        L.mgl_lzma_encode_packet(state, C.byref(enc), _Packet(t[pos], d[pos], ln[pos]))
        pos += ln[pos]
    L.mgl_lzma_state_free(state)
    return total.value


def seeded_run(data, stream, props, steps=200, **kw):
    lc = {k: props.get(k, 0) for k in ("lc", "lp", "pb")}
    slab, st = binding.stream_import(stream, data)
    want = host_cost(data, slab, **lc)
    sa = binding.SA(data, neighbours_per_step=4096, **props, **kw)
    assert sa.cost_slab(slab, want_cum=False)["total"] == want
    seed = sa.seed_stream(stream)
    assert seed == want
    sa.begin_epoch(0, from_best=True)
    run = sa.run(steps)
    best, best_cost = sa.best()
    assert best_cost <= seed
    out = binding.emit_stream(data, best, **lc)
    assert lzma.decompress(out, format=lzma.FORMAT_ALONE) == data
    assert len(out) <= len(stream)
    print(f"seed {18 + seed / 16384:.1f} B (stream {len(stream)} B) -> best {18 + best_cost / 16384:.1f} B after {steps} steps, "
          f"emitted {len(out)} B; best < seed: {best_cost < seed}; improving_neighbours {run['improving_neighbours']}, "
          f"dropped_neighbours {run['dropped_neighbours']}, imported {st}")
    sa.close()
    return seed, best_cost, run


@pytest.mark.parametrize("cfg", ["c2", "c5"])
def test_seed_from_liblzma_stream(cfg):
    data = corpus.config_input(cfg)[0]
    props = CONFIGS[cfg]
    stream = alone(data, EXTREME, props.get("lc", 0), props.get("lp", 0), props.get("pb", 0))
    seeded_run(data, stream, props)


def test_stream_props_differ_from_the_handle():
    """A parse is valid under any lc/lp/pb: a 3/0/2 stream seeds a 0/0/0 handle, costed at 0/0/0."""
    data = corpus.config_input("c2")[0]
    stream = alone(data, EXTREME, 3, 0, 2)
    slab, _ = binding.stream_import(stream, data)
    sa = binding.SA(data, neighbours_per_step=4096)
    assert sa.seed_stream(stream) == host_cost(data, slab) != host_cost(data, slab, 3, 0, 2)
    sa.close()


def test_clipped_seed():
    key = rand_bytes(64 << 10, 0x6B)
    data = key + corpus.enwik_like(5 << 20, 0x5A) + key
    stream = alone(data, 1, dict_size=8 << 20)
    sa = binding.SA(data, neighbours_per_step=4096)
    with pytest.raises(binding.MglError):
        sa.seed_stream(stream)
    seed = sa.seed_stream(stream, clip=True)
    sa.begin_epoch(0, from_best=True)
    sa.run(20)
    best, best_cost = sa.best()
    assert best_cost <= seed
    assert lzma.decompress(binding.emit_stream(data, best), format=lzma.FORMAT_ALONE) == data
    sa.close()


def test_seed_from_xz_stream():
    data = corpus.config_input("c2")[0]
    stream = lzma.compress(data, format=lzma.FORMAT_XZ, preset=EXTREME)
    info = binding.stream_info(stream)
    seeded_run(data, stream, {k: info[k] for k in ("lc", "lp", "pb")})


def test_cli_seed_stream(tmp_path):
    data = corpus.config_input("c2")[0]
    f = tmp_path / "c2.bin"
    f.write_bytes(data)
    s = tmp_path / "c2.lzma"
    s.write_bytes(alone(data, EXTREME, 3, 0, 2))
    out = tmp_path / "out.lzma"
    common = ["--epochs", "1", "--phases", "1", "--steps", "100"]
    r = subprocess.run([build.CLI, "--seed-stream", str(s)] + common + ["-o", str(out), str(f)], capture_output=True, timeout=600)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-600:]
    assert "seed stream:" in err and "0 re-expressed, 0 clipped" in err, err[-600:]
    o = out.read_bytes()
    assert o[0] == (2 * 5 + 0) * 9 + 3  # no --lc/--lp/--pb: the stream's properties
    assert lzma.decompress(o, format=lzma.FORMAT_ALONE) == data
    assert len(o) <= s.stat().st_size
    # given properties win, with a note
    r = subprocess.run([build.CLI, "--seed-stream", str(s), "--pb", "0"] + common + ["-o", str(out), str(f)],
                       capture_output=True, timeout=600)
    assert r.returncode == 0 and b"note:" in r.stderr, r.stderr.decode()[-600:]
    o = out.read_bytes()
    assert o[0] == 0 and lzma.decompress(o, format=lzma.FORMAT_ALONE) == data
    # usage errors and a stream of another input: non-zero, nothing written
    slab_file = tmp_path / "x.slab"
    slab_file.write_bytes(b"MGLSLAB1")
    g = tmp_path / "other.bin"
    g.write_bytes(corpus.enwik_like(len(data), 0x99))
    for extra, target in ((["--load-slab", str(slab_file)], f), (["--greedy-seed", "256"], f), ([], g)):
        o2 = tmp_path / "none.lzma"
        r = subprocess.run([build.CLI, "--seed-stream", str(s)] + extra + common + ["-o", str(o2), str(target)],
                           capture_output=True, timeout=600)
        assert r.returncode != 0 and r.stdout == b"" and not o2.exists(), (extra, r.stderr.decode()[-400:])
