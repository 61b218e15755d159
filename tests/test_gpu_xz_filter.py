"""The driver's --format xz, --filter and --dict-size on the device: what it writes decodes with liblzma and declares
what was asked for, --filter auto follows the exact costs of the two seeds, an [x86, LZMA2] seed stream selects the
filter, and a run without the new options writes what it wrote before."""
import lzma
import re
import subprocess

import numpy as np
import pytest

from megalania_amd import binding, build, corpus

pytestmark = pytest.mark.gpu

RUN = ["--epochs", "1", "--phases", "1", "--steps", "20", "--neighbours", "1024"]
EXTREME = 9 | lzma.PRESET_EXTREME


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build_all()


def elf_slice() -> bytes:
    return corpus.elf1m()[0][524288:524288 + 16384]


def prose() -> bytes:
    return corpus.prose_like(16384, 0x51)


def cli(tmp_path, data, args, ok=True):
    f = tmp_path / "in.bin"
    f.write_bytes(data)
    out = tmp_path / "out.bin"
    if out.exists():
        out.unlink()
    r = subprocess.run([build.CLI] + RUN + args + ["-o", str(out), str(f)], capture_output=True, timeout=120)
    err = r.stderr.decode(errors="replace")
    assert (r.returncode == 0) == ok, err[-600:]
    return (out.read_bytes() if ok else None), err


def best_cost(err: str) -> float:
    return float(re.findall(r"best: ([0-9.]+)", err)[-1])


def test_cli_xz_x86_roundtrip(tmp_path):
    e = elf_slice()
    for props in ([], ["--lc", "3", "--pb", "2"]):
        x, _ = cli(tmp_path, e, ["--format", "xz", "--filter", "x86"] + props)
        assert lzma.decompress(x) == e
        info = binding.stream_info_x(x)
        assert info["filter"] == 4 and info["declared_size"] == len(e) and info["dict_size"] == 1 << 22
        assert (info["lc"], info["lp"], info["pb"]) == ((3, 0, 2) if props else (0, 0, 0))
    cli(tmp_path, e, ["--filter", "x86"], ok=False)  # an .lzma stream cannot declare it


_SEED_COSTS = {}


def seed_cost(d: bytes) -> int:
    """exact cost of the optimal seed at its defaults on a handle over d"""
    if d not in _SEED_COSTS:
        sa = binding.SA(d, neighbours_per_step=1024)
        sa.seed_optimal()
        _SEED_COSTS[d] = sa.current()[1]
        sa.close()
    return _SEED_COSTS[d]


@pytest.mark.parametrize("name", ["elf", "prose", "synthetic"])
def test_cli_filter_auto_follows_exact_costs(name, tmp_path):
    d = {"elf": elf_slice, "prose": prose, "synthetic": lambda: corpus._synthetic_elf(16384, 0xEF)}[name]()
    x, err = cli(tmp_path, d, ["--format", "xz", "--filter", "auto"])
    m = re.search(r"filter auto: none (\d+) x86 (\d+) -> (none|x86) \(exact costs (\d+) (\d+)\)", err)
    assert m, err[-600:]
    plain, filtered = seed_cost(d), seed_cost(binding.bcj_x86(d))
    print(f"{name}: none {plain} x86 {filtered} cost units ({plain / 16384:.1f} / {filtered / 16384:.1f} B) -> {m.group(3)}")
    assert (int(m.group(4)), int(m.group(5))) == (plain, filtered)
    assert (int(m.group(1)), int(m.group(2))) == (-(-plain // 16384), -(-filtered // 16384))
    want = "x86" if filtered < plain else "none"
    assert m.group(3) == want
    assert binding.stream_info_x(x)["filter"] == (4 if want == "x86" else 0)
    assert lzma.decompress(x) == d
    if name == "prose":
        assert plain == filtered and want == "none"
    if name == "elf" and corpus.elf1m()[1].startswith("first 1 MiB of"):
        assert filtered < plain and want == "x86"


def test_cli_seed_stream_x86(tmp_path):
    e = elf_slice()
    xs = lzma.compress(e, format=lzma.FORMAT_XZ,
                       filters=[dict(id=lzma.FILTER_X86), dict(id=lzma.FILTER_LZMA2, preset=EXTREME, lc=0, lp=0, pb=0)])
    s = tmp_path / "seed.xz"
    s.write_bytes(xs)
    x, err = cli(tmp_path, e, ["--format", "xz", "--seed-stream", str(s)])
    seed = float(re.search(r"seed stream: \d+ packets, estimate ([0-9.]+) bytes", err).group(1))
    assert best_cost(err) <= seed
    assert binding.stream_info_x(x)["filter"] == 4 and lzma.decompress(x) == e
    _, err = cli(tmp_path, e, ["--format", "lzma", "--seed-stream", str(s)], ok=False)
    assert "x86" in err and "--format xz" in err
    _, err = cli(tmp_path, e, ["--format", "xz", "--filter", "none", "--seed-stream", str(s)], ok=False)
    assert "x86" in err


@pytest.mark.parametrize("fmt", ["lzma", "xz"])
def test_cli_dict_size_small_window(fmt, tmp_path):
    p = prose()
    x, _ = cli(tmp_path, p, ["--format", fmt, "--dict-size", "4096", "--greedy-seed", "16"])
    assert binding.stream_info_x(x)["dict_size"] == 4096
    # liblzma keeps a dictionary of the declared size only: one copy from farther back would not decode
    assert lzma.decompress(x) == p
    slab, st = binding.stream_import(x, p, window=4096, clip=True)
    assert st["clipped"] == 0 and st["matches"] > 0
    assert int(slab["dist"][slab["type"] == binding.MATCH].max()) < 4096


def test_cli_default_unchanged(tmp_path):
    p = prose()
    slab_path = tmp_path / "best.slab"
    x, _ = cli(tmp_path, p, ["--save-slab", str(slab_path)])
    raw = slab_path.read_bytes()
    assert raw[:8] == b"MGLSLAB1" and int.from_bytes(raw[8:16], "little") == len(p)
    slab = np.frombuffer(raw[24:], dtype=binding.PACKET)
    assert x == binding.emit_stream(p, slab)
    assert binding.stream_info(x) == dict(container=binding.CONTAINER_LZMA, lc=0, lp=0, pb=0, dict_size=1 << 22, declared_size=len(p))
