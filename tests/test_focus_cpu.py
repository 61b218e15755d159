"""The focus window (mgl_sa_set_focus, mgl_sa_focus, mgl_focus_slice, include/megalania_hip.h) without a GPU: the slice rule
against its restatement, the interface, and the CLI's refusals.  tests/test_gpu_focus.py holds the device to the target rule."""
import ctypes as C
import os
import subprocess

import pytest

from megalania_amd import binding, build, corpus, multi_gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MGL_EINVAL = -1


def sizes(world):
    return (2 * world, 2 * world + 1, 4097, 10 ** 8)


def slice_rule(n, world, rank, rnd):
    """Even rounds cut at i n / world; odd rounds keep 0 and n and cut at (2 i - 1) n / (2 world) between."""
    B = [i * n // world for i in range(world + 1)] if rnd % 2 == 0 else \
        [0] + [(2 * i - 1) * n // (2 * world) for i in range(1, world)] + [n]
    return B[rank], B[rank + 1]


@pytest.mark.parametrize("world", range(1, 10))
def test_slices_equal_the_rule_and_tile_the_file(world):
    for n in sizes(world):
        per_round = []
        for rnd in range(4):
            got = [binding.focus_slice(n, world, r, rnd) for r in range(world)]
            assert got == [slice_rule(n, world, r, rnd) for r in range(world)], (n, world, rnd)
            assert got[0][0] == 0 and got[-1][1] == n
            assert all(lo < hi for lo, hi in got), (n, world, rnd, got)  # none is empty
            assert all(got[r][1] == got[r + 1][0] for r in range(world - 1))  # no gap, no overlap
            per_round.append(got)
        assert per_round[0] == per_round[2] and per_round[1] == per_round[3]
        if world >= 2 and n >= 4 * world:
            # every inner bound of an odd round lies strictly between two bounds of the even rounds: no boundary stays fixed
            even = [s[0] for s in per_round[0]] + [n]
            for i in range(1, world):
                b = per_round[1][i][0]
                assert even[i - 1] < b < even[i], (n, world, i, b, even)


def test_slice_refusals():
    L = binding.hip_lib()
    lo, hi = C.c_uint64(7), C.c_uint64(7)
    for n, world, rank in ((100, 0, 0), (100, 4, 4), (100, 4, 5), (7, 4, 0), (1, 1, 0), (0, 1, 0)):
        assert L.mgl_focus_slice(n, world, rank, 0, C.byref(lo), C.byref(hi)) == MGL_EINVAL, (n, world, rank)
        assert L.mgl_focus_slice(n, world, rank, 1, C.byref(lo), C.byref(hi)) == MGL_EINVAL, (n, world, rank)
        with pytest.raises(binding.MglError) as e:
            binding.focus_slice(n, world, rank, 0)
        assert e.value.rc == MGL_EINVAL
    assert (lo.value, hi.value) == (7, 7)  # a refusal writes nothing
    assert L.mgl_focus_slice(100, 4, 0, 0, None, C.byref(hi)) == MGL_EINVAL
    assert L.mgl_focus_slice(100, 4, 0, 0, C.byref(lo), None) == MGL_EINVAL
    assert L.mgl_focus_slice(8, 4, 3, 1, C.byref(lo), C.byref(hi)) == 0 and (lo.value, hi.value) == (5, 8)
    # a null handle is refused by the two calls that take one
    assert L.mgl_sa_set_focus(None, 0, 0) == MGL_EINVAL and L.mgl_sa_focus(None, C.byref(lo), C.byref(hi), None) == MGL_EINVAL


def test_the_interface_names_the_new_calls():
    header = open(os.path.join(ROOT, "include", "megalania_hip.h")).read()
    for decl in ("int mgl_sa_set_focus(mgl_sa* sa, uint64_t lo, uint64_t hi);",
                 "int mgl_sa_focus(mgl_sa* sa, uint64_t* lo, uint64_t* hi, uint64_t* packets);",
                 "int mgl_focus_slice(uint64_t n, uint32_t world, uint32_t rank, uint64_t round, uint64_t* lo, uint64_t* hi);"):
        assert decl in header, decl
    for sym in ("mgl_sa_set_focus", "mgl_sa_focus", "mgl_focus_slice"):
        assert sym in binding.HIP_SYMBOLS and hasattr(binding.hip_lib(), sym)  # the library exports them without a GPU
    assert callable(binding.SA.set_focus) and callable(binding.SA.focus) and callable(binding.focus_slice)
    assert callable(multi_gpu.focus_chain)
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "--focus" in open(os.path.join(ROOT, doc)).read(), doc


def test_usage_names_the_option_and_keeps_the_pinned_strings():
    r = subprocess.run([build.CLI], capture_output=True, timeout=60)
    assert r.returncode != 0 and r.stdout == b""
    for s in (b"--focus LO:HI", b"--focus rank", b"--exchange best|cross|cross-all", b"--filter none|x86|auto", b"--format lzma|xz",
              b"--dict-size BYTES"):
        assert s in r.stderr, s


CHAINS = ["--chains", "2", "--rank", "0", "--comm-file", "some.comm", "--transport", "shm"]


@pytest.mark.parametrize("args", [
    ["--focus"],
    ["--focus", ""],
    ["--focus", "12"],
    ["--focus", "12:"],
    ["--focus", ":12"],
    ["--focus", "a:b"],
    ["--focus", "4:12x"],
    ["--focus", "-4:12"],
    ["--focus", "12:12"],
    ["--focus", "12:4"],
    ["--focus", "0:0"],
    ["--focus", "ranks"],
    ["--focus", "rank"],
    ["--focus", "rank", "--chains", "1", "--rank", "0", "--comm-file", "some.comm", "--transport", "shm"],
    ["--focus", "4:12", "--focus", "4:12"],
    ["--focus", "rank", "--focus", "rank"] + CHAINS,
    ["--focus", "4:12", "--focus", "rank"] + CHAINS,
    CHAINS + ["--focus", "rank", "--focus", "4:12"],
], ids=["no-value", "empty", "no-colon", "no-hi", "no-lo", "letters", "trailing", "negative", "lo-equals-hi", "lo-above-hi", "zero-zero",
        "unknown-word", "rank-without-chains", "rank-with-one-chain", "range-twice", "rank-twice", "range-then-rank", "rank-then-range"])
def test_cli_refuses_before_it_touches_a_device(args, tmp_path):
    f = tmp_path / "in.bin"
    f.write_bytes(corpus.prose_like(64, 1))
    r = subprocess.run([build.CLI] + args + [str(f)], capture_output=True, timeout=60, cwd=str(tmp_path))
    assert r.returncode != 0 and r.stdout == b""
    assert b"usage:" in r.stderr and b"no HIP device" not in r.stderr
    assert not os.path.exists(tmp_path / "some.comm")
    # ... before the input is opened, too: the same line with a file that does not exist is the same refusal
    r2 = subprocess.run([build.CLI] + args + [str(tmp_path / "absent.bin")], capture_output=True, timeout=60, cwd=str(tmp_path))
    assert r2.returncode != 0 and b"usage:" in r2.stderr and b"could not open" not in r2.stderr
