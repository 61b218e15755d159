"""CLI --props-joint without a GPU: the usage text names the option, and every combination the option refuses ends with
a usage error before the input is opened or a device is looked for."""
import subprocess

import pytest

from megalania_amd import build

JOINT = ["--props", "auto", "--adaptive-seed", "2", "--parse-sweep", "--props-joint", "3"]


def _run(args):
    return subprocess.run([build.CLI] + args, capture_output=True, timeout=60)


def test_usage_names_the_option():
    r = _run([])
    assert r.returncode != 0 and r.stdout == b""
    assert b"usage:" in r.stderr and b"--props-joint" in r.stderr


@pytest.mark.parametrize("args", [
    ["--props", "auto", "--adaptive-seed", "2", "--props-joint", "3"],
    ["--adaptive-seed", "2", "--parse-sweep", "--props-joint", "3"],
    JOINT + ["--seed-stream", "some.lzma"],
    JOINT + ["--load-slab", "some.slab"],
    JOINT + ["--greedy-seed", "8"],
    JOINT + ["--lc", "3"],
    JOINT + ["--chains", "2", "--rank", "0", "--comm-file", "some.comm"],
    JOINT[:-1] + ["0"],
    JOINT[:-1] + ["5"],
], ids=["no-parse-sweep", "no-props-auto", "seed-stream", "load-slab", "greedy-seed", "lc", "chains", "T0", "T5"])
def test_refused_combinations(args, tmp_path):
    f = tmp_path / "in.bin"
    f.write_bytes(b"some input that is never opened")
    r = _run(args + [str(f)])
    assert r.returncode != 0 and r.stdout == b""
    assert b"usage:" in r.stderr and b"no HIP device" not in r.stderr
