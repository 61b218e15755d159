"""The CLI's --parse-sweep argument checks: they come before the input is opened and before any device call, so they
are the same with and without a GPU."""
import subprocess

import pytest

from megalania_amd import build


@pytest.mark.parametrize("args", [["--parse-sweep"], ["--parse-sweep", "--optimal-seed", "3"],
                                  ["--parse-sweep", "--adaptive-seed", "3", "--match-finder", "frontier"],
                                  ["--parse-sweep", "--adaptive-seed", "3", "--match-finder", "nearest"]],
                         ids=["alone", "optimal", "frontier", "nearest"])
def test_parse_sweep_refusals(tmp_path, args):
    f = tmp_path / "in.txt"
    f.write_bytes(b"hello hello hello")
    r = subprocess.run([build.CLI] + args + [str(f)], capture_output=True, timeout=60)
    assert r.returncode != 0 and r.stdout == b""
    assert b"usage:" in r.stderr and b"no HIP device" not in r.stderr
