"""One parse costed under every supported lc/lp/pb at once (mgl_props_sweep, SA.props_sweep, CLI --props auto).
A packet slab is a valid parse whatever the properties are; the sweep walks it once per triple with the whole model
in LDS.  Every comparison is an exact integer: against the CPU oracle for all 75 triples, against the device's own
costing on handles made with the triple, and end to end through the CLI and liblzma.  `-m gpu`."""
import ctypes as C
import lzma
import re
import subprocess

import numpy as np
import pytest

from _libs import Oracle, literal_slab
from conftest import rand_bytes, sha_slab, slab_from_rle
from megalania_amd import binding, build, corpus
from megalania_amd.binding import PROPS_TRIPLES, best_props

pytestmark = pytest.mark.gpu

EXTREME = 9 | lzma.PRESET_EXTREME
MGL_EINVAL, MGL_ERANGE = -1, -4


def alone(data, lc=0, lp=0, pb=0):
    return lzma.compress(data, format=lzma.FORMAT_ALONE,
                         filters=[dict(id=lzma.FILTER_LZMA1, preset=EXTREME, dict_size=1 << 22, lc=lc, lp=lp, pb=pb)])


def xz_parse(data, lc=0, lp=0, pb=0):
    return binding.stream_import(alone(data, lc, lp, pb), data)[0]


def oracle_table(data, slab):
    return [Oracle(data, lc, lp, pb).cost_slab(slab)["total"] for lc, lp, pb in PROPS_TRIPLES]


def c5_256k():
    return corpus.config_input("c5")[0][: 1 << 18]


def check_against_oracle(data, slabs):
    sa = binding.SA(data, neighbours_per_step=64)
    try:
        for name, slab in slabs:
            got, ms = sa.props_sweep(slab)
            want = oracle_table(data, slab)
            assert got.dtype == np.uint64 and len(got) == 75
            bad = [(PROPS_TRIPLES[t], int(got[t]), want[t]) for t in range(75) if int(got[t]) != want[t]]
            print(f"{name}: n {len(data)}, sweep {ms:.3f} ms, cheapest {best_props(got)} {int(min(got))}, 0/0/0 {int(got[0])}, "
                  f"{len(bad)} mismatches")
            assert not bad, (name, bad[:5])
    finally:
        sa.close()


@pytest.mark.parametrize("cfg", ["c1", "c2", "c5"])
def test_sweep_equals_oracle_on_xz_parses(cfg):
    data = c5_256k() if cfg == "c5" else corpus.config_input(cfg)[0]
    slabs = [("xz 0/0/0", xz_parse(data)), ("xz 3/0/2", xz_parse(data, 3, 0, 2))]
    if cfg == "c2":
        slabs.append(("all-literal", literal_slab(len(data))))
    check_against_oracle(data, slabs)


def test_sweep_equals_oracle_on_golden_walks(golden, golden_input):
    """every walk of the stored vectors: all four LONG_REP indices, SHORT_REP, 15 direct bits, length 273"""
    by_input = {}
    for w in golden["walks"]:
        by_input.setdefault(w["input"], []).append(w)
    for name, walks in by_input.items():
        data = golden_input(name)
        check_against_oracle(data, [(w["name"], slab_from_rle(len(data), w["packets"])) for w in walks])


def test_sweep_equals_oracle_on_random_bytes():
    data = rand_bytes(1 << 16, 0x5EED)
    check_against_oracle(data, [("xz 0/0/0", xz_parse(data)), ("all-literal", literal_slab(len(data)))])


@pytest.mark.parametrize("props", [(0, 0, 0), (3, 0, 2), (0, 4, 0), (4, 0, 4), (0, 2, 2)])
def test_sweep_equals_device_costing(props):
    data = corpus.config_input("c2")[0]
    slab = xz_parse(data)
    lc, lp, pb = props
    sa = binding.SA(data, neighbours_per_step=64, lc=lc, lp=lp, pb=pb)
    try:
        got, _ = sa.props_sweep(slab)
        assert int(got[PROPS_TRIPLES.index(props)]) == sa.cost_slab(slab, want_cum=False)["total"]
    finally:
        sa.close()


def _raw_sweep(sa, slab, cap):
    out = (binding.PropsCost * max(cap, 1))()
    cnt = C.c_size_t(0)
    rc = sa.L.mgl_props_sweep(sa.h, None if slab is None else slab.ctypes.data_as(C.c_void_p), out, cap, C.byref(cnt), None)
    return rc, cnt.value, out


def test_contract():
    data = corpus.config_input("c2")[0]
    n = len(data)
    slab = xz_parse(data)
    a = binding.SA(data, neighbours_per_step=64)
    b = binding.SA(data, neighbours_per_step=64, lc=3, lp=0, pb=2)
    try:
        # 75 entries in canonical order whatever the handle's own triple is
        rc, cnt, out = _raw_sweep(a, np.ascontiguousarray(slab, dtype=binding.PACKET), 75)
        assert rc == 0 and cnt == 75
        assert [(e.props.lc, e.props.lp, e.props.pb) for e in out] == PROPS_TRIPLES
        ta, tb = a.props_sweep(slab)[0], b.props_sweep(slab)[0]
        assert [e.cost for e in out] == ta.tolist() == tb.tolist()
        # a buffer that is too small
        rc, cnt, _ = _raw_sweep(a, np.ascontiguousarray(slab, dtype=binding.PACKET), 10)
        assert rc == MGL_ERANGE and cnt == 75
        # what cost_slab refuses, the sweep refuses
        off_end = literal_slab(n)
        off_end[n - 1] = (binding.MATCH, 0, 5)
        type0 = slab.copy()
        type0[0]["type"] = 0
        for bad in (off_end, type0):
            with pytest.raises(binding.MglError) as e1:
                a.cost_slab(bad, want_cum=False)
            with pytest.raises(binding.MglError) as e2:
                a.props_sweep(bad)
            assert e1.value.rc == MGL_EINVAL and e2.value.rc == MGL_EINVAL
        # packets == NULL: the current slab
        a.run(2)
        cur, cur_cost = a.current()
        t_null, t_cur = a.props_sweep()[0], a.props_sweep(cur)[0]
        assert t_null.tolist() == t_cur.tolist() and int(t_null[0]) == cur_cost
    finally:
        a.close()
        b.close()


def test_sweep_leaves_the_search_untouched():
    data = corpus.config_input("c2")[0]
    one = binding.SA(data, neighbours_per_step=4096)
    two = binding.SA(data, neighbours_per_step=4096)
    try:
        s1 = one.run(8)
        m1 = one.step_modes()
        two.run(4)
        m2a = two.step_modes()
        two.props_sweep()
        two.props_sweep(xz_parse(data))
        s2 = two.run(4)
        m2 = np.concatenate([m2a, two.step_modes()])
        (c1, cc1), (c2, cc2) = one.current(), two.current()
        assert sha_slab(c1) == sha_slab(c2) and cc1 == cc2
        assert one.best()[1] == two.best()[1] and s1["best_cost"] == s2["best_cost"] and s1["current_cost"] == s2["current_cost"]
        assert m1.tolist() == m2.tolist()
    finally:
        one.close()
        two.close()


@pytest.mark.parametrize("cfg", ["c1", "c2"])
def test_ties_go_to_the_first_triple(cfg):
    """on 7-bit text lc = 1 adds nothing: 0/0/0 and 1/0/0 cost the same, and the first in canonical order wins"""
    data = corpus.config_input(cfg)[0]
    sa = binding.SA(data, neighbours_per_step=64)
    try:
        got, _ = sa.props_sweep(xz_parse(data))
    finally:
        sa.close()
    assert int(got[PROPS_TRIPLES.index((0, 0, 0))]) == int(got[PROPS_TRIPLES.index((1, 0, 0))])
    assert best_props(got) == (0, 0, 0)


def _cli(tmp_path, data, args, name):
    f = tmp_path / "in.bin"
    f.write_bytes(data)
    r = subprocess.run([build.CLI] + args + ["--epochs", "1", "--phases", "1", "--steps", "20", str(f)], capture_output=True, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-600:]
    assert lzma.decompress(r.stdout, format=lzma.FORMAT_ALONE) == data
    print(f"{name}: {len(r.stdout)} B; " + " | ".join(ln for ln in r.stderr.decode().splitlines() if ln.startswith("props:")))
    return r.stdout, r.stderr.decode()


def test_cli_props_auto_from_a_stream(tmp_path):
    data = c5_256k()
    stream = alone(data, 3, 0, 2)
    seed = tmp_path / "seed.lzma"
    seed.write_bytes(stream)
    table = oracle_table(data, binding.stream_import(stream, data)[0])
    lc, lp, pb = best_props(table)
    print(f"oracle: cheapest {lc}/{lp}/{pb} {min(table)} ({-(-min(table) // 16384)} B), "
          f"3/0/2 {table[PROPS_TRIPLES.index((3, 0, 2))]} ({-(-table[PROPS_TRIPLES.index((3, 0, 2))] // 16384)} B)")
    auto, err = _cli(tmp_path, data, ["--seed-stream", str(seed), "--props", "auto", "--props-table"], "auto")
    fixed, _ = _cli(tmp_path, data, ["--seed-stream", str(seed), "--lc", "3", "--lp", "0", "--pb", "2"], "3/0/2")
    assert auto[0] == (pb * 5 + lp) * 9 + lc
    assert len(auto) <= len(fixed)
    assert f"props: lc={lc} lp={lp} pb={pb}, sweep {-(-min(table) // 16384)} B" in err
    rows = re.findall(r"props-table: lc=(\d) lp=(\d) pb=(\d) cost (\d+)", err)
    assert [(int(a), int(b), int(c)) for a, b, c, _ in rows] == PROPS_TRIPLES and [int(r[3]) for r in rows] == table


def test_cli_props_auto_reseeds_the_optimal_parse(tmp_path):
    data = c5_256k()
    auto, err = _cli(tmp_path, data, ["--optimal-seed", "1", "--props", "auto"], "auto")
    fixed, _ = _cli(tmp_path, data, ["--optimal-seed", "1", "--lc", "0", "--lp", "0", "--pb", "0"], "0/0/0")
    m = re.search(r"props: lc=(\d) lp=(\d) pb=(\d), sweep (\d+) B, at 0/0/0 (\d+) B, (\d+) rounds", err)
    assert m, err[-600:]
    lc, lp, pb, sweep, at0, rounds = (int(x) for x in m.groups())
    assert (lc, lp, pb) in PROPS_TRIPLES and sweep < at0 and 1 <= rounds <= 3
    assert auto[0] == (pb * 5 + lp) * 9 + lc
    assert len(auto) < len(fixed)


def test_cli_props_auto_refuses_explicit_properties(tmp_path):
    f = tmp_path / "in.bin"
    f.write_bytes(corpus.lorem(2048))
    for extra in (["--lc", "1"], ["--chains", "2", "--rank", "0", "--comm-file", str(tmp_path / "comm")]):
        r = subprocess.run([build.CLI, "--props", "auto"] + extra + [str(f)], capture_output=True, timeout=60)
        assert r.returncode != 0 and b"usage" in r.stderr and r.stdout == b""
