"""Where a parse spends its bits, on the device (mgl_cost_map, SA.cost_map, CLI --cost-map / --cost-report /
--cost-bucket): the device returns the integers of the host form (binding.host_cost_map, which tests/test_cost_map_cpu.py
pins to the oracle) -- map and report, under the handle's triple and under a foreign one -- and leaves the search alone.
Shapes: the smallest at which k_costmap_walk / k_costmap_spread can go wrong (mgl_sa_create accepts n = 1, so that is the
smallest), the 64-position window's edges, a packet that ends at n.  `-m gpu`."""
import ctypes as C
import lzma
import re
import subprocess

import numpy as np
import pytest

import _random_parse as rp
import _validity
from _libs import LONG_REP, MATCH, PACKET, SHORT_REP, literal_slab
from conftest import sha_slab, slab_from_rle
from megalania_amd import binding, build, corpus

pytestmark = pytest.mark.gpu

MGL_EINVAL, MGL_ENOMEM = -1, -2
EXTREME = 9 | lzma.PRESET_EXTREME
FOREIGN = [(3, 0, 2), (0, 2, 2)]


def xz_parse(data, lc=0, lp=0, pb=0):
    stream = lzma.compress(data, format=lzma.FORMAT_ALONE,
                           filters=[dict(id=lzma.FILTER_LZMA1, preset=EXTREME, dict_size=1 << 22, lc=lc, lp=lp, pb=pb)])
    return binding.stream_import(stream, data)[0]


def assert_device_equals_host(sa, data, slab, props=None, what=""):
    """props None: the handle's own triple"""
    got_map, got = sa.cost_map(slab, props)
    own = (sa.props.lc, sa.props.lp, sa.props.pb)
    want_map, want = binding.host_cost_map(data, slab, own if props is None else props)
    ms = got.pop("gpu_ms")
    assert ms > 0 and got_map.dtype == np.uint32 and len(got_map) == len(data)
    assert got == want, (what, props, got, want)
    bad = np.nonzero(got_map != want_map)[0]
    assert len(bad) == 0, (what, props, bad[:5], got_map[bad[:5]], want_map[bad[:5]])
    assert int(got_map.astype(np.int64).sum()) == got["total"]
    if props is None:
        assert got["total"] == sa.cost_slab(slab, want_cum=False)["total"], what
    return got_map, got, ms


C2 = corpus.config_input("c2")[0]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_device_equals_host_at_small_sizes(n):
    data = C2[:n]
    slabs = [("all-literal", literal_slab(n)), ("random, stale entries", rp.random_parse(data, 41, rp.TEXT, "any")), ("xz", xz_parse(data))]
    sa = binding.SA(data, neighbours_per_step=64)
    try:
        for name, slab in slabs:
            for props in [None] + FOREIGN:
                assert_device_equals_host(sa, data, slab, props, f"n {n} {name}")
    finally:
        sa.close()


# ---- planted edges: n = 466 (seven windows of 64 and a ragged eighth)
#   [51, 128)   MATCH that starts inside window 0, straddles the edge at 64 and ends at the edge at 128
#   128         a literal directly behind the copy, the first position of its window: its match byte (data[127]) and, with
#               lc > 0, its previous byte are in the window before; the byte differs from the match byte
#   [130, 192)  LONG_REP 0 that ends at an edge; 192 SHORT_REP, the first position of its window
#   [193, 466)  MATCH of 273 bytes over four edges that ends exactly at n
EDGE_N = 466


def edge_case():
    data = corpus.lorem(50) + b"a" * 78 + b"b" + b"a" * (EDGE_N - 129)
    slab = literal_slab(EDGE_N)
    slab[51] = (MATCH, 0, 77)
    slab[130] = (LONG_REP, 0, 62)
    slab[192] = (SHORT_REP, 0, 1)
    slab[193] = (MATCH, 0, 273)
    assert len(data) == EDGE_N and 193 + 273 == EDGE_N and data[128] != data[127] and 51 + 77 == 128
    return data, _validity.poisoned(slab)


@pytest.mark.parametrize("created_at", [(0, 0, 0), (2, 1, 2)])
def test_window_edges_and_a_longest_packet_that_ends_at_n(created_at):
    data, slab = edge_case()
    lc, lp, pb = created_at
    sa = binding.SA(data, neighbours_per_step=64, lc=lc, lp=lp, pb=pb)
    try:
        for props in [None] + FOREIGN:
            got_map, rep, _ = assert_device_equals_host(sa, data, slab, props, "edges")
            assert rep["type_packets"] == [53, 2, 1, 1] and rep["type_bytes"] == [53, 350, 1, 62]
            assert (got_map[193:] > 0).any() and len(got_map) == EDGE_N
    finally:
        sa.close()


def test_foreign_triples_equal_handles_created_at_them():
    data = C2[:8192]
    slab = xz_parse(data)
    plain = binding.SA(data, neighbours_per_step=64)
    try:
        assert_device_equals_host(plain, data, slab, None, "own 0/0/0")
        for props in FOREIGN:
            lc, lp, pb = props
            native = binding.SA(data, neighbours_per_step=64, lc=lc, lp=lp, pb=pb)
            try:
                m1, r1, _ = assert_device_equals_host(plain, data, slab, props, "foreign")
                m2, r2, _ = assert_device_equals_host(native, data, slab, None, "native")
                assert (m1 == m2).all() and r1 == r2
                assert r2["total"] == native.cost_slab(slab, want_cum=False)["total"]
                # and back: the handle at the triple asked for 0/0/0
                m3, r3, _ = assert_device_equals_host(native, data, slab, (0, 0, 0), "back")
                assert r3["total"] == plain.cost_slab(slab, want_cum=False)["total"]
            finally:
                native.close()
    finally:
        plain.close()


GOLDEN_INPUTS = ["hello", "abab", "aaab", "lorem512", "lorem4k", "enwik3k", "rand2k", "reps", "zeros600", "far"]


@pytest.mark.parametrize("name", GOLDEN_INPUTS)
def test_golden_walks(golden, golden_input, name):
    """every walk of the stored vectors: all four LONG_REP indices, SHORT_REP, 15 direct bits (far), length 273"""
    assert {w["input"] for w in golden["walks"]} == set(GOLDEN_INPUTS)
    walks = [w for w in golden["walks"] if w["input"] == name]
    data = golden_input(name)
    sa = binding.SA(data, neighbours_per_step=64)
    try:
        for w in walks:
            _, rep, ms = assert_device_equals_host(sa, data, slab_from_rle(len(data), w["packets"]), None, w["name"])
            assert rep["total"] == w["total"] and rep["packets"] == w["npackets"]
        print(f"{name}: n {len(data)}, {len(walks)} walks, last map {ms:.3f} ms")
    finally:
        sa.close()


@pytest.mark.parametrize("cfg", ["c1", "c2", "c5"])
def test_xz_parses(cfg):
    data = corpus.config_input("c1")[0] if cfg == "c1" else corpus.config_input(cfg)[0][: 1 << 14]
    sa = binding.SA(data, neighbours_per_step=64)
    try:
        for props in [(0, 0, 0), (3, 0, 2), (0, 2, 0)]:
            assert_device_equals_host(sa, data, xz_parse(data, *props), props, f"{cfg} xz {props}")
    finally:
        sa.close()


@pytest.mark.parametrize("base", ["enwik4k", "doubled", "two_periods", "edge", "far9k"])
def test_random_parses_with_stale_entries(base):
    data, slab = rp.base(base)
    sa = binding.SA(data, neighbours_per_step=64)
    try:
        m1, r1, _ = assert_device_equals_host(sa, data, slab, None, base)
        m2, r2, _ = assert_device_equals_host(sa, data, _validity.poisoned(slab), None, base + " poisoned")
        assert (m1 == m2).all() and r1 == r2
        assert_device_equals_host(sa, data, slab, tuple(rp.ALT_PROPS[k] for k in ("lc", "lp", "pb")), base + " alt")
    finally:
        sa.close()


def _search_pair(data, **kw):
    return binding.SA(data, neighbours_per_step=1024, **kw), binding.SA(data, neighbours_per_step=1024, **kw)


@pytest.mark.parametrize("fullwalk", [False, True], ids=["incremental", "fullwalk"])
def test_current_slab_and_the_search_left_untouched(fullwalk):
    """packets = NULL is the current slab; a handle that is asked for maps between two runs ends where one that is not ends"""
    data = C2[:8192] if fullwalk else C2[: 1 << 15]
    one, two = _search_pair(data, fullwalk=fullwalk)
    try:
        s1 = one.run(8)
        m1 = one.step_modes()
        two.run(4)
        m2a = two.step_modes()
        cur, cur_cost = two.current()
        null_map, null_rep = two.cost_map()
        cur_map, cur_rep = two.cost_map(cur)
        null_rep.pop("gpu_ms"), cur_rep.pop("gpu_ms")
        assert (null_map == cur_map).all() and null_rep == cur_rep and null_rep["total"] == cur_cost
        assert_device_equals_host(two, data, cur, None, "current")
        two.cost_map(None, (3, 0, 2))
        two.cost_map(xz_parse(data), (0, 2, 2))
        s2 = two.run(4)
        m2 = np.concatenate([m2a, two.step_modes()])
        (c1, cc1), (c2, cc2) = one.current(), two.current()
        assert sha_slab(c1) == sha_slab(c2) and cc1 == cc2
        assert one.best()[1] == two.best()[1] and s1["best_cost"] == s2["best_cost"] and s1["current_cost"] == s2["current_cost"]
        assert m1.tolist() == m2.tolist()
    finally:
        one.close()
        two.close()


def _raw(sa, slab, props=None, want_map=True, want_report=True):
    """(rc, map, report bytes): both buffers hold a sentinel beforehand"""
    out = np.full(sa.n, 0xA5A5A5A5, dtype=np.uint32)
    rep = (C.c_uint8 * C.sizeof(binding.CostReport))(*([0xA5] * C.sizeof(binding.CostReport)))
    slab = None if slab is None else np.ascontiguousarray(slab, dtype=PACKET)
    rc = sa.L.mgl_cost_map(sa.h, None if slab is None else slab.ctypes.data_as(C.c_void_p),
                           None if props is None else C.byref(binding.Properties(*props)),
                           out.ctypes.data_as(C.c_void_p) if want_map else None,
                           C.cast(rep, C.POINTER(binding.CostReport)) if want_report else None)
    return rc, out, bytes(rep)


def test_refusals_equal_cost_slab_and_leave_the_handle_usable():
    data, base, cases = _validity.cases()
    untouched = bytes([0xA5]) * C.sizeof(binding.CostReport)
    sa = binding.SA(data, neighbours_per_step=64, dict_limit=_validity.DICT_LIMIT)
    try:
        refused = 0
        for case in cases:
            slab = _validity.as_slab(case.slab)
            try:
                want_rc, want_total = 0, sa.cost_slab(slab, want_cum=False)["total"]
            except binding.MglError as e:
                want_rc, want_total = e.rc, None
            # the walk of mgl_cost_slab refuses an entry that is no packet; what it makes of a packet with a wrong source the
            # header leaves open (tests/test_gpu_slab_validity.py), and mgl_cost_map does whatever it does
            assert want_rc != 0 if case.clause in _validity.MALFORMED else want_rc == 0 if case.clause is None else True, case.id
            rc, out, rep = _raw(sa, slab)
            assert rc == want_rc, case.id
            if rc:
                refused += 1
                assert rc == MGL_EINVAL and (out == 0xA5A5A5A5).all() and rep == untouched, case.id
            elif case.clause is None:
                assert_device_equals_host(sa, data, slab, None, case.id)
            else:
                got = binding.CostReport.from_buffer_copy(rep)
                assert got.total == want_total == int(out.astype(np.int64).sum()) == sum(got.class_cost) == sum(got.type_cost), case.id
                assert sum(got.type_bytes) == len(data), case.id
        assert refused >= 13
        good = _validity.as_slab(base)
        # an unsupported triple; either output alone
        for props in [(4, 1, 0), (0, 5, 0), (0, 0, 5)]:
            rc, out, rep = _raw(sa, good, props)
            assert rc == MGL_EINVAL and (out == 0xA5A5A5A5).all() and rep == untouched
        assert sa.L.mgl_cost_map(None, None, None, None, None) == MGL_EINVAL
        want_map, want = binding.host_cost_map(data, good)
        rc, out, rep = _raw(sa, good, want_report=False)
        assert rc == 0 and (out == want_map).all() and rep == untouched
        rc, out, rep = _raw(sa, good, want_map=False)
        assert rc == 0 and (out == 0xA5A5A5A5).all() and binding.CostReport.from_buffer_copy(rep).total == want["total"]
        # no room for the call's buffers: MGL_ENOMEM once, then the same call goes through
        sa.debug_set(binding.KEY.COSTMAP_NOMEM, 1)
        rc, out, rep = _raw(sa, good)
        assert rc == MGL_ENOMEM and (out == 0xA5A5A5A5).all() and rep == untouched
        assert_device_equals_host(sa, data, good, None, "after ENOMEM")
        # the search still runs and nothing is pending
        st = sa.run(2)
        assert st["steps"] == 2
        cur, cost = sa.current()
        assert sa.cost_slab(cur, want_cum=False)["total"] == cost
        assert_device_equals_host(sa, data, cur, None, "after the refusals")
    finally:
        sa.close()


def _cli(tmp_path, data, extra, tag):
    f = tmp_path / "in.bin"
    f.write_bytes(data)
    slab = tmp_path / f"slab_{tag}"
    r = subprocess.run([build.CLI, "--epochs", "1", "--phases", "1", "--steps", "20", "--save-slab", str(slab)] + extra + [str(f)],
                       capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-600:]
    assert lzma.decompress(r.stdout, format=lzma.FORMAT_ALONE) == data
    return r.stdout, r.stderr.decode(), slab


def test_cli_cost_map_report_and_buckets(tmp_path):
    data = corpus.config_input("c1")[0]
    n = len(data)
    plain, err0, _ = _cli(tmp_path, data, [], "plain")
    assert "cost-" not in err0
    mapfile = tmp_path / "map.u32"
    stream, err, slabfile = _cli(tmp_path, data, ["--cost-map", str(mapfile), "--cost-report", "--cost-bucket", "512"], "map")
    assert stream == plain
    # the saved slab is the emitted one: its cost through the binding
    raw = slabfile.read_bytes()
    assert raw[:8] == b"MGLSLAB1" and int.from_bytes(raw[8:16], "little") == n
    saved_cost = int.from_bytes(raw[16:24], "little")
    slab = np.frombuffer(raw[24:], dtype=PACKET).copy()
    sa = binding.SA(data, neighbours_per_step=64)
    try:
        total = sa.cost_slab(slab, want_cum=False)["total"]
        want_map, want = sa.cost_map(slab)
    finally:
        sa.close()
    assert total == saved_cost == want["total"]
    got_map = np.frombuffer(mapfile.read_bytes(), dtype="<u4")
    assert len(got_map) == n and int(got_map.astype(np.int64).sum()) == total and (got_map == want_map).all()
    head = re.findall(r"^cost-report: total ([\d.]+) B exact (\d+) packets (\d+) lc=0 lp=0 pb=0 [\d.]+ ms$", err, re.M)
    assert len(head) == 1 and int(head[0][1]) == total and int(head[0][2]) == want["packets"] and head[0][0] == f"{total / 16384:.3f}"
    rows = re.findall(r"^cost-class: (\w+) bits (\d+) cost ([\d.]+) B share ([\d.]+) % exact (\d+)$", err, re.M)
    assert [r[0] for r in rows] == binding.COST_CLASSES
    assert [int(r[4]) for r in rows] == want["class_cost"] and [int(r[1]) for r in rows] == want["class_bits"]
    assert sum(int(r[4]) for r in rows) == total
    assert all(r[2] == f"{int(r[4]) / 16384:.3f}" and r[3] == f"{100 * int(r[4]) / total:.2f}" for r in rows)
    rows = re.findall(r"^cost-type: (\w+) packets (\d+) bytes (\d+) cost ([\d.]+) B share ([\d.]+) % exact (\d+)$", err, re.M)
    assert [r[0] for r in rows] == binding.PACKET_TYPES
    assert [int(r[5]) for r in rows] == want["type_cost"] and [int(r[1]) for r in rows] == want["type_packets"]
    assert [int(r[2]) for r in rows] == want["type_bytes"] and sum(int(r[2]) for r in rows) == n
    rows = re.findall(r"^cost-bucket: offset (\d+) bytes (\d+) cost ([\d.]+) B bpb ([\d.]+) exact (\d+)$", err, re.M)
    assert [int(r[0]) for r in rows] == list(range(0, n, 512)) and sum(int(r[1]) for r in rows) == n
    assert [int(r[4]) for r in rows] == [int(want_map[o:o + 512].astype(np.int64).sum()) for o in range(0, n, 512)]
    # each option alone: the same stream, only its own lines
    alone_r, err_r, _ = _cli(tmp_path, data, ["--cost-report"], "r")
    alone_b, err_b, _ = _cli(tmp_path, data, ["--cost-bucket", "4096"], "b")
    assert alone_r == plain and "cost-class:" in err_r and "cost-bucket:" not in err_r
    assert alone_b == plain and "cost-class:" not in err_b and len(re.findall(r"^cost-bucket: ", err_b, re.M)) == 1
