"""Every candidate segment of a parse costed under every lc/lp/pb on the device (mgl_props_sweep_spans, mgl_segment_cuts,
mgl_sa_segment_props, CLI --segment-props).  Every comparison is an exact integer: each entry of the
device's table against the host's segment cost (tests/test_segments_cpu.py ties that to the restatement), the whole-file span
against mgl_props_sweep, the cuts and the partition against tests/_segments.py.  `-m gpu`."""
import ctypes as C
import lzma
import re
import subprocess

import numpy as np
import pytest

import _segments as S
from conftest import sha_slab
from megalania_amd import binding, build, corpus
from megalania_amd.binding import DUMP, PACKET, PROPS_TRIPLES

pytestmark = pytest.mark.gpu

MGL_EINVAL, MGL_ERANGE = -1, -4
GRAIN = 1024


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build_all()


@pytest.fixture(scope="module")
def mixed():
    return S.mixed_input()


def check_table(sa, data, slab, cuts, what, null_slab=False):
    """device table == host table on every span and triple; the whole-file span == mgl_props_sweep"""
    m = len(cuts) - 1
    got, ms = sa.props_sweep_spans(cuts, None if null_slab else slab)
    want = S.host_table(data, slab, cuts)
    bad = np.argwhere(got != want)
    print(f"{what}: n {len(data)}, {m} leaves, {len(got)} spans, {got.size} walks, {ms:.3f} ms, {len(bad)} mismatches")
    assert got.shape == want.shape == (m * (m + 1) // 2, 75) and got.dtype == np.uint64
    assert not len(bad), (what, [(int(s), PROPS_TRIPLES[int(t)], int(got[s, t]), int(want[s, t])) for s, t in bad[:5]])
    whole, _ = sa.props_sweep(None if null_slab else slab)
    assert got[S.span_index(0, m, m)].tolist() == whole.tolist(), what
    return got


@pytest.mark.parametrize("fullwalk", [False, True], ids=["incremental", "fullwalk"])
def test_spans_equal_host_on_the_search_s_own_slabs(mixed, fullwalk):
    """the greedy seed's slab and the slab 20 steps later, read where they lie (packets == NULL) and handed in"""
    sa = binding.SA(mixed, neighbours_per_step=256, fullwalk=fullwalk)
    try:
        sa.seed_greedy(16)
        for name in ("greedy", "20 steps"):
            cur, cost = sa.current()
            cuts = sa.segment_cuts(GRAIN)
            assert cuts == S.grain_cuts(cur, GRAIN) == sa.segment_cuts(GRAIN, cur) and len(cuts) - 1 <= 8
            tab = check_table(sa, mixed, cur, cuts, name, null_slab=True)
            assert (tab == sa.props_sweep_spans(cuts, cur)[0]).all()
            assert int(tab[S.span_index(0, len(cuts) - 1, len(cuts) - 1), 0]) == cost  # the handle's own 0/0/0
            # the chained call is the three calls in a row
            res = sa.segment_props(GRAIN)
            want, total = S.partition(tab, cuts, binding.SEG_OVERHEAD)
            assert (S.as_tuples(res["segments"]), res["total"]) == (want, total)
            assert res["single_best"] == int(tab[S.span_index(0, len(cuts) - 1, len(cuts) - 1)].min()) >= res["total"]
            assert res == {**sa.segment_props(GRAIN, cur), "gpu_ms": res["gpu_ms"]}
            sa.run(20)
    finally:
        sa.close()


def test_the_mixed_input_is_written_in_two_segments(mixed):
    """the device's partition of the encoder's parse pays, and its stream decodes"""
    slab = S.xz_parse(mixed)
    sa = binding.SA(mixed, neighbours_per_step=64)
    try:
        res = sa.segment_props(GRAIN, slab)
    finally:
        sa.close()
    assert len(res["segments"]) >= 2 and res["total"] < res["single_best"]
    stream = binding.emit_xz_segments(mixed, mixed, slab, res["segments"])
    assert lzma.decompress(stream) == mixed


REPEATED = (b"The quick brown fox jumps over the lazy dog, and the dog, who had seen it all before, did not so much as lift an ear. " * 40)[:4096]


@pytest.mark.parametrize("name,grain", [("lorem", 512), ("paragraph", 512), ("zeros", 256)])
def test_cuts_inside_rep_chains(name, grain):
    """parses that are chains of rep packets -- 273-byte LONG_REP 0 on the repeated paragraph and on zeros -- cut in their middle:
    the first packet of nearly every span is re-expressed.  zeros at the finest grain: a cut at every 273-byte packet but the first."""
    data = {"lorem": corpus.lorem(4096), "paragraph": REPEATED, "zeros": bytes(4096)}[name]
    slab = S.xz_parse(data)
    cuts = S.grain_cuts(slab, grain)
    starts = S.walk_starts(slab)
    if name != "lorem":
        on_rep = [c for c in cuts[1:-1] if int(slab[c]["type"]) in (binding.LONG_REP, binding.SHORT_REP)]
        assert on_rep and max(int(slab[p]["len"]) for p in starts[:-1]) == 273, (name, cuts)
    if name == "zeros":
        assert len(cuts) >= 15
    sa = binding.SA(data, neighbours_per_step=64)
    try:
        assert sa.segment_cuts(grain, slab) == cuts
        check_table(sa, data, slab, cuts, name)
    finally:
        sa.close()


@pytest.mark.parametrize("n", [8200, 131149])
def test_sizes_off_the_window_s_edge(n):
    """n no multiple of 64, grain 0 = 65536.  8 200 bytes are one leaf, one span.  131 149 bytes have the candidates 65 536 and
    131 072 (the rule's k g' below n), 77 bytes before the end: walks that start in the middle of the file and cross the 64-position
    window's refills from there, and a last leaf shorter than a window"""
    data = corpus.config_input("c5")[0][70_000:70_000 + n]
    slab = S.xz_parse(data)
    starts = S.walk_starts(slab)
    sa = binding.SA(data, neighbours_per_step=64)
    try:
        cuts = sa.segment_cuts(0, slab)
        assert cuts == S.grain_cuts(slab, 0) == ([0, n] if n == 8200 else S.grain_cuts(slab, 65536))
        if n == 131149:
            assert cuts[0] == 0 and cuts[-1] == n and len(cuts) in (3, 4) and 65536 <= cuts[1] < 65536 + 273
        check_table(sa, data, slab, cuts, f"n {n} grain 0")
        if n == 8200:
            mid = [next(p for p in starts if p >= x) for x in (n // 3 + 1, 2 * n // 3 + 5)]
            check_table(sa, data, slab, [0] + mid + [n], f"n {n} cuts {mid}")
            fine = sa.segment_cuts(1000, slab)
            assert fine == S.grain_cuts(slab, 1000) and len(fine) == 10
            check_table(sa, data, slab, fine, "n 8200 grain 1000")
    finally:
        sa.close()


def test_the_handle_s_triple_plays_no_part(mixed):
    slab = S.xz_parse(mixed)
    cuts = S.grain_cuts(slab, 2048)
    a = binding.SA(mixed, neighbours_per_step=64)
    b = binding.SA(mixed, neighbours_per_step=64, lc=3, lp=0, pb=2)
    try:
        ta = check_table(a, mixed, slab, cuts, "handle 0/0/0")
        tb = check_table(b, mixed, slab, cuts, "handle 3/0/2")
        assert (ta == tb).all()
        ra, rb = a.segment_props(2048, slab), b.segment_props(2048, slab)
        assert ra["segments"] == rb["segments"] and (ra["total"], ra["single_best"]) == (rb["total"], rb["single_best"])
        b.seed_greedy(16)  # its current slab, costed under its own 3/0/2, through the NULL path
        cur, cost = b.current()
        cc = b.segment_cuts(2048)
        t = check_table(b, mixed, cur, cc, "handle 3/0/2, current slab", null_slab=True)
        assert int(t[S.span_index(0, len(cc) - 1, len(cc) - 1), PROPS_TRIPLES.index((3, 0, 2))]) == cost
    finally:
        a.close()
        b.close()


def _raw_spans(sa, slab, cuts, cap):
    cuts = np.ascontiguousarray(cuts, dtype=np.uint64)
    out = np.full(max(cap, 1), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    cnt = C.c_size_t(12345)
    rc = sa.L.mgl_props_sweep_spans(sa.h, None if slab is None else slab.ctypes.data_as(C.c_void_p), cuts.ctypes.data_as(C.c_void_p),
                                    len(cuts), out.ctypes.data_as(C.c_void_p), cap, C.byref(cnt), None)
    return rc, cnt.value, out


def test_contract_and_refusals(mixed):
    n = len(mixed)
    slab = np.ascontiguousarray(S.xz_parse(mixed), dtype=PACKET)
    starts = S.walk_starts(slab)
    on = set(starts)
    a, b = starts[len(starts) // 3], starts[2 * len(starts) // 3]
    off = next(p for p in range(1, n) if p not in on)       # the first position inside a packet
    off_a = next(p for p in range(a + 1, n) if p not in on)  # and the first one behind a
    assert off < a < off_a < n
    sa = binding.SA(mixed, neighbours_per_step=64)
    try:
        alloc0 = sa.debug_dump(DUMP.ALLOCATIONS).tolist()
        rc, cnt, out = _raw_spans(sa, slab, [0, a, b, n], 6 * 75)
        assert rc == 0 and cnt == 450 and (out != 0xA5A5A5A5A5A5A5A5).all()
        # a buffer that is too small: the count, nothing written
        rc, cnt, out = _raw_spans(sa, slab, [0, a, b, n], 449)
        assert rc == MGL_ERANGE and cnt == 450 and (out == 0xA5A5A5A5A5A5A5A5).all()
        # a cut off the walk, as first, middle or last inner cut
        for cuts, bad_cut in (([0, off, n], off), ([0, a, off_a, n], off_a), ([0, off, a, n], off)):
            rc, cnt, out = _raw_spans(sa, slab, cuts, 6 * 75)
            assert rc == MGL_ERANGE and (out == 0xA5A5A5A5A5A5A5A5).all(), cuts
            assert f"cut {bad_cut} " in sa.L.mgl_last_error().decode()
        # cuts that are no cuts
        eighteen = [0] + starts[1:17] + [n]
        assert len(eighteen) == 18 and eighteen == sorted(set(eighteen))
        for cuts in ([0, b, a, n], [0, a, a, n], [a, b, n], [0, a, b], [0, a, n + 1], [0], [], eighteen, [0, n, n]):
            rc, _, out = _raw_spans(sa, slab, cuts, 200 * 75)
            assert rc == MGL_EINVAL and (out == 0xA5A5A5A5A5A5A5A5).all(), cuts
        # the most cuts there may be: 136 spans, compared like any other table
        seventeen = [0] + starts[1:16] + [n]
        assert _raw_spans(sa, slab, seventeen, 136 * 75)[:2] == (0, 136 * 75)
        check_table(sa, mixed, slab, seventeen, "17 cuts")
        # what cost_slab refuses, the sweep and the cuts refuse
        type0 = slab.copy()
        type0[starts[3]]["type"] = 0
        off_end = binding.literal_slab(n)
        off_end[n - 1] = (binding.MATCH, 0, 5)
        for bad in (type0, off_end):
            with pytest.raises(binding.MglError) as e0:
                sa.cost_slab(bad, want_cum=False)
            assert e0.value.rc == MGL_EINVAL
            assert _raw_spans(sa, bad, [0, n], 75)[0] == MGL_EINVAL
            for call in (lambda: sa.segment_cuts(GRAIN, bad), lambda: sa.segment_props(GRAIN, bad)):
                with pytest.raises(binding.MglError) as e:
                    call()
                assert e.value.rc == MGL_EINVAL
        assert sa.L.mgl_props_sweep_spans(None, None, None, 0, None, 0, None, None) == MGL_EINVAL
        # too little room for the segments: the count
        segs = (binding.Segment * 1)()
        nseg = C.c_size_t(0)
        rc = sa.L.mgl_sa_segment_props(sa.h, slab.ctypes.data_as(C.c_void_p), GRAIN, segs, 1, C.byref(nseg), None, None, None)
        assert rc == MGL_ERANGE and nseg.value == len(sa.segment_props(GRAIN, slab)["segments"]) >= 2
        cuts17 = np.zeros(17, dtype=np.uint64)
        ncuts = C.c_size_t(0)
        assert sa.L.mgl_segment_cuts(sa.h, slab.ctypes.data_as(C.c_void_p), 1, cuts17.ctypes.data_as(C.c_void_p), 3, C.byref(ncuts)) == MGL_ERANGE
        assert ncuts.value == 17 == len(sa.segment_cuts(1, slab))  # capped at 16 leaves
        # the call's buffers died with it; the handle works
        assert sa.debug_dump(DUMP.ALLOCATIONS).tolist() == alloc0
        assert sa.run(2)["steps"] == 2
        cur, cost = sa.current()
        assert sa.cost_slab(cur, want_cum=False)["total"] == cost
    finally:
        sa.close()


@pytest.mark.parametrize("fullwalk", [False, True], ids=["incremental", "fullwalk"])
def test_search_state_is_untouched(mixed, fullwalk):
    """a handle that is asked for cuts, tables and partitions between two runs ends where one that is not ends; current slab, costs,
    the next step's neighbours and the allocation count read the same before and after"""
    foreign = S.xz_parse(mixed)
    one = binding.SA(mixed, neighbours_per_step=256, fullwalk=fullwalk)
    two = binding.SA(mixed, neighbours_per_step=256, fullwalk=fullwalk)
    try:
        for sa in (one, two):
            sa.seed_greedy(16)
        s1 = one.run(8)
        m1 = one.step_modes()
        two.run(4)
        m2a = two.step_modes()
        before = (sha_slab(two.current()[0]), two.current()[1], two.best()[1], two.neighbours(4, want_diffs=False)[0].tolist(),
                  two.debug_dump(DUMP.ALLOCATIONS).tolist())
        cuts = two.segment_cuts(GRAIN)
        two.props_sweep_spans(cuts)
        two.segment_props(GRAIN)
        two.props_sweep_spans(S.grain_cuts(foreign, 2048), foreign)
        two.segment_props(0, foreign)
        with pytest.raises(binding.MglError):
            two.props_sweep_spans([0, 5, 3, len(mixed)])
        after = (sha_slab(two.current()[0]), two.current()[1], two.best()[1], two.neighbours(4, want_diffs=False)[0].tolist(),
                 two.debug_dump(DUMP.ALLOCATIONS).tolist())
        assert before == after
        s2 = two.run(4)
        m2 = np.concatenate([m2a, two.step_modes()])
        (c1, cc1), (c2, cc2) = one.current(), two.current()
        assert sha_slab(c1) == sha_slab(c2) and cc1 == cc2
        assert one.best()[1] == two.best()[1] and s1["best_cost"] == s2["best_cost"] and s1["current_cost"] == s2["current_cost"]
        assert m1.tolist() == m2.tolist()
    finally:
        one.close()
        two.close()


def test_cli_end_to_end(mixed, tmp_path):
    """one run on the 8 KiB input: the stream decodes, its chunks reset where the `segment:` lines say, and the lines are the
    figures the library gives for the slab the run saved"""
    f = tmp_path / "in.bin"
    f.write_bytes(mixed)
    saved = tmp_path / "best.slab"
    seed = tmp_path / "seed.lzma"  # the search starts from the encoder's parse, whose halves want different triples
    seed.write_bytes(lzma.compress(mixed, format=lzma.FORMAT_ALONE,
                                   filters=[dict(id=lzma.FILTER_LZMA1, preset=S.EXTREME, dict_size=1 << 22, lc=0, lp=0, pb=0)]))
    run = ["--seed-stream", str(seed), "--epochs", "1", "--phases", "1", "--steps", "20", "--neighbours", "1024"]
    r = subprocess.run([build.CLI, "--format", "xz", "--segment-props", str(GRAIN), "--save-slab", str(saved)] + run + [str(f)],
                       capture_output=True, timeout=600)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-800:]
    assert lzma.decompress(r.stdout) == mixed
    head = re.findall(r"^segment-props: grain (\d+) cuts (\d+) spans (\d+) single lc=(\d) lp=(\d) pb=(\d) ([\d.]+) B exact (\d+) "
                      r"segmented ([\d.]+) B exact (\d+) segments (\d+) [\d.]+ ms$", err, re.M)
    assert len(head) == 1, err[-800:]
    grain, ncuts, spans, lc, lp, pb, single_b, single, seg_b, total, nseg = head[0]
    rows = re.findall(r"^segment: offset (\d+) bytes (\d+) lc=(\d) lp=(\d) pb=(\d) cost ([\d.]+) B exact (\d+) reexpressed (\d+)$", err, re.M)
    assert int(grain) == GRAIN and len(rows) == int(nseg) and int(spans) == (int(ncuts) - 1) * int(ncuts) // 2
    assert single_b == f"{int(single) / 16384:.3f}" and seg_b == f"{int(total) / 16384:.3f}"
    assert all(row[5] == f"{int(row[6]) / 16384:.3f}" for row in rows)
    # the segments tile the file; their costs sum to the segmented figure minus the overheads
    assert [int(row[0]) for row in rows] == [0] + [int(row[0]) + int(row[1]) for row in rows[:-1]]
    assert int(rows[-1][0]) + int(rows[-1][1]) == len(mixed)
    assert sum(int(row[6]) for row in rows) == int(total) - (len(rows) - 1) * binding.SEG_OVERHEAD
    assert int(nseg) >= 2 and int(total) < int(single)  # 25 B on the encoder's own parse (tests/test_xz_segments_cpu.py); 20 steps move little
    assert len(r.stdout) < len(binding.emit_xz(mixed, mixed, np.frombuffer(saved.read_bytes()[24:], dtype=PACKET), int(lc), int(lp), int(pb)))
    # the same figures from the library, for the slab the run saved
    raw = saved.read_bytes()
    assert raw[:8] == b"MGLSLAB1"
    slab = np.frombuffer(raw[24:], dtype=PACKET).copy()
    sa = binding.SA(mixed, neighbours_per_step=64)
    try:
        res = sa.segment_props(GRAIN, slab)
        whole, _ = sa.props_sweep(slab)
        assert len(sa.segment_cuts(GRAIN, slab)) == int(ncuts)
    finally:
        sa.close()
    assert (res["total"], res["single_best"]) == (int(total), int(single))
    assert (int(lc), int(lp), int(pb)) == binding.best_props(whole)
    assert [(s["lo"], s["hi"] - s["lo"], *s["props"], s["cost"]) for s in res["segments"]] == \
        [(int(row[0]), int(row[1]), int(row[2]), int(row[3]), int(row[4]), int(row[6])) for row in rows]
    for s, row in zip(res["segments"], rows):
        assert binding.host_segment_cost(mixed, slab, s["lo"], s["hi"], s["props"]) == (s["cost"], int(row[7]))
    # the stream is the writer's, and its chunks reset at the segments' starts with their props bytes
    assert r.stdout == binding.emit_xz_segments(mixed, mixed, slab, res["segments"])
    resets = [(c[0], c[1]) for c in S.lzma2_chunks(r.stdout) if c[0] != 0x80]
    assert resets == [(0xE0 if k == 0 else 0xC0, S.props_byte(s["props"])) for k, s in enumerate(res["segments"])]
    # without the option the same run writes the single-triple stream, and no such line
    r0 = subprocess.run([build.CLI, "--format", "xz"] + run + [str(f)], capture_output=True, timeout=600)
    assert r0.returncode == 0 and lzma.decompress(r0.stdout) == mixed and b"segment-props:" not in r0.stderr and b"segment: " not in r0.stderr
    assert r0.stdout == binding.emit_xz(mixed, mixed, slab)
    print(f"cli: {len(r0.stdout)} B plain, {len(r.stdout)} B segmented, {nseg} segments")
