"""The validity rule of slabs (tests/_validity.py) and its table of cases, without a GPU.

1. The table meets the rule it was built for: every refused case violates exactly one clause, at one packet, and together
   the cases cover every clause and every placement (the edges of a bitmap word and of a block of 256 threads, the first
   non-literal packet, the last packet).
2. The host gate (slab_is_valid in front of the emitters, host/mgl_host.c) refuses exactly the refused cases, names the
   clause and the position on stderr, and what it accepts decodes to the input.
3. mgl_pk_wellformed (csrc/mgl_model.h), the predicate every walk of an outside slab asks before it plans an entry: what it
   passes plans inside the probability table and without a context twice, and it fails exactly the entries the table's
   malformed cases plant.

tests/test_gpu_slab_validity.py runs the same table through the device's gates."""
import lzma
import os
import subprocess

import pytest

import _validity as V
from megalania_amd import binding

DATA, BASE, CASES = V.cases()
BY_ID = {c.id: c for c in CASES}
IDS = [c.id for c in CASES]
FULL_WINDOW = 0x400000
PROPS = [(0, 0, 0), (2, 1, 2)]

# what slab_is_valid prints for a clause (the window's reason is the one for a declared dictionary other than 4 MiB)
HOST_REASON = {
    V.NOT_A_PACKET: "not a packet",
    V.LITERAL_LONG: "literal longer than one byte",
    V.SHORT_REP_LONG: "short rep longer than one byte",
    V.LENGTH_RANGE: "match length outside 2..273",
    V.REP_INDEX: "rep index above 3",
    V.BEFORE_START: "distance reaches before the start of the input",
    V.OUTSIDE_WINDOW: "distance outside the declared dictionary",
    V.BYTES_DIFFER: "does not reproduce the input",
}


# ---- 1. the table

@pytest.mark.parametrize("cid", IDS)
def test_case_meets_its_expectation_under_the_rule(cid):
    c = BY_ID[cid]
    first = V.violations(DATA, c.slab, V.DICT_LIMIT)
    along = V.violations(DATA, c.slab, V.DICT_LIMIT, every=True)
    if c.clause is None:
        assert first == [] and along == []
        return
    # one clause, at one packet, and nothing else wrong on the rest of the walk: a gate without that clause lets it pass
    assert len(first) == 1 and first[0][1] == c.clause and along == first, (first, along)
    twin = BY_ID[c.twin]
    assert twin.clause is None
    diff = [int(p) for p in range(V.N) if tuple(c.slab[p]) != tuple(twin.slab[p])]
    assert diff == [p for p, _ in c.edits] and len(diff) == 1, diff
    assert V.on_walk(twin.slab)[diff[0]] and V.on_walk(c.slab)[diff[0]]
    if cid == "rep-stack-shift":
        # the edited MATCH is a valid packet with a valid source: the packet that fails is one the edit did not touch
        assert first[0][0] != diff[0] and tuple(c.slab[first[0][0]]) == tuple(BASE[first[0][0]])
    else:
        assert first[0][0] == diff[0]


def test_the_table_covers_every_clause_line_and_placement():
    refused = [c for c in CASES if c.clause is not None]
    assert {c.clause for c in refused} == set(V.CLAUSES)
    assert {c.line for c in CASES} == set(range(14)) | {15}
    where = {c.id: V.violations(DATA, c.slab, V.DICT_LIMIT)[0][0] for c in refused}
    for name, holds in V.PLACEMENTS.items():
        hit = [cid for cid, p in where.items() if holds(p)]
        assert hit, name
        print(name, hit)
    # a malformed entry and a copy of wrong bytes at both edges of a block of 256 threads
    for edge in (255, 0):
        kinds = {BY_ID[cid].clause in V.MALFORMED for cid, p in where.items() if p % 256 == edge}
        assert kinds == {True, False}, edge
    # every refused case has its accepted twin, and some accepted case differs from the base only off the walk
    assert all(BY_ID[c.twin].clause is None for c in refused)
    on = V.on_walk(BASE)
    poison = BY_ID["poison"].slab
    assert all(tuple(poison[p]) == tuple(BASE[p]) for p in range(V.N) if on[p])
    off = [tuple(int(x) for x in poison[p]) for p in range(V.N) if not on[p]]
    assert any(t == 0 for t, _, _ in off) and any(t == 9 for t, _, _ in off)
    assert any(l == 0 for _, _, l in off) and any(l == 60000 for _, _, l in off)


def test_the_base_parse_holds_what_the_cases_need():
    on = V.on_walk(BASE)
    walked = [tuple(int(x) for x in BASE[p]) for p in range(V.N) if on[p]]
    assert {t for t, _, _ in walked} == {V.LITERAL, V.MATCH, V.SHORT_REP, V.LONG_REP}
    assert {d for t, d, _ in walked if t == V.LONG_REP} == {0, 1, 2, 3}
    assert (V.MATCH, 0, 273) in walked                       # the overlapping copy
    assert DATA[:V.RUN] == b"a" * V.RUN and len(DATA) == V.N == 773 and V.DICT_LIMIT == 256
    # stale entries off the walk: well-formed, and many of them no valid packet where they lie
    stale = [(p, tuple(int(x) for x in BASE[p])) for p in range(V.N) if not on[p]]
    assert all(V.wellformed(*e) for _, e in stale) and sum(e[0] != V.LITERAL for _, e in stale) > 200
    assert any(e[0] == V.MATCH and p > V.RUN and (e[1] + 1) % V.PERIOD for p, e in stale)


# ---- 2. the host gate

def _emit(slab, window, lc, lp, pb):
    if window == FULL_WINDOW:
        return binding.emit_stream(DATA, slab, lc, lp, pb)
    return binding.emit_stream_dict(DATA, slab, window, lc, lp, pb)


@pytest.mark.parametrize("window", [FULL_WINDOW, V.DICT_LIMIT], ids=["emit_stream", "emit_stream_dict-256"])
@pytest.mark.parametrize("cid", IDS)
def test_host_gate_refuses_exactly_the_refused_cases_and_says_why(cid, window, capfd):
    """mgl_emit_stream has the fixed 4 MiB window, under which the window's case is a valid parse; mgl_emit_stream_dict
    takes the table's 256.  The host does not compare a SHORT_REP's distance with the window (the device does): harmless,
    because a rep distance was a MATCH's distance, which it compared when that MATCH was walked -- no case can tell."""
    c = BY_ID[cid]
    want = V.violations(DATA, c.slab, window)
    valid_here = c.clause is None or (c.clause == V.OUTSIDE_WINDOW and window == FULL_WINDOW)
    assert [cl for _, cl in want] == ([] if valid_here else [c.clause])
    capfd.readouterr()
    if want:
        with pytest.raises(binding.MglError):
            _emit(c.slab, window, 0, 0, 0)
        err = capfd.readouterr().err
        assert f"slab entry at {want[0][0]}: " in err and HOST_REASON[want[0][1]] in err, err
        assert sum(reason in err for reason in set(HOST_REASON.values())) == 1, err
        return
    for lc, lp, pb in PROPS:
        stream = _emit(c.slab, window, lc, lp, pb)
        assert lzma.decompress(stream, format=lzma.FORMAT_ALONE) == DATA
    assert capfd.readouterr().err == ""


# ---- 3. the shared predicate

def test_what_the_predicate_passes_plans_inside_the_table(tmp_path):
    exe = tmp_path / "wellformed"
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "wellformed_main.c")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=gnu11", "-O1", "-Wall", "-Wextra", "-Werror", "-o", str(exe), src])
    planted = [(c, e) for c in CASES for _, e in c.edits]
    r = subprocess.run([str(exe)], input="".join(f"{t} {d} {l}\n" for _, (t, d, l) in planted), capture_output=True, text=True)
    lines = r.stdout.splitlines()
    print("\n".join(lines[-3:]))
    assert r.returncode == 0 and lines[-1].endswith(" 0 misses") and not lines[-1].startswith("0 plans"), lines[-5:]
    grid = {}
    for ln in lines:
        f = ln.split()
        if len(f) == 4 and all(x.isdigit() for x in f):
            grid[(int(f[0]), int(f[1]), int(f[2]))] = int(f[3])
    # the whole grid, against the rule restated in Python
    want = {(t, d, l): int(V.wellformed(t, d, l)) for t in (0, 1, 2, 3, 4, 5, 255) for l in list(range(301)) + [65535]
            for d in (0, 1, 2, 3, 4, 5, 0xFFFFFFFF)}
    assert grid == want, [k for k in want if grid.get(k) != want[k]][:10]
    assert sum(want.values()) == 7 + 7 + 272 * 7 + 272 * 4  # literal, short rep, MATCH 2..273 (any distance), LONG_REP 2..273 x 4
    # the entries the table plants: malformed exactly in the refused cases of lines 1, 3, 4 and 5 (line 2's packet is one,
    # it only does not fit; lines 6 to 13 plant packets whose sources are wrong)
    answers = [ln.split() for ln in lines if ln.startswith("? ")]
    assert len(answers) == len(planted)
    for (c, e), a in zip(planted, answers):
        assert tuple(int(x) for x in a[1:4]) == e
        assert int(a[4]) == (0 if c.clause is not None and c.line in (1, 3, 4, 5) else 1), (c.id, e, a)
        assert (c.clause in V.MALFORMED and c.line != 2) == (c.clause is not None and c.line in (1, 3, 4, 5)), c.id
