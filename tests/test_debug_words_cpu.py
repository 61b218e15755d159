"""The control blocks that kernels and host share (megalania_amd/csrc/mgl_words.h) and the names of the debug hooks
(include/megalania_hip.h), as megalania_amd/binding.py sees them.  The layouts come from the host C compiler: a stand-alone
program that includes mgl_words.h prints every struct's size and every field's offset and size.  The numbers of the
selectors, keys, limits and give-up bits are the ABI; the literal lists below are its one numeric copy.  No GPU."""
import os
import re
import subprocess

import numpy as np

from megalania_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS_H = os.path.join(ROOT, "megalania_amd", "csrc", "mgl_words.h")

DUMP_VALUES = ([*range(0, 17), 18, 19, *range(21, 29), *range(30, 36), *range(40, 46), *range(50, 56), *range(60, 66),
                *range(70, 78), *range(80, 88)])
SITES = ["apply_events", "apply_guard", "apply_sub", "apply_span", "apply_pieces", "apply_pool", "apply_jobs", "apply_span_area",
         "apply_scratch", "apply_shift", "cl_journal", "cl_order", "walk_ops", "walk_events", "walk_guard", "walk_invalid",
         "walk_overrun", "ch_sub", "ch_span_area", "ch_shift", "ch_pool", "ch_jobs", "ch_scratch", "ch_runs", "forced_early",
         "forced_late", "ch_span_rerun"]


def _structs():
    """{struct: [field names]} as mgl_words.h declares them (`a, b` and `a[4]` declarators included)"""
    text = re.sub(r"/\*.*?\*/", "", open(WORDS_H).read(), flags=re.S)
    out = {}
    for body, name in re.findall(r"typedef struct \w+ \{(.*?)\} (\w+);", text, re.S):
        decls = [d.split()[-1] for stmt in body.split(";") if stmt.strip() for d in stmt.split(",")]
        out[name] = [re.sub(r"\[\d+\]", "", d) for d in decls]
    return out


def _compiled_layout(tmp_path):
    """{struct: (size, [(field, offset, size)])} from a program the host C compiler builds around mgl_words.h"""
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "mgl_words.h"', "int main(void) {"]
    for name, fields in _structs().items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'printf("{name}.{f} %zu %zu\\n", offsetof({name}, {f}), sizeof((({name}*)0)->{f}));' for f in fields]
    lines += ["return 0;", "}"]
    src, exe = tmp_path / "words.c", tmp_path / "words"
    src.write_text("\n".join(lines))
    subprocess.run([os.environ.get("CC", "cc"), "-std=c11", "-Wall", "-Wextra", "-Werror", f"-I{os.path.dirname(WORDS_H)}", "-o", str(exe), str(src)], check=True)
    out = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        what, *nums = line.split()
        if "." in what:
            out[what.split(".")[0]][1].append((what.split(".")[1], int(nums[0]), int(nums[1])))
        else:
            out[what] = (int(nums[0]), [])
    return out


def test_binding_dtypes_have_the_compiled_layout(tmp_path):
    layout = _compiled_layout(tmp_path)
    assert set(layout) == {"BulkHdr", "BatchHdr", "BatchAcc", "ApplyHdr", "PbAcc", "StepCounts"}
    assert {k: v[0] for k, v in layout.items()} == {"BulkHdr": 64, "BatchHdr": 64, "BatchAcc": 32, "ApplyHdr": 64, "PbAcc": 72, "StepCounts": 32}
    for name, dtype in (("BatchHdr", binding.BATCH_HDR), ("BatchAcc", binding.BATCH_ACC), ("ApplyHdr", binding.APPLY_HDR),
                        ("PbAcc", binding.PB_ACC), ("StepCounts", binding.STEP_COUNTS)):
        size, fields = layout[name]
        assert dtype.itemsize == size, name
        assert [(f, dtype.fields[f][1], dtype.fields[f][0].itemsize) for f in dtype.names] == fields, name
    # what the dumps of these blocks hand out: the whole struct, but the builder's totals stop before PbAcc's last field
    table = binding.DUMP_DTYPE
    assert table[binding.DUMP.BATCH_HDR] == binding.BATCH_HDR and table[binding.DUMP.APPLY_HDR] == binding.APPLY_HDR
    assert table[binding.DUMP.BATCH_ACC] == binding.BATCH_ACC and table[binding.DUMP.STEP_COUNTS] == binding.STEP_COUNTS
    head = table[binding.DUMP.PBUILD_TOTALS]
    assert head.names == binding.PB_ACC.names[:-1] and head.itemsize == binding.PB_ACC.fields["left"][1]
    assert all(head.fields[f] == binding.PB_ACC.fields[f] for f in head.names)
    assert table[binding.DUMP.PICKSTATE].itemsize == 32 and table[binding.DUMP.PICKSTATE].fields["mutated"][1] == 7 * 4
    assert set(table) == set(binding.DUMP)


def test_enums_are_the_frozen_numbers():
    assert [(m.name, int(m)) for m in binding.LIM] == [(m.name, i + 1) for i, m in enumerate(binding.LIM)] and len(binding.LIM) == 18
    assert [(m.name.lower(), int(m)) for m in binding.GU] == [(name, 1 << bit) for bit, name in enumerate(SITES)] and len(SITES) == 27
    assert [int(m) for m in binding.KEY] == list(range(12)) and binding.KEY.PROBE_FORM == 11
    assert sorted(int(m) for m in binding.DUMP) == DUMP_VALUES
    assert [int(m) for m in binding.BATCH] == [0, 1, 2, 3]
    for e in (binding.DUMP, binding.KEY, binding.LIM, binding.GU, binding.BATCH):
        assert len(e.__members__) == len(list(e)), e  # an alias would be a value that occurs twice
    header = open(os.path.join(ROOT, "include", "megalania_hip.h")).read()
    raw = binding._header_enum("mgl_dump_selector", "MGL_DUMP_")
    assert len(raw) == len({v for _, v in raw}) == len(re.findall(r"\bMGL_DUMP_[A-Z0-9_]+ = ", header))
    assert dict(binding._header_enum("mgl_accept_limit", "MGL_LIM_"))["COUNT"] == 19
    assert np.dtype("u4") == binding.DUMP_DTYPE[binding.DUMP.GIVEUP_SITES]
