"""mgl_debug_dump and mgl_debug_set as a whole: every selector of `binding.DUMP` answers on an incremental handle with a
size that fits its element type (`binding.DUMP_DTYPE`); a handle of the full-walk engine answers three of them; numbers
outside the enums and null handles are refused; the give-up word is cleared by its dump.  Nothing is provoked and no step
runs beyond the three bulk steps of the fixture.  `-m gpu`."""
import ctypes as C

import numpy as np
import pytest

from megalania_amd import binding, corpus
from megalania_amd.binding import DUMP, KEY

pytestmark = pytest.mark.gpu

MGL_OK, MGL_EINVAL, MGL_ERANGE = 0, -1, -4
DATA = corpus.lorem(600)


def _dump(sa, what, cap):
    """(rc, *bytes, the buffer) of one raw call"""
    out = np.zeros(max(1, cap), dtype=np.uint8)
    need = C.c_size_t(1 << 60)
    rc = sa.L.mgl_debug_dump(sa.h, int(what), out.ctypes.data_as(C.c_void_p), cap, C.byref(need))
    return rc, need.value, out


@pytest.fixture(scope="module")
def incremental():
    sa = binding.SA(DATA, neighbours_per_step=64, accept="bulk")
    sa.run(3)
    yield sa
    sa.close()


@pytest.fixture(scope="module")
def fullwalk():
    sa = binding.SA(DATA, neighbours_per_step=64, fullwalk=True)
    yield sa
    sa.close()


def test_every_selector_answers_with_whole_elements(incremental):
    sa = incremental
    for d in DUMP:
        rc, need, _ = _dump(sa, d, 0)
        assert rc in (MGL_OK, MGL_ERANGE) and need < 1 << 60, d  # the size probe: *bytes is set either way
        assert rc == MGL_OK or need > 0, d
        assert need % binding.DUMP_DTYPE[d].itemsize == 0, (d, need)
        rc, got, _ = _dump(sa, d, need)
        assert rc == MGL_OK and got == need, d
        assert sa.debug_dump(d).nbytes == need, d


def test_fullwalk_handle_answers_three(fullwalk):
    sa = fullwalk
    for d in DUMP:
        rc, need, _ = _dump(sa, d, 1 << 16)
        if d in (DUMP.WINDOWS, DUMP.SOFT_ENDS, DUMP.ALLOCATIONS):
            assert rc == MGL_OK and need > 0, d
        else:
            assert rc == MGL_EINVAL and sa.L.mgl_last_error().decode() == "mgl_debug_dump: handle runs the full-walk engine", d


def test_numbers_outside_the_enums_and_null_handles_are_refused(incremental):
    sa = incremental
    for what in sorted(set(range(0, 100)) - {int(d) for d in DUMP}) + [1000, 0xFFFFFFFF]:
        assert _dump(sa, what, 1 << 16)[0] == MGL_EINVAL and sa.L.mgl_last_error().decode() == "mgl_debug_dump: unknown selector", what
    for key in (len(KEY), 50, 0xFFFFFFFF):
        assert sa.L.mgl_debug_set(sa.h, key, 0) == MGL_EINVAL and sa.L.mgl_last_error().decode() == "mgl_debug_set: unknown key", key
    for key in KEY:
        assert sa.L.mgl_debug_set(None, int(key), 0) == MGL_EINVAL, key


def test_the_giveup_word_is_cleared_by_its_dump(incremental):
    sa = incremental
    sa.giveup_sites()
    assert sa.giveup_sites() == 0
