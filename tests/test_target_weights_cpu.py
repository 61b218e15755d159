"""Target weights without a device: the Python restatement of the rule (tests/_weighted_targets.py) against the definition
taken position by position, mgl_weight_value against Python integers at the widths where a single 31-bit draw fails, its
refusals, and the four entry points in the header and in the library."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from _weighted_targets import DRAW2, brute_targets, targets, value
from megalania_amd import binding, build

MGL_EINVAL = -1
HEADER = os.path.join(os.path.dirname(os.path.abspath(build.__file__)), "..", "include", "megalania_hip.h")
NAMES = ["mgl_sa_set_target_weights", "mgl_sa_weight_targets_by_cost", "mgl_sa_target_weights", "mgl_weight_value"]


def tiny_cases():
    rng = np.random.default_rng(0x7E16)
    for n in (1, 2, 7, 40):
        for pattern in ("zeros", "ones", "mixed", "sparse"):
            if pattern == "zeros":
                w = np.zeros(n, dtype=np.uint32)
            elif pattern == "ones":
                w = np.ones(n, dtype=np.uint32)
            elif pattern == "mixed":
                w = rng.choice(np.array([0, 1, 7], dtype=np.uint32), size=n)
            else:
                w = np.zeros(n, dtype=np.uint32)
                w[rng.integers(0, n)] = 7
            starts = [0] + sorted(int(p) for p in np.nonzero(rng.integers(0, 3, size=n) == 0)[0] if p > 0)
            yield n, pattern, w, np.array(starts)


def test_helper_equals_the_definition_on_tiny_cases():
    L = binding.hip_lib()
    met, cases = {}, 0
    for n, pattern, w, starts in tiny_cases():
        windows = [None] + [(lo, hi) for lo in range(n) for hi in range(lo + 1, n + 1)]  # every window
        for k, window in enumerate(windows):
            for K in (1, 3):
                step = k % 5
                got = targets(L, w, starts, window, 99, step, K, info=met)
                assert got == brute_targets(L, w, starts, window, 99, step, K), (n, pattern, window, K)
                cases += 1
    assert cases > 3000 and met["empty_slice"] and met["below_lo"]


WIDTHS = lambda K: [1, K - 1, K, K + 1, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, 1 << 38, (1 << 44) - 1]  # noqa: E731


def test_weight_value_equals_python_integers():
    L = binding.hip_lib()
    single_draw_fails = 0
    for K in (1, 64, 4096, 1 << 20):
        for W in WIDTHS(K):
            if W == 0:
                continue  # K - 1 at K = 1: refused, below
            for j in sorted({0, 1, K // 2, K - 1}):
                if j >= K:
                    continue
                for seed, step in ((1673551, 0), (20260, 12345678901)):
                    v, a, b = value(L, W, K, j, seed, step)
                    assert binding.weight_value(W, K, j, seed, step) == v, (W, K, j, seed, step)
                    assert a <= v < max(b, a + 1) and (b > a or v == a)
                    if b > a:
                        u0 = int(L.mgl_rng_draw_at(seed, step, j, 0))
                        single_draw_fails += a + u0 % (b - a) != v
                    if b - a > 1 << 31:
                        assert int(L.mgl_rng_draw_at(seed, step, j, 0)) < 1 << 31 and int(L.mgl_rng_draw_at(seed, step, j, DRAW2)) < 1 << 31
    assert single_draw_fails > 20  # the second draw matters


def test_weight_value_reaches_above_one_draw():
    """a slice of 2^38: some neighbour's value lies above 2^31, which one 31-bit draw cannot give"""
    assert max(binding.weight_value(1 << 38, 1, 0, 7, step) for step in range(8)) >= 1 << 31


@pytest.mark.parametrize("W,K,j", [(0, 1, 0), (1 << 44, 1, 0), ((1 << 44) + 5, 64, 3), (1 << 63, 1, 0), (5, 0, 0), (5, (1 << 20) + 1, 0), (5, 4, 4), (5, 4, 5),
                                   (5, 1, 1), (0, 0, 0)])
def test_weight_value_refusals(W, K, j):
    L = binding.hip_lib()
    v = C.c_uint64(77)
    assert L.mgl_weight_value(W, K, j, 1, 2, C.byref(v)) == MGL_EINVAL and v.value == 77
    assert b"mgl_weight_value" in L.mgl_last_error()
    with pytest.raises(binding.MglError) as e:
        binding.weight_value(W, K, j, 1, 2)
    assert e.value.rc == MGL_EINVAL


def test_weight_value_refuses_a_null_result():
    L = binding.hip_lib()
    assert L.mgl_weight_value(5, 4, 3, 1, 2, None) == MGL_EINVAL
    v = C.c_uint64(0)
    assert L.mgl_weight_value((1 << 44) - 1, 1 << 20, (1 << 20) - 1, 1, 2, C.byref(v)) == 0 and v.value < (1 << 44) - 1  # the largest arguments


def test_header_declares_and_library_exports():
    text = open(HEADER).read()
    L = C.CDLL(build.HIP_SO)  # no device is touched by loading
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, text, re.M), name
        assert getattr(L, name) is not None and name in binding.HIP_SYMBOLS
    assert re.search(r"^int mgl_sa_set_target_weights\(mgl_sa\* sa, const uint32_t\* weights", text, re.M)
    assert re.search(r"^int mgl_sa_weight_targets_by_cost\(mgl_sa\* sa, const mgl_packet\* packets, uint32_t floor, uint64_t\* total, double\* gpu_ms\);", text, re.M)
    assert re.search(r"^int mgl_sa_target_weights\(mgl_sa\* sa, uint32_t\* weights_out, uint64_t\* total, uint64_t\* window\);", text, re.M)
    assert re.search(r"^int mgl_weight_value\(uint64_t W, uint32_t K, uint32_t j, uint64_t seed, uint64_t step, uint64_t\* v\);", text, re.M)
    for method in ("set_target_weights", "weight_targets_by_cost", "target_weights"):
        assert callable(getattr(binding.SA, method))
    assert len(list(itertools.islice(tiny_cases(), 3))) == 3


def test_null_handles_are_refused_without_a_device():
    L = binding.hip_lib()
    w = np.ones(4, dtype=np.uint32)
    t = C.c_uint64(0)
    assert L.mgl_sa_set_target_weights(None, w.ctypes.data_as(C.c_void_p)) == MGL_EINVAL
    assert L.mgl_sa_set_target_weights(None, None) == MGL_EINVAL
    assert L.mgl_sa_weight_targets_by_cost(None, None, 0, C.byref(t), None) == MGL_EINVAL
    assert L.mgl_sa_target_weights(None, None, C.byref(t), C.byref(t)) == MGL_EINVAL
