"""Inputs whose frontier list at one chosen position is known in advance, so that the limits of the frontier match finder
(mgl_matchfinder.hip; the rule is `frontier_rule` in tests/test_match_frontier_cpu.py) are reached on purpose.  Test
infrastructure only: pure Python, no GPU, no oracle.

A pattern T is drawn from random.Random(seed).  An occurrence of length L is T[:L] followed by the separator T[L] ^ 0xFF, so
its match against T is exactly L bytes long.  The occurrences come first, the longest step farthest back, and T itself
starts at position i: seen from i, every step's occurrences are nearer than those of every longer step.  Each generator
returns (data, i).

What tests/test_frontier_planted_cpu.py asserts about them, against `frontier_rule`:

  ladder(1, 75)                                 at depth >= 52 the list at i has exactly 60 entries (lengths 2..61 of the 74
                                                on offer) and spends 52 of the budget; at depth 40 it has 48 entries
  stairs(7, [(12, N), (40, 1)])                 8-byte run: the far source is the run's entry of ordinal N (1-based), taken
                                                iff depth >= N
  stairs(7, [(20, N), (40, 1)])                 the same in the 16-byte run
  stairs(11, [(10, 70), (24, 130), (50, 1)])    70 of the budget go in the 8-byte run, 130 in the 16-byte run
  stairs(12, [(15, 1), (40, 1)])                best == 15 from the direct look-ups: the look-up at need == 16 is free
  stairs(13, [(10, 1), (15, 1), (40, 1)])       best == 15 out of the 8-byte run
  stairs(13, [(10, 1), (15, 1), (16, 1), (40, 1)])   and the 16-byte run behind the free look-up
  stairs(14, [(12, 64), (300, 1)])              a match capped at 273
  stairs(14, [(12, 3), (100, 1)])               a match capped by the end of the input
  zero_run(), zero_tail()                       inputs that end like the zero padding behind them"""
import random

SEP = 0xFF


def stairs(seed, steps, tail=0):
    """steps = [(length, copies), ...], nearest first.  The file: `copies` occurrences of every step, the last step's
    first, then T[:max length + tail] from position i on."""
    longest = max(length for length, _ in steps)
    rng = random.Random(seed)
    T = bytes(rng.randrange(256) for _ in range(longest + tail + 1))
    out = bytearray()
    for length, copies in reversed(steps):
        out += (T[:length] + bytes([T[length] ^ SEP])) * copies
    i = len(out)
    out += T[:longest + tail]
    return bytes(out), i


def ladder(seed, lmax):
    """one occurrence of every length lmax .. 2, then T and 40 more bytes: from i the source of every length 2..lmax is
    nearer than every longer one"""
    return stairs(seed, [(length, 1) for length in range(2, lmax + 1)], tail=40)


def zero_run(n=700):
    """nothing but the byte the padding holds"""
    return b"\0" * n


def zero_tail(seed=15, block=200, run=300, tail=20):
    """a zero tail shorter than an earlier zero run: rnd + run zeros + rnd + tail zeros"""
    rng = random.Random(seed)
    rnd = bytes(rng.randrange(1, 256) for _ in range(block))
    return rnd + b"\0" * run + rnd + b"\0" * tail


def single_step(level_len, copies):
    """`copies` occurrences of `level_len` bytes (12: the scan stays in the 8-byte run; 20: in the 16-byte run) in front of
    one of 40: the long one is the run's entry of ordinal `copies`, counted from 1 beyond the nearest"""
    return stairs(7, [(level_len, copies), (40, 1)])


TWO_STEP = [(10, 70), (24, 130), (50, 1)]  # stairs(11, TWO_STEP)
EXACT_15 = {  # best == 15 on the way: name -> (seed, steps)
    "direct": (12, [(15, 1), (40, 1)]),
    "scanned": (13, [(10, 1), (15, 1), (40, 1)]),
    "scanned_16": (13, [(10, 1), (15, 1), (16, 1), (40, 1)]),
}
CAPPED = {"273": (14, [(12, 64), (300, 1)]), "end": (14, [(12, 3), (100, 1)])}
SINGLE_COPIES = (63, 64, 65, 128, 129)


def all_planted():
    """every planted input by name: what has to hold on all of them (brute force == rule at unlimited depth)"""
    out = {"ladder": ladder(1, 75), "two_step": stairs(11, TWO_STEP), "window_mid": stairs(7, [(12, 100), (40, 1)]),
           "zero_run": (zero_run(), 0), "zero_tail": (zero_tail(), 0)}
    for length in (12, 20):
        for copies in SINGLE_COPIES:
            out[f"single_{length}x{copies}"] = single_step(length, copies)
    for name, (seed, steps) in {**EXACT_15, **CAPPED}.items():
        out[f"stairs_{name}"] = stairs(seed, steps)
    return out
