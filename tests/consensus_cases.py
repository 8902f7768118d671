"""The lists the consensus tests share (tests/test_consensus_cpu.py, tests/test_gpu_consensus.py): name -> (hypotheses, weights),
and want(name) = the definition's answer (tests/consensus_ref.py), computed once per process and never changed."""
import functools
import random
import struct

import consensus_ref as R

# every boundary of the kernel's layout (4 columns per lane, 64 lanes, 256 rows), in an order that puts the longer sequence of
# a pair first as often as second, and an empty hypothesis against a full one
LENGTHS = [255, 0, 1, 129, 3, 4, 128, 5, 63, 252, 64, 65, 127]
A, B, C = 7, 8, 9


def _seq(rng, n, alphabet):
    return [rng.choice(alphabet) for _ in range(n)]


def _build():
    rng = random.Random(20260)
    c = {}
    # 2 to 3 symbols: many optimal alignments exist, so the preference of the way back decides the mask
    c["lengths"] = ([_seq(rng, n, (A, B, C)) for n in LENGTHS], [1.0 if i % 2 else 2.0 ** -40 for i in range(len(LENGTHS))])
    c["one"] = ([_seq(rng, 5, (A, B))], [1.0])
    c["one_empty"] = ([[]], [0.0])
    same = _seq(rng, 65, (A, B, C))
    c["identical"] = ([same, list(same)], [0.5, 0.5])                              # D = 0, an exact tie: index 0
    c["disjoint"] = ([[1] * 64, [2] * 65], [0.0, 1.0])                             # D = the longer length; one-hot
    top = 2 ** 31 - 1
    c["high_bits"] = ([[5, 5 + 2 ** 16, top], [5, 5, top], [5 + 2 ** 16, 5, -top - 1]], [0.5, 0.0, 0.5])
    c["tie"] = ([[1, 2, 3], [1, 2, 4], [1, 2, 5]], [0.4, 0.4, 0.2])               # risk_0 == risk_1 < risk_2
    c["five"] = ([_seq(rng, n, (A, B)) for n in (5, 63, 4, 65, 64)], [0.2] * 5)
    c["wide"] = ([_seq(rng, 129 if i == 40 else 65 if i == 3 else (i * 7) % 13, (A, B, C)) for i in range(64)],
                 [1.0 / (i + 3) for i in range(64)])                              # products that round: a fused multiply-add shows
    # consensus_pick's ROW dimension: a dominant weight forces the winner to a long hypothesis (its risk stays below 1, every
    # other's is at least its distance to it), the small non-dyadic weights of the others keep their masks visible in conf
    for n in (255, 252, 129, 128):
        k = LENGTHS.index(n)
        c["rows_%d" % n] = (c["lengths"][0], [1.0 if i == k else 2.0 ** -12 / (i + 3) for i in range(len(LENGTHS))])
    # 64 hypotheses against a winner of 255 ids: every wave (j mod 4) walks back over full rows against a long, a short and an
    # empty hypothesis
    long_at = {0: 255, 5: 255, 6: 252, 7: 129, 8: 128}
    c["rows_wide"] = ([_seq(rng, long_at.get(i, (0, 1, 3, 4, 5, 2, 6, 7)[i % 8]), (A, B, C)) for i in range(64)],
                      [1.0 if i == 0 else 2.0 ** -14 / (i + 3) for i in range(64)])
    # the preferences of the way back, by hand (the winner is hypothesis 0; HAND_MASKS is the second one's mask)
    for name, x, y in (("ab_ba", [A, B], [B, A]), ("aab_ab", [A, A, B], [A, B]), ("ab_aab", [A, B], [A, A, B]), ("abc_c", [A, B, C], [C])):
        c[name] = ([x, y], [0.75, 0.25])
    return c


CASES = _build()
WINNER_LEN = {"rows_255": 255, "rows_252": 252, "rows_129": 129, "rows_128": 128, "rows_wide": 255}
HAND_MASKS = {"ab_ba": [0, 0], "aab_ab": [0, 1, 1], "ab_aab": [1, 1], "abc_c": [0, 0, 1]}


def bits(v):
    """the float64 bit patterns of v"""
    return [struct.pack("<d", float(x)) for x in v]


def same(got, wanted):
    """a ConsensusResult against want(name): integers equal, floats bit for bit"""
    w, risk, conf, D = wanted
    return got.winner == w and got.D.tolist() == D and bits(got.risk) == bits(risk) and bits(got.conf) == bits(conf)


@functools.lru_cache(maxsize=None)
def want(name):
    return R.consensus(*CASES[name])
