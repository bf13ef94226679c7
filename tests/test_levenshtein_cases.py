"""CPU checks of the Levenshtein edge cases: the word-level transcription of the
kernel loop equals the plain DP at 64 bits, and the defects the cases exist to
catch do change a distance on them.
"""

import levenshtein_cases as lc


def _run(**kw):
    chars, lens = lc.packed()
    rows, ln = chars.tolist(), lens.tolist()
    return {p: lc.myers(rows, ln, p[0], p[1], **kw) for p in lc.distinct_pairs()}


def test_cases_are_what_they_claim():
    s = lc.strings()
    assert len(s) == 2 * len(lc.LENGTHS) + len(lc.EXTRA)
    assert sorted({len(t) for t in s}) == lc.LENGTHS
    chars, lens = lc.packed()
    for i, t in enumerate(s):
        assert int(lens[i]) == len(t)
        assert (chars[i, len(t):] == lc.PAD).all()
    p = lc.pairs()
    n = len(s)
    assert len(p) == n * (n + 1) and len(lc.distinct_pairs()) == n * n
    exp = lc.expected()
    assert all(exp[(i, i)] == 0 for i in range(n))
    assert all(exp[(i, j)] == exp[(j, i)] for i, j in p)


def test_transcription_equals_dp_at_64_bits():
    got, exp = _run(bits=64), lc.expected()
    bad = [(p, got[p], exp[p]) for p in exp if got[p] != exp[p]]
    assert not bad, bad[:5]


def test_63_bit_word_differs_for_every_string_of_length_64():
    got, exp = _run(bits=63), lc.expected()
    s = lc.strings()
    long_ones = [i for i, t in enumerate(s) if len(t) == 64]
    assert len(long_ones) == 2 + len(lc.EXTRA)
    for i in long_ones:
        assert any(got[p] != exp[p] for p in exp if i in p), s[i]
    # nothing shorter than 64 reaches the top bit
    assert all(got[p] == exp[p] for p in exp if len(s[p[0]]) < 64 and len(s[p[1]]) < 64)


def test_no_swap_is_an_optimisation_and_a_half_swap_is_a_defect():
    """Every string fits the 64-bit word and the distance is symmetric, so
    taking the first string as the pattern without any swap computes the same
    distances: the swap only shortens the Eq loop. What the (j, i) pairs and
    the ``ord("a")`` padding catch is a swap done by half: lengths without
    pointers reads past the shorter string, pointers without lengths cuts the
    longer one."""
    exp = lc.expected()
    none = _run(swap="none")
    assert all(none[p] == exp[p] for p in exp)
    s = lc.strings()
    for how in ("lens", "ptrs"):
        got = _run(swap=how)
        differing = [p for p in exp if got[p] != exp[p]]
        print(f"swap='{how}': {len(differing)} of {len(exp)} pairs differ")
        assert differing
        # only pairs that take the swap branch can differ
        assert all(len(s[i]) > len(s[j]) for i, j in differing)
