"""Differential tests against the REFERENCE implementation itself.

tests/golden/reference_differential.json.gz holds, per property, a fixed
seeded set of hypothesis-drawn inputs with what the reference's own
consensus/alignment/consolidation code returned for each (or the exception it
raised); scripts/record_reference_goldens.py recorded it from a reference
checkout. Each test runs THIS implementation on the same inputs and asserts
exact agreement — parity against the reference's code, not a re-derivation,
without needing the reference to run the suite.

Where the reference crashed, only its documented crash classes may be
skipped (hardened divergences, docs/PARITY.md); the entry points with crash
parity must raise the same exception type.
"""

import asyncio
import gzip
import importlib
import json
import math
import os
import random

import pytest

from kllms_amd.consensus import (
    ConsensusSettings,
    consensus_values,
    lists_alignment,
    low_cutoff_bound,
    recursive_list_alignments,
    remove_outliers,
    sort_by_original_majority,
)
from kllms_amd.consensus import fuzzy_key_selection, key_selection
from kllms_amd.consensus.aio import async_consolidate_chat_completions
from kllms_amd.consensus.consolidation import consolidate_chat_completions
from kllms_amd.consensus.key_based_alignment import recursive_align
from kllms_amd.consensus.similarity import (
    compute_similarity_scores,
    generic_similarity,
    normalize_string,
    numerical_similarity,
    sanitize_value,
)
from kllms_amd.consensus.values import intermediary_consensus_cleanup

GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                           "golden", "reference_differential.json.gz")


@pytest.fixture(scope="module")
def golden():
    with gzip.open(GOLDEN_PATH, "rt") as f:
        return json.load(f)


def _hashable(v):
    return tuple(_hashable(x) for x in v) if isinstance(v, list) else v


def _dec(v):
    """Inverse of the recorder's encoding: {"__items__": [[k, v], ...]} is a
    dict with non-string keys; everything else is plain JSON."""
    if isinstance(v, dict):
        if set(v) == {"__items__"}:
            return {_hashable(_dec(k)): _dec(x) for k, x in v["__items__"]}
        return {k: _dec(x) for k, x in v.items()}
    if isinstance(v, list):
        return [_dec(x) for x in v]
    return v


def _deep_eq(a, b, path="", tol=1e-9):
    if isinstance(a, float) and isinstance(b, float):
        assert (math.isnan(a) and math.isnan(b)) or a == pytest.approx(b, abs=tol), f"{path}: {a} != {b}"
        return
    if isinstance(a, dict) and isinstance(b, dict):
        assert set(a) == set(b), f"{path}: keys {set(a)} != {set(b)}"
        for k in a:
            _deep_eq(a[k], b[k], f"{path}.{k}", tol)
        return
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        assert len(a) == len(b), f"{path}: len {len(a)} != {len(b)}"
        for i, (x, y) in enumerate(zip(a, b)):
            _deep_eq(x, y, f"{path}[{i}]", tol)
        return
    assert a == b, f"{path}: {a!r} != {b!r}"


def _approx(tol):
    def check(got, want, label):
        assert got == pytest.approx(want, abs=tol), label
    return check


def _known_ref_crash(crash, _rerun):
    """Only the documented reference crash classes may be skipped; anything
    else means the recording miscalled the reference (which would make every
    comparison silently vacuous)."""
    msg = crash["msg"]
    known = (
        "unhashable" in msg                      # Counter on list/dict votes
        or "has no len()" in msg                 # key-aligner None-mixed lists
        or "'<' not supported" in msg            # key-aligner mixed-type key sort
        or crash["type"] == "builtins.RecursionError"
    )
    assert known, f"unexpected reference crash treated as divergence: {crash['type']}: {msg}"


def _same_crash(crash, rerun):
    """Crash parity: ours must fail with the SAME exception type (e.g.
    all-empty contents -> likelihoods=1.0 -> pydantic rejects; ValueError
    "No extractions" / "No scalar candidate paths" in key selection)."""
    mod, _, qual = crash["type"].rpartition(".")
    with pytest.raises(getattr(importlib.import_module(mod), qual)):
        rerun()


def _same_crash_unless_unhashable(crash, rerun):
    if "unhashable" not in crash["msg"]:   # documented hardening divergence
        _same_crash(crash, rerun)


def _replay(golden, name, n_cases, ours, check=_deep_eq, on_crash=_known_ref_crash):
    """Run ours(input) on every recorded case of property `name` (at least
    n_cases, the count the property was fuzzed at — a truncated recording
    must not pass) and compare with the reference's recorded result."""
    cases = golden[name]
    assert len(cases) >= n_cases, f"{name}: {len(cases)} recorded cases < {n_cases}"
    for i, c in enumerate(cases):
        x = json.loads(json.dumps(c["in"]))   # fresh copy per case
        if "crash" in c:
            on_crash(c["crash"], lambda: ours(x))
        else:
            check(ours(x), _dec(c["want"]), f"{name} case {i}: {c['in']!r}")


def fake_embed(texts):
    return [[float(len(t) % 7) + 0.25, float(sum(map(ord, t)) % 11), 1.0] for t in texts]


def _lev():
    return ConsensusSettings(string_similarity_method="levenshtein")


def test_generic_similarity_matches_reference(golden):
    _replay(golden, "generic_similarity", 150,
            lambda x: generic_similarity(x[0], x[1], "levenshtein", fake_embed), check=_approx(1e-9))


def test_consensus_values_matches_reference(golden):
    _replay(golden, "consensus_values", 120, lambda v: consensus_values(v, _lev(), fake_embed))


def test_recursive_alignment_matches_reference(golden):
    _replay(golden, "recursive_alignment", 80,
            lambda v: recursive_list_alignments(v, "levenshtein", fake_embed, None, 0.51))


def test_lists_alignment_matches_reference(golden):
    def sim(a, b):
        return generic_similarity(a, b, "levenshtein", fake_embed)

    _replay(golden, "lists_alignment", 80, lambda v: lists_alignment(v, sim, min_support_ratio=0.51))


def test_numeric_consensus_matches_reference(golden):
    """Hybrid numeric clustering incl. tie-breaks by cross-cluster support,
    signless and power-of-10 equivalence (ref :1127-1219), on clustered
    number lists with power-of-10 / signless twins."""
    _replay(golden, "numeric_consensus", 200,
            lambda v: consensus_values(v, ConsensusSettings(), fake_embed))


def test_similarity_methods_match_reference(golden):
    """All four string-similarity methods, incl. the >50-char embeddings gate
    falling back to levenshtein below it (ref :797-824)."""
    _replay(golden, "similarity_methods", 150,
            lambda x: generic_similarity(x[0], x[1], x[2], fake_embed), check=_approx(1e-9))


def test_long_string_embeddings_consensus_matches_reference(golden):
    """string_consensus 'centroid' on long strings routes through the
    embeddings medoid on both sides (same injected embedder)."""
    _replay(golden, "long_string_embeddings_consensus", 60,
            lambda v: consensus_values(v, ConsensusSettings(), fake_embed))


# ---------------------------------------------------------------------------
# Full consolidation differential (the reference's §3.1 entry point)
# ---------------------------------------------------------------------------

def _mk_completion(contents):
    from kllms_amd.types.openai_compat import (
        ChatCompletion, ChatCompletionMessage, Choice, CompletionUsage,
    )

    return ChatCompletion(
        id="chatcmpl-difftest",
        choices=[
            Choice(finish_reason="stop", index=i,
                   message=ChatCompletionMessage(role="assistant", content=c))
            for i, c in enumerate(contents)
        ],
        created=1700000000,
        model="diff-model",
        usage=CompletionUsage(prompt_tokens=10, completion_tokens=5 * len(contents),
                              total_tokens=10 + 5 * len(contents)),
    )


def _completion_eq(got, want, label):
    """want: the recorded summary of a reference completion — choices as
    [index, finish_reason, content], likelihoods, usage dump."""
    assert [[g.index, g.finish_reason, g.message.content] for g in got.choices] == want["choices"], label
    _deep_eq(got.likelihoods, want["likelihoods"], f"{label} likelihoods")
    assert got.usage.model_dump() == want["usage"], label


def test_consolidate_chat_completions_matches_reference(golden):
    _replay(golden, "consolidate_chat_completions", 100,
            lambda c: consolidate_chat_completions(_mk_completion(c), fake_embed),
            check=_completion_eq, on_crash=_same_crash_unless_unhashable)


def test_async_consolidation_matches_reference(golden):
    """The reference's ASYNC consolidation is hand-duplicated code (not a
    bridge) and has genuinely drifted from its own sync path on bool/number
    mixtures (e.g. contents 0 vs false: sync -> numeric consensus 0.0 at
    confidence 0.5, async -> enum-like 0 at confidence 1.0). Ours is one
    shared impl bridged to async, so it matches the reference's SYNC
    behavior everywhere — asserted here; where the reference's async agrees
    with its sync, ours must match it too (docs/PARITY.md)."""
    async def aembed(texts):
        return fake_embed(texts)

    def check(got, want, label):
        sync, asyn = want["sync"], want["async"]
        _completion_eq(got, sync, f"{label} (sync)")   # ours always equals the reference's SYNC behavior
        # and equals the async result wherever the reference hasn't drifted
        if ([c[2] for c in asyn["choices"]] == [c[2] for c in sync["choices"]]
                and asyn["likelihoods"] == sync["likelihoods"]):
            assert [g.message.content for g in got.choices] == [c[2] for c in asyn["choices"]], label
            _deep_eq(got.likelihoods, asyn["likelihoods"], f"{label} likelihoods(async)")

    _replay(golden, "async_consolidation", 60,
            lambda c: asyncio.run(async_consolidate_chat_completions(_mk_completion(c), aembed)),
            check=check, on_crash=_same_crash_unless_unhashable)


# ---------------------------------------------------------------------------
# Key-based aligner differential (C42-C44, the dormant-but-shipped L1b)
# ---------------------------------------------------------------------------

def _records(lists_of_records):
    return [r for lst in lists_of_records for r in lst]


def test_key_based_recursive_align_matches_reference(golden):
    """Record-shaped candidates (lists of dicts with scalar fields — what
    key-based alignment exists for) plus arbitrary JSON for its fallbacks."""
    _replay(golden, "key_based_recursive_align", 100, lambda v: recursive_align(v, "levenshtein", 0.5))


def test_key_selection_matches_reference(golden):
    """The cascade's chosen alignment keys must match (C42/C43)."""
    _replay(golden, "key_selection", 100,
            lambda v: key_selection.select_best_keys(_records(v)).model_dump(), on_crash=_same_crash)


def test_compute_similarity_scores_matches_reference(golden):
    _replay(golden, "compute_similarity_scores", 100,
            lambda v: list(compute_similarity_scores(v, _lev(), fake_embed)))


def test_sort_by_original_majority_matches_reference(golden):
    """Condorcet column ordering (C41): identical aligned permutations feed
    both implementations; identity-keyed original-position lookup must agree."""
    def ours(originals):
        rng = random.Random(sum(len(o) for o in originals))
        perm = list(range(min(len(o) for o in originals)))
        rng.shuffle(perm)
        # identity lookup requires the SAME cell objects; ints are interned for
        # this value range, so aligned and originals share identities
        aligned = [[row[j] for j in perm] for row in originals]
        got = sort_by_original_majority(aligned, [list(o) for o in originals])
        return [list(got[0]), list(got[1])]

    _replay(golden, "sort_by_original_majority", 100, ours)


def test_intermediary_cleanup_matches_reference(golden):
    _replay(golden, "intermediary_cleanup", 120, intermediary_consensus_cleanup)


def test_outlier_cutoff_matches_reference(golden):
    def check(got, want, label):
        assert got[0] == pytest.approx(want[0], abs=1e-12), label
        _deep_eq(got[1], want[1], label)

    _replay(golden, "outlier_cutoff", 120,
            lambda d: [low_cutoff_bound(list(d)), remove_outliers(list(d))], check=check)


def test_string_normalization_matches_reference(golden):
    """normalize_string + sanitize_value: the voting/similarity equivalence
    keys (transliteration itself is the shared stub; the lower/strip/regex
    logic is independent code on each side)."""
    def check(got, want, label):
        assert got == want, label

    _replay(golden, "string_normalization", 200,
            lambda s: [normalize_string(s), sanitize_value(s)], check=check)


def test_numerical_similarity_matches_reference(golden):
    _replay(golden, "numerical_similarity", 200,
            lambda x: numerical_similarity(x[0], x[1]), check=_approx(1e-12))


def test_fuzzy_key_selection_matches_reference(golden):
    """C43: canonicalized (fuzzy) key cascade and the fuzzy-fallback picker
    must agree with the reference, incl. the stability-tuple tie-break."""
    _replay(golden, "fuzzy_key_selection", 100,
            lambda v: fuzzy_key_selection.select_best_keys_with_fuzzy_fallback(_records(v)).model_dump(),
            on_crash=_same_crash)
