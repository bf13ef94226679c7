#!/usr/bin/env python3
"""Record the vectors that tests/test_reference_differential.py replays.

    PYTHONHASHSEED=0 python scripts/record_reference_goldens.py --reference /path/to/k-LLMs

Imports a reference checkout's consensus machinery with its uninstalled
third-party deps stubbed (Levenshtein / unidecode -> kllms_amd.utils.text,
cachetools.TTLCache -> dict, openai / retab -> inert types), draws a seeded
set of inputs per property, runs the REFERENCE on each and writes inputs +
results (or the exception raised) to tests/golden/. The inputs are seeded;
the reference sums over set unions, so without a fixed hash seed a few
results move in the last ulp. --mult N multiplies the example counts for
deep campaigns (write those to a scratch --out).
"""

import argparse
import asyncio
import gzip
import importlib.util
import json
import os
import random
import sys
import types
import zlib
from typing import TypeVar

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from hypothesis import HealthCheck, Phase, given, seed, settings, strategies as st  # noqa: E402

from kllms_amd.types import openai_compat as oc  # noqa: E402
from kllms_amd.utils.text import ascii_transliterate, levenshtein_distance  # noqa: E402


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    return sys.modules.setdefault(name, m)


def _cls(name):
    return type(name, (), {})


class _TTLCacheStub(dict):
    def __init__(self, maxsize=1024, ttl=300):
        super().__init__()
        self.maxsize = maxsize

    def __setitem__(self, k, v):
        if len(self) >= self.maxsize:
            self.clear()
        super().__setitem__(k, v)


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = sys.modules[name] = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _package(name, path):
    pkg = types.ModuleType(name)
    pkg.__path__ = [path]
    sys.modules.setdefault(name, pkg)


def load_reference(ref_root):
    """Load the reference's utils modules (as package _refk) and its
    consolidation entry point; the openai CHAT types are this repo's
    pydantic-compatible re-declarations, so the reference code runs on the
    same objects our implementation consumes."""
    pkg_dir = os.path.join(ref_root, "k_llms")
    utils = os.path.join(pkg_dir, "utils")
    _stub("Levenshtein", distance=levenshtein_distance)
    _stub("unidecode", unidecode=ascii_transliterate)
    _stub("cachetools", TTLCache=_TTLCacheStub)
    openai = _stub("openai", OpenAI=_cls("OpenAI"), AsyncOpenAI=_cls("AsyncOpenAI"))
    openai.types = _stub("openai.types")
    _stub("openai.types.completion_usage", CompletionUsage=_cls("CompletionUsage"),
          CompletionTokensDetails=_cls("CompletionTokensDetails"),
          PromptTokensDetails=_cls("PromptTokensDetails"))
    for name in ("retab", "retab.types", "retab.types.documents"):
        _stub(name)
    _stub("retab.types.documents.extract", RetabParsedChatCompletion=_cls("RetabParsedChatCompletion"))
    openai.types.chat = _stub("openai.types.chat", ChatCompletion=oc.ChatCompletion,
                              ParsedChatCompletion=oc.ParsedChatCompletion,
                              ChatCompletionMessage=oc.ChatCompletionMessage)
    _stub("openai.types.chat.chat_completion", Choice=oc.Choice)
    _stub("openai.types.chat.parsed_chat_completion", ParsedChoice=oc.ParsedChoice,
          ParsedChatCompletionMessage=oc.ParsedChatCompletionMessage)
    _stub("openai.lib")
    _stub("openai.lib._parsing", ResponseFormatT=TypeVar("ResponseFormatT"))

    _package("_refk", utils)
    for sub in ("majority_sorting", "consensus_utils", "key_selection",
                "fuzzy_key_selection", "key_based_alignment"):
        _load(f"_refk.{sub}", os.path.join(utils, f"{sub}.py"))
    _package("_refpkg", pkg_dir)
    _package("_refpkg.types", os.path.join(pkg_dir, "types"))
    _package("_refpkg.utils", utils)
    for sub in ("majority_sorting", "consensus_utils"):  # reuse for the relative imports
        sys.modules[f"_refpkg.utils.{sub}"] = sys.modules[f"_refk.{sub}"]
    _load("_refpkg.types.completions", os.path.join(pkg_dir, "types", "completions.py"))
    _load("_refpkg.types.parsed", os.path.join(pkg_dir, "types", "parsed.py"))
    return _load("_refpkg.utils.consolidation", os.path.join(utils, "consolidation.py"))


def fake_embed(texts):
    return [[float(len(t) % 7) + 0.25, float(sum(map(ord, t)) % 11), 1.0] for t in texts]


def mk_completion(contents):
    return oc.ChatCompletion(
        id="chatcmpl-difftest",
        choices=[oc.Choice(finish_reason="stop", index=i,
                           message=oc.ChatCompletionMessage(role="assistant", content=c))
                 for i, c in enumerate(contents)],
        created=1700000000,
        model="diff-model",
        usage=oc.CompletionUsage(prompt_tokens=10, completion_tokens=5 * len(contents),
                                 total_tokens=10 + 5 * len(contents)),
    )


def enc(v):
    """Plain JSON, except dicts with non-string keys (key mappings), which
    become {"__items__": [[key, value], ...]}; tuples become lists."""
    if isinstance(v, dict):
        if all(isinstance(k, str) for k in v) and "__items__" not in v:
            return {k: enc(x) for k, x in v.items()}
        return {"__items__": [[enc(k), enc(x)] for k, x in v.items()]}
    if isinstance(v, (list, tuple)):
        return [enc(x) for x in v]
    if hasattr(v, "item") and not isinstance(v, (bool, int, float, str)):
        return enc(v.item())  # numpy scalars
    return v


def completion_summary(c):
    return {"choices": [[ch.index, ch.finish_reason, ch.message.content] for ch in c.choices],
            "likelihoods": c.likelihoods, "usage": c.usage.model_dump()}


# strategies: ASCII-restricted so the transliteration stub is exercised
# identically on both sides
ascii_text = st.text(alphabet=st.characters(min_codepoint=0x20, max_codepoint=0x7E), max_size=14)
scalars = st.one_of(
    st.none(), st.booleans(), st.integers(min_value=-10**6, max_value=10**6),
    st.floats(allow_nan=False, allow_infinity=False, width=32), ascii_text,
)
json_values = st.recursive(
    scalars,
    lambda ch: st.one_of(
        st.lists(ch, max_size=3),
        st.dictionaries(st.sampled_from(["a", "b", "k1", "k2", "name"]), ch, max_size=3),
    ),
    max_leaves=8,
)
# targeted distributions for rarely-hit branches
_centers = st.sampled_from([0.0, 1.0, -1.0, 10.0, 0.001, -1000.0, 1e6])
_jitter = st.floats(min_value=-0.05, max_value=0.05, allow_nan=False)
clustered_numbers = st.lists(
    st.one_of(
        st.tuples(_centers, _jitter).map(lambda t: t[0] * (1.0 + t[1])),
        st.tuples(_centers, _jitter).map(lambda t: t[0] * (1.0 + t[1]) * 10.0),   # power-of-10 twins
        st.tuples(_centers, _jitter).map(lambda t: -t[0] * (1.0 + t[1])),         # signless twins
        st.none(),
        st.integers(min_value=-5, max_value=5),
    ),
    min_size=2, max_size=7,
)
content_strings = st.one_of(json_values.map(json.dumps), ascii_text)  # JSON or free text
# record-shaped candidates: lists of dicts with scalar fields (what key-based
# alignment exists for)
_record = st.dictionaries(
    st.sampled_from(["id", "name", "qty", "price", "tag"]),
    st.one_of(st.integers(min_value=0, max_value=30), ascii_text, st.none(),
              st.floats(allow_nan=False, allow_infinity=False, width=16)),
    min_size=1, max_size=4,
)
record_lists = st.lists(st.lists(_record, max_size=4), min_size=2, max_size=4)
numbers = st.one_of(st.booleans(), st.integers(-10**6, 10**6),
                    st.floats(allow_nan=False, allow_infinity=False))
json_lists = lambda lo, hi: st.lists(json_values, min_size=lo, max_size=hi)  # noqa: E731


def record(label, strategy, n, run_ref):
    """n examples of strategy, seeded by the label, each with the reference's
    result or crash (the test decides what parity means for a crash)."""
    inputs = []

    @seed(zlib.crc32(label.encode()))
    @settings(max_examples=n, database=None, deadline=None, phases=[Phase.generate],
              suppress_health_check=list(HealthCheck))
    @given(strategy)
    def collect(x):
        inputs.append(json.dumps(x))

    collect()
    cases = []
    for x in inputs:
        case = {"in": json.loads(x)}
        try:
            case["want"] = enc(run_ref(json.loads(x)))
        except Exception as e:
            case["crash"] = {"type": f"{type(e).__module__}.{type(e).__qualname__}", "msg": str(e)[:300]}
        cases.append(case)
    print(f"  {label}: {len(cases)} cases, {sum('crash' in c for c in cases)} reference crashes",
          file=sys.stderr)
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="reference checkout (the dir holding k_llms/)")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "reference_differential.json.gz"))
    ap.add_argument("--mult", type=int, default=1, help="example-count multiplier")
    args = ap.parse_args()

    con = load_reference(args.reference)
    ref, ms, sel, fuzzy, key = (sys.modules[f"_refk.{m}"] for m in (
        "consensus_utils", "majority_sorting", "key_selection", "fuzzy_key_selection",
        "key_based_alignment"))
    lev = lambda: ref.ConsensusSettings(string_similarity_method="levenshtein")  # noqa: E731
    flat = lambda lol: [r for lst in lol for r in lst]  # noqa: E731

    def ref_sim(a, b):
        return ref.generic_similarity(a, b, "levenshtein", fake_embed)

    async def aembed(texts):
        return fake_embed(texts)

    def both_consolidations(c):
        asyn = asyncio.run(con.async_consolidate_chat_completions(mk_completion(c), aembed, None))
        sync = con.consolidate_chat_completions(mk_completion(c), fake_embed, None)
        return {"sync": completion_summary(sync), "async": completion_summary(asyn)}

    def majority(originals):
        # the aligned permutation is derived from the input exactly as the test derives it
        rng = random.Random(sum(len(o) for o in originals))
        perm = list(range(min(len(o) for o in originals)))
        rng.shuffle(perm)
        aligned = [[row[j] for j in perm] for row in originals]
        got = ms.sort_by_original_majority(aligned, [list(o) for o in originals])
        return [list(got[0]), list(got[1])]

    properties = [  # (name, strategy, examples, reference call)
        ("generic_similarity", st.tuples(json_values, json_values), 150,
         lambda x: ref.generic_similarity(x[0], x[1], "levenshtein", fake_embed)),
        ("consensus_values", json_lists(1, 5), 120,
         lambda v: ref.consensus_values(v, lev(), fake_embed, None)),
        ("recursive_alignment", json_lists(2, 4), 80,
         lambda v: ref.recursive_list_alignments(v, "levenshtein", fake_embed, None, 0.51)),
        ("lists_alignment", st.lists(st.lists(ascii_text, max_size=4), min_size=2, max_size=4), 80,
         lambda v: ref.lists_alignment(v, ref_sim, None, min_support_ratio=0.51)),
        ("numeric_consensus", clustered_numbers, 200,
         lambda v: ref.consensus_values(v, ref.ConsensusSettings(), fake_embed, None)),
        ("similarity_methods",
         st.tuples(json_values, json_values, st.sampled_from(["jaccard", "hamming", "embeddings"])), 150,
         lambda x: ref.generic_similarity(x[0], x[1], x[2], fake_embed)),
        ("long_string_embeddings_consensus",
         st.lists(st.text(alphabet="abcdefgh ", min_size=45, max_size=70), min_size=2, max_size=4), 60,
         lambda v: ref.consensus_values(v, ref.ConsensusSettings(), fake_embed, None)),
        ("consolidate_chat_completions", st.lists(content_strings, min_size=1, max_size=5), 100,
         lambda c: completion_summary(con.consolidate_chat_completions(mk_completion(c), fake_embed, None))),
        ("async_consolidation", st.lists(content_strings, min_size=1, max_size=4), 60, both_consolidations),
        ("key_based_recursive_align", st.one_of(record_lists, json_lists(2, 4)), 100,
         lambda v: key.recursive_align(v, "levenshtein", 0.5)),
        ("key_selection", record_lists, 100, lambda v: sel.select_best_keys(flat(v)).model_dump()),
        ("compute_similarity_scores", json_lists(1, 5), 100,
         lambda v: list(ref.compute_similarity_scores(v, lev(), fake_embed))),
        ("sort_by_original_majority",
         st.lists(st.lists(st.integers(min_value=0, max_value=9), min_size=1, max_size=5),
                  min_size=2, max_size=4), 100, majority),
        ("intermediary_cleanup", json_values, 120, ref.intermediary_consensus_cleanup),
        ("outlier_cutoff",
         st.lists(st.floats(min_value=0.0, max_value=1.0, allow_nan=False), max_size=10), 120,
         lambda d: [ref.low_cutoff_bound(list(d)), ref.remove_outliers(list(d))]),
        ("string_normalization", ascii_text, 200, lambda s: [ref.normalize_string(s), ref.sanitize_value(s)]),
        ("numerical_similarity", st.tuples(numbers, numbers), 200,
         lambda x: ref.numerical_similarity(x[0], x[1])),
        ("fuzzy_key_selection", record_lists, 100,
         lambda v: fuzzy.select_best_keys_with_fuzzy_fallback(flat(v)).model_dump()),
    ]
    out = {name: record(name, strat, max(1, args.mult) * n, fn) for name, strat, n, fn in properties}

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as f:
        f.write(json.dumps(out, separators=(",", ":")).encode())
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes)", file=sys.stderr)


if __name__ == "__main__":
    main()
