"""The member encoder of palace_bgzf_deflate on a CPU (palace_amd/host/deflate_selftest_main.cpp runs the phases of
csrc/deflate_enc.hpp thread by thread) over the edge catalogue of tests/deflate_enc_cases.py: every member is read back with the
reader written from RFC 1951 (tests/deflate_read.py) and held to the exact model of tests/deflate_enc_model.py -- the one token
sequence the rules allow, trimmed counts, complete codes within 15 / 15 / 7 bits, the optimal coded size wherever the optimal
tree fits the limit, the stored decision (tests/deflate_enc_checks.py) -- and the bytes do not depend on where the text lies in
memory.  `enc_rank` + `enc_build_code` are also run on their own, on histograms no member can have.  The sanitizer build of the
same program runs the catalogue too.  The device is held to the same members in tests/test_gpu_bgzf_deflate_edges.py."""
import os
import subprocess

import numpy as np
import pytest

from tests import deflate_enc_cases as dc
from tests import deflate_enc_checks as ck
from tests import deflate_enc_model as dm
from tests import deflate_streams as ds


@pytest.fixture(scope="module")
def members(tmp_path_factory):
    ck.make(ck.TOOL)
    tmp = tmp_path_factory.mktemp("enc_edges")
    pieces = [p for _, p in dc.cases()]
    return [ck.host_members(tmp, pieces, mis) for mis in range(4)]


def test_the_catalogue_reaches_every_length_symbol_every_distance_code_and_a_tree_past_the_limit():
    """on the model alone: what the other tests check is what the rules make of these pieces"""
    lengths, dists, deep = set(), set(), []
    for name, piece in dc.cases():
        tokens, lit, dist, _ = ck.model_of(piece)
        assert dm.text_of(tokens) == piece, name
        lengths |= {s for s in range(257, 286) if lit[s]}
        dists |= {s for s in range(30) if dist[s]}
        if dm.huffman_cost(lit)[1] > 15:
            deep.append(name)
    assert lengths == set(range(257, 286))
    assert dists == set(range(30))
    assert deep
    far = dict(dc.cases())[f"distance_{dc.TOO_FAR}_no_match"]
    assert not any(t[0] == "match" for t in ck.model_of(far)[0])
    window = [t for t in ck.model_of(dict(dc.cases())["distance_32768"])[0] if t[0] == "match"]
    assert len(window) == -(-(dc.MAX_TEXT - 32768) // 258) and {t[2] for t in window} == {32768}
    overlapping = [n for n, p in dc.cases() if any(t[0] == "match" and t[2] < t[1] for t in ck.model_of(p)[0])]
    assert {f"distance_{d}" for d in range(1, 9)} <= set(overlapping)


def test_every_member_is_what_the_model_says(members):
    named = dc.cases()
    faults, btype = ck.catalogue_faults(named, members[0])
    assert not faults, faults[:20]
    assert len(btype) == len(named) and all(btype[n] in (0, 2) for n, p in named if p)


def test_the_coded_members_use_every_length_symbol_and_every_distance_code(members):
    """in blocks the encoder really wrote as dynamic ones (a piece of a few bytes is stored, whatever its tokens would be)"""
    lengths, dists = set(), set()
    for (name, piece), m in zip(dc.cases(), members[0]):
        _, kind, ls, dsy = ck.member_faults(piece, m)
        if kind == 2:
            lengths |= ls
            dists |= dsy
    assert lengths == set(range(257, 286)) and dists == set(range(30))
    by = {name: ck.member_faults(piece, m)[1] for (name, piece), m in zip(dc.cases(), members[0])}
    assert by["literal_tree_21_levels_deep"] == 2 and by[f"distance_{dc.TOO_FAR}_no_match"] == 2 and by["distance_32768"] == 2
    assert all(by[f"distance_{d}"] == 2 for d in dc.DISTANCES) and all(by[f"lines_{k}"] == 2 for k in dc.PAIR_LENGTHS)


def test_texts_that_barely_compress_fall_on_both_sides_of_the_stored_decision(members):
    kinds = [ck.member_faults(piece, m)[1] for (name, piece), m in zip(dc.cases(), members[0]) if name.startswith("barely_")]
    assert kinds[0] == 2 and kinds[-1] == 0 and kinds == sorted(kinds, reverse=True), kinds


def test_the_bytes_do_not_depend_on_the_misalignment(members):
    for mis in (1, 2, 3):
        differ = [name for (name, _), a, b in zip(dc.cases(), members[0], members[mis]) if a != b]
        assert not differ, (mis, differ[:10])


def test_the_sanitizer_build_runs_the_catalogue_clean(tmp_path):
    ck.make(ck.TOOL_ASAN)
    pieces = [p for _, p in dc.cases()]
    plain = ck.host_members(tmp_path, pieces, 3)
    assert ck.host_members(tmp_path, pieces, 3, tool=ck.TOOL_ASAN) == plain
    assert ck.host_members(tmp_path, pieces, 0, tool=ck.TOOL_ASAN) == plain


# ---- enc_rank + enc_build_code on their own -------------------------------------------------------------------------------------

def fibonacci(n, period):
    fib = [1, 2]
    while len(fib) < period:
        fib.append(fib[-1] + fib[-2])
    return [fib[i % period] for i in range(n)]


def histograms():
    """[(name, symbols, bit limit, frequencies)]; every sum stays below 2^32, as the encoder's 32-bit weights need"""
    rng = np.random.default_rng(1952)
    out = [("fibonacci_19_limit_7", 19, 7, fibonacci(19, 19)), ("fibonacci_30_limit_15", 30, 15, fibonacci(30, 30)),
           ("fibonacci_286_limit_15", 286, 15, fibonacci(286, 40)), ("fibonacci_286_of_a_member", 286, 15, fibonacci(286, 18)),
           ("fibonacci_19_reversed", 19, 7, fibonacci(19, 19)[::-1])]
    for n, limit in ((19, 7), (30, 15), (286, 15)):
        one, two = [0] * n, [0] * n
        one[n // 2] = 5
        two[0], two[n - 1] = 7, 1
        out += [(f"one_symbol_{n}", n, limit, one), (f"two_symbols_{n}", n, limit, two), (f"all_equal_{n}", n, limit, [3] * n),
                (f"all_but_one_equal_{n}", n, limit, [1] * (n - 1) + [1000])]
        for k in range(12):
            f = rng.integers(0, int(rng.choice([2, 4, 50, 3000])), n)
            f = f * (rng.random(n) < rng.choice([0.2, 0.6, 1.0]))
            if k % 3 == 0:                                                # a few heavy symbols over many rare ones: deep trees
                f = np.where(rng.random(n) < 0.3, f * int(rng.integers(100, 100000)), f)
            if not f.any():
                f[0] = 1
            out.append((f"random_{n}_{k}", n, limit, [int(v) for v in f]))
    assert all(sum(f) < 1 << 32 and len(f) == n for _, n, _, f in out)
    return out


def test_codes_of_histograms_no_member_has(tmp_path):
    ck.make(ck.TOOL)
    hs = histograms()
    src, out = str(tmp_path / "histograms.txt"), str(tmp_path / "codes.txt")
    with open(src, "w") as f:
        f.write("".join(f"{n} {limit} {' '.join(map(str, freqs))}\n" for _, n, limit, freqs in hs))
    ck.run_tool(ck.TOOL, ["codes", src, out], timeout=120)
    ck.make(ck.TOOL_ASAN)                                                 # the limiter's shifts and indices under the sanitizers: same output
    ck.run_tool(ck.TOOL_ASAN, ["codes", src, out + ".asan"], timeout=120)
    assert open(out + ".asan").read() == open(out).read()
    lines = [[int(v) for v in ln.split()] for ln in open(out).read().splitlines()]
    assert len(lines) == 2 * len(hs)
    faults, limited = [], 0
    for (name, n, limit, freqs), lengths, codes in zip(hs, lines[0::2], lines[1::2]):
        assert len(lengths) == n and len(codes) == n, name
        faults += [(name, x) for x in ck.code_faults("code", freqs, lengths, limit, lone_ok=True)]
        want = [c[0] if c else 0 for c in ds.canonical(lengths)]          # RFC 1951 3.2.2, bits reversed for an LSB-first bit string
        if codes != want:
            faults.append((name, "the codes are not the canonical ones, bit-reversed"))
        limited += dm.huffman_cost(freqs)[1] > limit
    assert not faults, faults[:20]
    assert limited >= 6                                                   # the limiter really ran: Fibonacci and the heavy random ones
    by = {name: lengths for (name, *_), lengths in zip(hs, lines[0::2])}
    assert max(by["fibonacci_19_limit_7"]) == 7 and max(by["fibonacci_30_limit_15"]) == 15 and max(by["fibonacci_286_limit_15"]) == 15


def test_the_tools_usage(tmp_path):
    ck.make(ck.TOOL)
    p = subprocess.run([ck.TOOL, "batch", os.devnull, os.devnull], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and b"Usage" in p.stderr
