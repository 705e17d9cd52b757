"""The ABI chain behind split_fastg (csrc/fastg_split.hip): palace_fasta_index -> palace_fastg_derive -> palace_fasta_names_create
-> palace_fastg_plan -> palace_fastg_write and the `.fai` rows, byte for byte against what the reference's script wrote
(tests/golden/split_fastg_cases.npz) and against the Python restatement of tests/split_fastg_cases.py."""
import os

import numpy as np
import pytest

from palace_amd import capi, synth
from tests import split_fastg_cases as sc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "split_fastg_cases.npz")


@pytest.fixture(scope="module")
def ctx():
    with capi.Ctx(0) as c:
        yield c


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def same(got: bytes, want: bytes):
    if got != want:
        at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError((len(got), len(want), at, got[max(0, at - 20):at + 20], want[max(0, at - 20):at + 20]))


def split_on_device(ctx, text, cuts=()):
    fs = capi.FastgSplit(ctx, text)
    try:
        assert fs.verdict == (0, 0), fs.verdict
        got, intact = fs.windows(list(cuts))
        assert intact, "bytes outside a window were written"
        return fs, got
    finally:
        fs.close()


@pytest.mark.parametrize("name", sorted(sc.golden_inputs()))
def test_golden_bytes(ctx, golden, name):
    text, want = golden[name + "__in"].tobytes(), golden[name + "__out"].tobytes()
    fs, got = split_on_device(ctx, text)
    assert fs.total == len(want)
    same(got, want)


def test_derived_names_and_duplicates(ctx, golden):
    text = golden["quirks__in"].tobytes() + golden["three_of_one_name__in"].tobytes() + b">';\nACGT\n>'x\nAC\n"
    fs = capi.FastgSplit(ctx, text)
    assert fs.verdict == (0, 0)
    recs, primed, dup, out_off = fs.derived()
    want, _ = sc.records(text)
    assert [text[int(r["name_off"]):int(r["name_off"] + r["name_len"])] for r in recs] == [w[0] for w in want]
    assert [bool(p) for p in primed] == [w[1] for w in want]
    kept = {i for i, _, _ in sc.kept_records(text)}
    assert [i for i in range(len(recs)) if not dup[i]] == sorted(kept) and fs.n_kept == len(kept)
    names = [w[0] for w in want]
    assert names.count(b"") == 3 and not dup[names.index(b"")]                # the empty name: its first record is kept, too
    assert int(out_off[-1]) == fs.total == len(sc.split_fastg(text))
    fs.close()


def test_tile_boundary_sweep(ctx):
    """a header, a record's end and the middle of a primed record on each of the text's offsets 4090 .. 4100"""
    for text in sc.tile_sweep_texts(synth.rng_for(41)):
        want = sc.split_fastg(text)
        _, got = split_on_device(ctx, text, cuts=range(1000, len(want), 1000))
        same(got, want)


def test_record_starts_on_every_residue(ctx):
    text = sc.residue_text(synth.rng_for(42))
    want = sc.split_fastg(text)
    starts, at = set(), 0
    for _, name, seq in sc.kept_records(text):
        starts.add(at % 16)
        at += len(name) + len(seq) + 3
    assert starts == set(range(16))
    fs, got = split_on_device(ctx, text)
    same(got, want)
    assert fs.n_kept == want.count(b">")


@pytest.mark.parametrize("window", [64, 1000, 4097])
def test_windows_reproduce_the_whole(ctx, golden, window):
    text, want = golden["spades60__in"].tobytes(), golden["spades60__out"].tobytes()
    _, got = split_on_device(ctx, text, cuts=range(window, len(want), window))
    same(got, want)


def test_many_records_in_one_tile_and_one_long_record(ctx):
    rng = synth.rng_for(43)
    text = b"".join(sc.fold(b"E_%d%s" % (i // 2, b"';" if i % 2 else b";"), sc.dna(rng, i % 5), 60) for i in range(1200))
    text += sc.fold(b"LONG';", sc.dna(rng, 150001), 60) + sc.fold(b"LONG:E_1;", b"AC", 60)
    want = sc.split_fastg(text)
    _, got = split_on_device(ctx, text, cuts=[5, 4096, 8191, 100000])
    same(got, want)


@pytest.mark.parametrize("name", sorted(sc.fault_cases()))
def test_faults(ctx, name):
    text, code, line = sc.fault_cases()[name]
    fs = capi.FastgSplit(ctx, text)
    assert fs.verdict == (code, line)
    assert fs.new_verdict == sc.new_verdict(text)
    fs.close()


def test_fault_lines_do_not_depend_on_tiles(ctx):
    """faults far into the text, in different tiles: the smaller line is reported, and each alone is found"""
    rng = synth.rng_for(44)
    body = b"".join(sc.fold(b"E_%d';" % i, sc.dna(rng, 500), 60) for i in range(40))          # 400 lines, five tiles
    lines = body.split(b"\n")
    for (a, b) in ((37, 311), (311, 37), (201, 202)):
        bad = list(lines)
        for k in (a, b):
            assert not bad[k].startswith(b">")
            bad[k] = bad[k][:7] + b"N" + bad[k][8:]
        text = b"\n".join(bad)
        fs = capi.FastgSplit(ctx, text)
        assert fs.verdict == (capi.FASTG_EBASE, min(a, b) + 1) == sc.verdict(text)
        fs.close()
    plus = list(lines)
    plus[351] = b"+" + plus[351][1:]
    plus[101] = plus[101][:3] + b"n" + plus[101][4:]
    fs = capi.FastgSplit(ctx, b"\n".join(plus))
    assert fs.verdict == (capi.FASTG_EBASE, 102) == sc.verdict(b"\n".join(plus))
    fs.close()


def test_fai_rows(ctx, golden):
    for name in ("spades60", "quirks", "empty_sequences", "crlf_small"):
        text = golden[name + "__in"].tobytes()
        if name == "quirks":
            text += text[:text.index(b"\n>") + 1]                                            # a whole header a second time
        fs = capi.FastgSplit(ctx, text)
        assert fs.verdict == (0, 0)
        same(fs.output_fai(), sc.output_fai(text))
        rows, left_out = fs.graph_fai()
        want, want_left = sc.graph_fai(text)
        same(rows, want)
        assert int(left_out.sum()) == len(want_left) == (1 if name == "quirks" else 0)
        fs.close()
