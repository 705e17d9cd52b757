"""palace_depth_parse (csrc/depth_parse.hip) at the ABI: `samtools depth` text in windows -> totals, first bad line and per-window
runs, against the Python restatement of tests/depth_cases.py."""
import numpy as np
import pytest

from palace_amd import capi, synth
from tests import depth_cases as dc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with capi.Ctx(0) as c:
        yield c


def joined(windows):
    """the windows' runs in text order, a window's first run merged with the one before it when the names are equal"""
    runs = []
    for w in windows:
        for k, (name, s, n) in enumerate(w):
            if k == 0 and runs and runs[-1][0] == name:
                runs[-1][1] += s
                runs[-1][2] += n
            else:
                runs.append([name, s, n])
    return runs


def check(ctx, text, cuts):
    bad, n, total, per, runs = dc.restate(text)
    cur, windows, intact, _ = capi.depth_parse_windows(ctx, text, cuts)
    assert intact and not cur["error"]
    assert int(cur["bad_line"]) == bad and int(cur["lines"]) == n, (cuts, int(cur["bad_line"]), bad)
    if bad:
        return
    assert int(cur["sum"]) == total and int(cur["tail_len"]) == 0
    for w in windows:                                   # runs are maximal within a window and none is empty
        assert all(a[0] != b[0] for a, b in zip(w, w[1:])) and all(r[2] > 0 for r in w)
    assert joined(windows) == runs, cuts
    merged = {}
    for name, s, k in joined(windows):
        e = merged.setdefault(name, [0, 0])
        e[0] += s
        e[1] += k
    assert list(merged.items()) == list(per.items())


def small_text():
    lines = [b"ctg_one\t%d\t%d" % (p, 3 + p) for p in range(1, 5)] + [b"b\t7\t0", b"b\t8\t2147483647"] + \
            [b"ctg_one\t%d\t1" % p for p in range(90, 93)] + [b"third contig\t%d\t%d" % (p, p) for p in range(5, 9)]
    return b"\n".join(lines) + b"\n"


def test_every_two_window_cut(ctx):
    text = small_text()
    assert 150 < len(text) < 260
    for t in (text, text[:-1]):
        for cut in range(len(t) + 1):
            check(ctx, t, [cut])


@pytest.mark.parametrize("step", [1, 7])
def test_tiny_windows(ctx, step):
    for t in (small_text(), small_text()[:-1]):
        check(ctx, t, list(range(step, len(t), step)))


@pytest.mark.parametrize("seed", [5, 6])
def test_random_texts(ctx, seed):
    rng = synth.rng_for(seed)
    names = [bytes(rng.integers(33, 127, size=int(rng.integers(1, 301)), dtype=np.uint8).tolist()) for _ in range(40)]
    parts, size = [], 0
    while size < 64 << 10:
        name = names[int(rng.integers(0, 40))]
        k = int(rng.integers(1, 2001)) if rng.integers(0, 4) == 0 else int(rng.integers(1, 6))
        p0 = int(rng.integers(1, 1 << 20))
        for j in range(k):
            parts.append(b"%s\t%d\t%d\n" % (name, p0 + j, int(rng.integers(0, 500))))
            size += len(parts[-1])
            if size >= 64 << 10:
                break
    text = b"".join(parts)
    for n_win in (1, 2, 17, 50):
        cuts = sorted(int(c) for c in rng.integers(0, len(text) + 1, size=n_win - 1))
        if n_win == 17:
            cuts = sorted(cuts + cuts[:4])              # empty windows
        check(ctx, text, cuts)
    check(ctx, text[:-1], sorted(int(c) for c in rng.integers(0, len(text), size=9)))


def test_one_long_run_has_64_bit_sums(ctx):
    text = b"".join(b"the_only_contig\t%d\t%d\n" % (p, dc.VMAX - (p % 3)) for p in range(1, 11001))
    assert len(text) > 290 << 10
    bad, n, total, per, runs = dc.restate(text)
    assert total > 1 << 40 and len(runs) == 1
    check(ctx, text, [])
    check(ctx, text, [100000, 100001, 200003])


def test_bad_lines(ctx):
    good = [b"c1\t%d\t%d" % (p, p + 1) for p in range(1, 400)]          # ~ 4 KiB: more than one wave, two tiles with the long cases
    for bad_line in dc.BAD:
        for at in (0, 200, len(good)):
            lines = good[:at] + [bad_line] + good[at:]
            text = b"\n".join(lines) + b"\n"
            assert dc.restate(text)[0] == at + 1
            check(ctx, text, [len(text) // 3, 2 * len(text) // 3])
    # two bad lines: the earlier one is reported, whichever window or wave they fall in
    for a, b in ((3, 5), (10, 390), (150, 151), (0, 398), (64, 300)):
        lines = list(good)
        lines[b] = b"c1\t1"
        lines[a] = b"c1\t1\t-2"
        text = b"\n".join(lines) + b"\n"
        for cuts in ([], [len(text) // 2], [len(text) // 3, 2 * len(text) // 3]):
            check(ctx, text, cuts)
    check(ctx, b"\n".join(good) + b"\nc1\t5", [1000])                    # a bad last line without LF
    check(ctx, b"x" * 9000, [3000, 6000])                                # a line too long for the tail, never ended
    check(ctx, b"x" * 9000 + b"\t1\t1\nc\t1\t1\n", [3000, 6000])


def test_capacities(ctx):
    text = small_text()
    _, _, _, per, runs = dc.restate(text)
    name_bytes = sum(len(r[0]) for r in runs)
    cur, windows, intact, _ = capi.depth_parse_windows(ctx, text, [], runs_cap=len(runs), names_cap=name_bytes)
    assert intact and not cur["error"] and joined(windows) == runs      # exactly enough
    for rc, nc in ((len(runs) - 1, name_bytes), (len(runs), name_bytes - 1)):
        cur, windows, intact, untouched = capi.depth_parse_windows(ctx, text, [], runs_cap=rc, names_cap=nc)
        assert cur["error"] and windows == [None] and intact and untouched
        assert int(cur["win_runs"]) == len(runs) and int(cur["win_name_bytes"]) == name_bytes      # what the window needs
        assert int(cur["lines"]) == 0 and int(cur["sum"]) == 0
    # ... and every later window writes nothing either
    cur, windows, intact, untouched = capi.depth_parse_windows(ctx, text, [40, 120], runs_cap=1, names_cap=name_bytes)
    assert cur["error"] and windows[-1] is None and intact


def test_empty_text(ctx):
    for cuts in ([], [0, 0]):
        cur, windows, intact, untouched = capi.depth_parse_windows(ctx, b"", cuts)
        assert not cur["error"] and int(cur["lines"]) == 0 and int(cur["bad_line"]) == 0 and int(cur["sum"]) == 0
        assert all(w == [] for w in windows) and intact and untouched
