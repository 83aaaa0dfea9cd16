"""Per-hit details on the GPU (mp_search_annotate / mp_search_amplicons and what is built on
them) against the committed oracle and fixtures.

Expected values: a primer's mismatch count is the smallest n in 0..N for which
oracle.epcr_oracle.primer_match(segment, primer, strand, n, X, I) holds (defined for every hit:
a hit has at most N mismatches and none in the protected 3' bases); the expected amplicon is
sequence.upper()[pos1:pos2 + 1].
"""

import ctypes
import functools
import os
import random
import tempfile

import numpy as np
import pytest

from merpcr_amd import FASTARecord, MerPCR, _native, cli
from oracle import epcr_oracle as O
from tests.golden_io import case_inputs, data_path, load_golden

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ helpers
def _engine_for(case, td):
    """(engine with the case's STS loaded, its records) or (None, None) when the load fails."""
    eng = MerPCR(**case["params"])
    p = os.path.join(td, "x.sts")
    with open(p, "w") as fh:
        fh.write(case["sts_text"])
    if not eng.load_sts_file(p):
        return None, None
    if "fasta_text" in case:
        f = os.path.join(td, "x.fa")
        with open(f, "w", newline="") as fh:
            fh.write(case["fasta_text"])
        return eng, eng.load_fasta_file(f)
    return eng, [FASTARecord(defline=d, sequence=s) for d, s in case["records"]]


def _mm(seg, primer, strand, eng):
    for n in range(eng.mismatches + 1):
        if O.primer_match(seg, primer, strand, n, eng.three_prime_match, eng.iupac_mode):
            return n
    raise AssertionError(f"not a hit within N = {eng.mismatches}: {seg!r} vs {primer!r} ({strand})")


def _expect(eng, seqs, hits):
    """Per hit: (mm1, mm2, amplicon, primer-window text) from the oracle's compare and the
    upper-cased sequences."""
    ups = [s.upper() for s in seqs]
    recs = eng.sts_records
    out = []
    for p1, p2, sq, ri in zip(hits["pos1"].tolist(), hits["pos2"].tolist(), hits["seq"].tolist(),
                              hits["rec"].tolist()):
        S, r = ups[sq], recs[ri]
        w1, w2 = S[p1:p1 + len(r.primer1)], S[p2 + 1 - len(r.primer2):p2 + 1]
        out.append((_mm(w1, r.primer1, "+", eng), _mm(w2, r.primer2, "-", eng), S[p1:p2 + 1], w1 + w2))
    return out


def _check(eng, recs, seqs, d, counts=None):
    """d (HitDetails with amplicons) against the expectation; tallies the classes seen."""
    exp = _expect(eng, seqs, d.hits)
    assert d.mm1.tolist() == [e[0] for e in exp]
    assert d.mm2.tolist() == [e[1] for e in exp]
    assert d.size.tolist() == [len(e[2]) for e in exp]
    assert d.expected.tolist() == [eng.sts_records[ri].pcr_size for ri in d.hits["rec"].tolist()]
    for i, e in enumerate(exp):
        assert d.amplicon(i) == e[2], (i, d.hits[i])
    if counts is None:
        return
    for i, (m1, m2, amp, win) in enumerate(exp):
        h = d.hits[i]
        sq, p1, p2 = int(h["seq"]), int(h["pos1"]), int(h["pos2"])
        counts["hits"] += 1
        counts["mm1"] += m1 > 0
        counts["mm2"] += m2 > 0
        counts["non_acgt"] += bool(set(amp) - set("ACGT"))
        counts["u"] += "U" in amp
        counts["exc_in_primer"] += bool(set(win) - set("ACGT"))
        counts["non_ascii"] += not seqs[sq].isascii()
        counts["lower"] += seqs[sq].isascii() and seqs[sq][p1:p2 + 1] != amp
        counts["base0"] += p1 == 0
        counts["last_base"] += p2 == len(seqs[sq].upper()) - 1
        counts["later_seq"] += sq > 0


CLASSES = ("hits", "mm1", "mm2", "non_acgt", "u", "exc_in_primer", "non_ascii", "lower", "base0", "last_base",
           "later_seq")


# ------------------------------------------------------------------ a. golden corpus
def test_golden_corpus_details():
    """Every loadable case of both corpus files, default options: the detailed hits are find_hits'
    and every count and amplicon is the oracle's.  Every class the corpus is known to hold must
    have been seen (counted with the oracle: mm1 > 0 1,401 hits, mm2 > 0 2,313, non-ACGT
    amplicons 323 with 37 holding 'U', an exception base inside a primer window 211, non-ASCII
    records 571, lower case 243, base 0 81, a record's last base 201, a later sequence 233).
    The amplicons of a case are concatenated, so their varied sizes put them at every one of
    the 16 byte offsets inside an output line of the amplicon kernel (each occurs over 150
    times in the recorded outputs)."""
    counts = dict.fromkeys(CLASSES, 0)
    align = set()
    for name in ("random_cases.json.gz", "special_cases.json.gz"):
        for case in load_golden(name)["cases"]:
            with tempfile.TemporaryDirectory() as td:
                eng, recs = _engine_for(case, td)
            if eng is None:
                continue
            seqs = [s for _, s in case_inputs(case)[2]]
            plain = eng.find_hits(recs)
            d = eng.find_hits_detailed(recs, amplicons=True)
            assert np.array_equal(d.hits, plain), case["params"]
            _check(eng, recs, seqs, d, counts)
            align.update((d._amp[1][:-1] % 16).tolist())
    print(counts)
    assert all(counts[k] > 0 for k in CLASSES), counts
    assert align == set(range(16))


# ------------------------------------------------------------------ b. repeat: every misalignment, windows
@functools.lru_cache(maxsize=None)
def _repeat():
    case = load_golden("repeat.json.gz")
    with tempfile.TemporaryDirectory() as td:
        eng, recs = _engine_for(case, td)
    seqs = [s for _, s in case_inputs(case)[2]]
    d = eng.find_hits_detailed(recs, amplicons=True)
    return eng, recs, seqs, d


def test_repeat_offsets_and_text():
    eng, recs, seqs, d = _repeat()
    n = len(d)
    assert n == 15936
    assert int(d.size.max()) <= 68
    data, off = d._amp
    want = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(d.size, out=want[1:])
    assert np.array_equal(off, want)
    assert len(data) == int(off[-1])
    # the repeat's products are 8, 12, ... 68 bases: every 4-byte misalignment of the output
    # (the golden corpus test sees all 16)
    assert set((off[:-1] % 16).tolist()) == {0, 4, 8, 12}
    _check(eng, recs, seqs, d)


@pytest.mark.parametrize("window", [(0, 0), (1, 1), (7, 1000), "last", "last_after_full"])
def test_repeat_windows_equal_slices(window):
    eng, recs, seqs, d = _repeat()
    s = eng._dev_search
    n = len(d)
    data, off = d._amp
    mm = np.stack([d.mm1, d.mm2], axis=1)
    if window == "last_after_full":
        assert np.array_equal(s.annotate(0, n), mm)
        b, o = s.amplicons(0, n)
        assert np.array_equal(o, off) and np.array_equal(b, data)
    first, count = (n - 1, 1) if isinstance(window, str) else window
    assert np.array_equal(s.annotate(first, count), mm[first:first + count])
    b, o = s.amplicons(first, count)
    assert np.array_equal(o, off[first:first + count + 1] - off[first])
    assert np.array_equal(b, data[int(off[first]):int(off[first + count])])


# ------------------------------------------------------------------ c. long amplicons
LONG_PARAMS = dict(wordsize=11, margin=50, mismatches=2, iupac_mode=1)
LONG_LENGTHS = (70, 12345, 9001)  # none a multiple of 64


@functools.lru_cache(maxsize=None)
def _long_inputs():
    """Seeded input: products of ~9,000 bases with an 'N' run of 5,000 across two 4,096-base
    boundaries of the padded layout, IUPAC letters, 'U's and lower case inside them; one starts at
    base 0 with a 40-base primer, one ends on its record's last base and starts inside an 'N'
    run that begins before it; two short products carry mismatches and a 'U' in a primer window."""
    rng = random.Random(20240611)
    seqs = [[rng.choice("ACGT") for _ in range(n)] for n in LONG_LENGTHS]
    s1, s2 = seqs[1], seqs[2]
    sts = []
    # A: bases [0, 9000) of sequence 1, primer 1 of 40 bases
    sts.append(("A", "".join(s1[0:40]), "".join(s1[8976:9000]), 9000))
    for i in range(3500, 8500):
        s1[i] = "N"
    s1[100], s1[101], s1[500] = "R", "y", "K"
    s1[200] = s1[201] = s1[1000] = "U"
    for i in range(300, 400):
        s1[i] = s1[i].lower()
    # C: [9200, 9420) of sequence 1; a genome 'U' under primer 1's 'T', two mismatches in primer 2
    p1 = s1[9200:9222]
    p1[5], s1[9205] = "T", "U"
    p2 = s1[9398:9420]
    for j in (8, 12):
        p2[j] = "ACGT"["ACGT".index(p2[j]) ^ 1]
    sts.append(("C", "".join(p1), "".join(p2), 220))
    # D: [10000, 10300) of sequence 1, lower case throughout, one mismatch in primer 1, an IUPAC
    # letter of the genome inside primer 2's window
    for i in range(10000, 10300):
        s1[i] = s1[i].lower()
    p1 = [c.upper() for c in s1[10000:10025]]
    p1[15] = "ACGT"["ACGT".index(p1[15]) ^ 2]  # past the 11-base seed, before the protected 3' base
    p2 = [c.upper() for c in s1[10278:10300]]
    s1[10290] = "ACGT"["ACGT".index(p2[12]) ^ 1].lower()  # a genome mismatch ...
    s1[10284] = "n"                                        # ... and an 'N', which matches under I = 1
    sts.append(("D", "".join(p1), "".join(p2), 300))
    # B: bases [1, 9001) of sequence 2 -- its last base -- behind an 'N' run over bases [0, 2):
    # primer 1 starts with 'N' (the seed is taken one base in), the genome base under it is 'N'
    s2[0] = s2[1] = "N"
    sts.append(("B", "N" + "".join(s2[2:22]), "".join(s2[8979:9001]), 9000))
    s2[4000], s2[4001] = "U", "W"
    seqs = ["".join(s) for s in seqs]
    text = "".join(f"{i}\t{a}\t{b}\t{n}\talias {i}\n" for i, a, b, n in sts)
    # the oracle's hits, in output order
    prm = O.params(**LONG_PARAMS)
    table = O.load_sts_lines(text.splitlines(keepends=True), prm["wordsize"], prm["default_pcr_size"])
    want = []
    for q, s in enumerate(seqs):
        hs = O.scan_sequence(s, table, prm)
        hs.sort(key=lambda h: O.canonical_sort_key(h, table, len(s), prm))
        want += [(k, e, q, table.records[ri].sts_id, table.records[ri].direct) for k, e, ri in hs]
    return seqs, text, table, want


@functools.lru_cache(maxsize=None)
def _long_case():
    seqs, text, table, want = _long_inputs()
    eng = MerPCR(**LONG_PARAMS)
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "long.sts")
        with open(p, "w") as fh:
            fh.write(text)
        assert eng.load_sts_file(p)
    recs = [FASTARecord(defline=f">seq{i} synthetic", sequence=s) for i, s in enumerate(seqs)]
    d = eng.find_hits_detailed(recs, amplicons=True)
    return eng, recs, seqs, table, want, d


def test_long_amplicons():
    eng, recs, seqs, table, want, d = _long_case()
    got = [(int(h["pos1"]), int(h["pos2"]), int(h["seq"]), eng.sts_records[int(h["rec"])].id,
            eng.sts_records[int(h["rec"])].direct) for h in d.hits]
    assert got == want
    assert len(got) >= 4
    _check(eng, recs, seqs, d)
    by_id = {g[3]: i for i, g in enumerate(got)}
    assert set(by_id) == {"A", "B", "C", "D"}
    base = np.concatenate([[0], np.cumsum([(n + 63) // 64 * 64 for n in LONG_LENGTHS])])
    a, b, c, dd = (d.amplicon(by_id[k]) for k in "ABCD")
    ha, hb = d.hits[by_id["A"]], d.hits[by_id["B"]]
    # the planted classes
    run0, run1 = int(base[1]) + 3500, int(base[1]) + 8500  # the long 'N' run, global bases
    assert a[3500:8500] == "N" * 5000 and run1 // 4096 - run0 // 4096 == 2
    assert a[100:102] == "RY" and a[500] == "K" and a[200:202] == "UU" and a[1000] == "U"
    assert seqs[1][300:400].islower() and a[300:400] == seqs[1][300:400].upper()
    assert int(ha["pos1"]) == 0 and len(eng.sts_records[int(ha["rec"])].primer1) == 40 > 32
    assert int(hb["pos1"]) == 1 and seqs[2][0:2] == "NN" and b[0] == "N"   # the run begins before pos1
    assert int(hb["pos2"]) == LONG_LENGTHS[2] - 1                            # the record's last base
    assert b[3999:4001] == "UW" and len(a) == len(b) == 9000
    assert (int(d.mm1[by_id["B"]]), int(d.mm2[by_id["B"]])) == (0, 0)
    assert (int(d.mm1[by_id["C"]]), int(d.mm2[by_id["C"]])) == (0, 2) and c[5] == "U"
    assert (int(d.mm1[by_id["D"]]), int(d.mm2[by_id["D"]])) == (1, 1) and dd[284] == "N"
    # the whole list (mean amplicon 4,630 bytes) went a wave per amplicon; the two short
    # products alone (mean 260) go a quarter wave each, and give the same bytes
    assert sorted((by_id["C"], by_id["D"])) == [1, 2]
    data, off = d._amp
    b2, o2 = eng._dev_search.amplicons(1, 2)
    assert np.array_equal(o2, off[1:4] - off[1]) and np.array_equal(b2, data[int(off[1]):int(off[3])])


# ------------------------------------------------------------------ d. errors
def test_detail_errors():
    eng, recs, seqs, table, want, _ = _long_case()
    tb = eng.device_table()
    data = eng.encode_records(recs)
    lengths = [len(x) for x in data]
    g = _native.Genome(eng.device, lengths)
    s = _native.Search(tb, g)

    def fill():
        for i, x in enumerate(data):
            g.put(i, x)
        g.seal()

    def state(fn, *a):
        with pytest.raises(_native.NativeError) as e:
            fn(*a)
        assert e.value.code == _native.MP_E_STATE

    fill()
    state(s.annotate, 0, 0)       # no run yet
    state(s.amplicons, 0, 0)
    n = s.run()
    assert n == len(want)
    base_bytes = s.dev_bytes()
    mm = s.annotate()
    b, off = s.amplicons()
    assert s.dev_bytes() > base_bytes  # the scratch is counted once it exists
    assert s.annotate(n, 0).shape == (0, 2) and s.amplicons(0, 0)[1].tolist() == [0]
    for first, count in ((0, n + 1), (n, 1), (n + 1, 0), (2**64 - 1, 1)):
        with pytest.raises(ValueError):
            s.annotate(first, count)
        with pytest.raises(ValueError):
            s.amplicons(first, count)
    # MP_E_CAP: the need is reported, the offsets are filled, the buffer is untouched
    need = ctypes.c_uint64(0)
    buf = np.full(len(b), 0xA5, dtype=np.uint8)
    o2 = np.zeros(n + 1, dtype=np.uint64)
    rc = _native.lib().mp_search_amplicons(s._h, 0, n, _native.ptr(buf), len(b) - 1, _native.ptr(o2),
                                           ctypes.byref(need), None)
    assert rc == _native.MP_E_CAP and need.value == len(b)
    assert (buf == 0xA5).all() and np.array_equal(o2, off)
    # the genome refilled and sealed again: the planes no longer belong to the run
    g.reset(lengths)
    state(s.annotate, 0, 1)
    fill()
    state(s.annotate, 0, 1)
    state(s.amplicons, 0, 1)
    assert s.run() == n
    assert np.array_equal(s.annotate(), mm)
    b2, off2 = s.amplicons()
    assert np.array_equal(b2, b) and np.array_equal(off2, off)
    s.close()
    g.close()


# ------------------------------------------------------------------ e. output text
def test_search_details_text_and_amplicon_file(tmp_path):
    eng, recs, seqs, table, want, d = _long_case()
    out, amp = tmp_path / "hits.txt", tmp_path / "amp.fa"
    n = eng.search(recs, str(out), details=True, amplicon_file=str(amp))
    assert n == len(want)
    by_key = {(r.sts_id, r.direct): r for r in table.records}
    lines, fasta = [], []
    for k, e, q, sid, direct in want:
        r = by_key[(sid, direct)]
        S = seqs[q].upper()
        w1, w2 = S[k:k + len(r.primer1)], S[e + 1 - len(r.primer2):e + 1]
        head = f"seq{q}\t{k + 1}..{e + 1}\t{r.sts_id}\t{r.alias}\t({r.direct})"
        lines.append(f"{head}\t{_mm(w1, r.primer1, '+', eng)}\t{_mm(w2, r.primer2, '-', eng)}\t"
                     f"{e - k + 1}/{r.pcr_size}\n")
        fasta.append(f">seq{q}:{k + 1}..{e + 1}\t{r.sts_id}\t{r.alias}\t({r.direct})\n{S[k:e + 1]}\n")
    assert out.read_text() == "".join(lines)
    assert amp.read_text() == "".join(fasta)
    # the same call without the new arguments: the plain lines
    assert eng.search(recs, str(out)) == n
    assert out.read_text() == "".join(ln.rsplit("\t", 3)[0] + "\n" for ln in lines)


def test_cli_details_on_the_bundled_files(tmp_path):
    """The bundled pair's one hit: no mismatches, 201 bases against its STS size."""
    sts_size = None
    for ln in open(data_path("test.sts")):
        f = ln.rstrip("\n").split("\t")
        if f[0] == "AFM248yg9":
            sts_size = max(O.parse_pcr_size(f[3], 240), len(f[1]) + len(f[2]))
    out, amp = tmp_path / "o.txt", tmp_path / "a.fa"
    rc = cli.main([data_path("test.sts"), data_path("test.fa"), "--details", "--amplicons", str(amp), "-O", str(out)])
    assert rc == 0
    assert out.read_text() == ("L78833\t75823..76023\tAFM248yg9\t(D17S932)  Chr.17, 63.7 cM\t(-)"
                               f"\t0\t0\t201/{sts_size}\n")
    head, bases, rest = amp.read_text().split("\n")
    assert head == ">L78833:75823..76023\tAFM248yg9\t(D17S932)  Chr.17, 63.7 cM\t(-)"
    assert len(bases) == 201 and set(bases) <= set("ACGT") and rest == ""
    # without the options: today's bytes
    assert cli.main([data_path("test.sts"), data_path("test.fa"), "-O", str(out)]) == 0
    assert out.read_text() == "L78833\t75823..76023\tAFM248yg9\t(D17S932)  Chr.17, 63.7 cM\t(-)\n"


# ------------------------------------------------------------------ f. handle reuse
def test_run_after_details_is_unchanged():
    eng, recs, seqs, d = _repeat()
    s = eng._dev_search
    grown = s.regrowths()
    s.annotate()
    s.amplicons()
    n = s.run()
    assert n == len(d)
    assert np.array_equal(s.fetch(n), d.hits)
    assert s.regrowths() == grown
