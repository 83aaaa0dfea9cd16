"""Generate the golden fixtures under tests/golden/ by running the REFERENCE.

Run only in the build container, where the reference is importable:

    PYTHONPATH=/root/reference/src python3 tests/golden/make_golden.py
    PYTHONPATH=/root/reference/src python3 tests/golden/make_golden.py --chunked   # -T N corpus
    PYTHONPATH=/root/reference/src python3 tests/golden/make_golden.py --errors    # error paths
    ... make_golden.py --wide      # W >= 14, long primers, wide margins

Fixtures: bundled, repeat, random_cases, special_cases, threaded, unit_kats (.json.gz, the
plain run), chunked.json.gz (--chunked), errors.json.gz (--errors) and wide.json.gz (--wide:
65 planted cases at W 14/15/16 and 8/11, primers of W to 130 bases, margins 51 to 10,000, with
the list of what was planted where; its tally goes to stderr and tests/test_oracle_golden.py
asserts it).

The reference never ships with this repository and never runs on the GPU box;
what is committed is data only: the seeded inputs each case was built from and
the exact output the reference printed for them (plus unit-level known-answer
vectors for its helper functions).  The case generator below is this build's
own code.
"""

from __future__ import annotations

import gzip
import hashlib
import io
import json
import logging
import os
import random
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(HERE, "data")

IUPAC_EXTRA = "RYMKSWBDHVN"


def _ref():
    from merpcr import MerPCR  # noqa: F401  (reference, build container only)
    from merpcr.core.models import FASTARecord
    return MerPCR, FASTARecord


# --------------------------------------------------------------------------
# seeded case generator (this build's own code)
# --------------------------------------------------------------------------

def _rc(s):
    comp = {"A": "T", "C": "G", "G": "C", "T": "A", "U": "A", "B": "V", "V": "B",
            "D": "H", "H": "D", "K": "M", "M": "K", "R": "Y", "Y": "R",
            "N": "N", "S": "S", "W": "W", "X": "X"}
    return "".join(comp.get(c.upper(), "N") for c in reversed(s))


def _rand_seq(rng, n, mode):
    if n <= 0:
        return ""
    if mode == "acgt":
        return "".join(rng.choice("ACGT") for _ in range(n))
    if mode == "lowcomplex":
        alpha = rng.choice(["AT", "GC", "AC", "ACG", "A"])
        return "".join(rng.choice(alpha) for _ in range(n))
    if mode == "nruns":
        out = []
        while len(out) < n:
            if rng.random() < 0.08:
                out.extend("N" * rng.randint(1, 40))
            else:
                out.extend(rng.choice("ACGT") for _ in range(rng.randint(5, 120)))
        return "".join(out[:n])
    if mode == "iupac":
        return "".join(rng.choice("ACGT" * 6 + IUPAC_EXTRA + "X") for _ in range(n))
    if mode == "mixedcase":
        return "".join(rng.choice("ACGTacgt") for _ in range(n))
    if mode == "rna":
        return "".join(rng.choice("ACGU" + "ACGT" * 3) for _ in range(n))
    if mode == "junk":
        return "".join(rng.choice("ACGT" * 8 + "Nn*-.Z0x ") for _ in range(n))
    raise ValueError(mode)


def _mutate(rng, s, k, protect_tail=0, protect_head=0):
    s = list(s)
    L = len(s)
    for _ in range(k):
        lo = protect_head
        hi = L - 1 - protect_tail
        if hi < lo:
            break
        i = rng.randint(lo, hi)
        s[i] = rng.choice([c for c in "ACGT" if c != s[i].upper()] or ["A"])
    return "".join(s)


def _primer(rng, L, style):
    if style == "acgt":
        return "".join(rng.choice("ACGT") for _ in range(L))
    if style == "lower":
        return "".join(rng.choice("ACGTacgt") for _ in range(L))
    if style == "iupac":
        p = [rng.choice("ACGT") for _ in range(L)]
        for _ in range(rng.randint(1, max(1, L // 5))):
            p[rng.randrange(L)] = rng.choice(IUPAC_EXTRA)
        return "".join(p)
    if style == "rna":
        return "".join(rng.choice("ACGU") for _ in range(L))
    if style == "weird":
        p = [rng.choice("ACGT") for _ in range(L)]
        for _ in range(rng.randint(1, 3)):
            p[rng.randrange(L)] = rng.choice("XZ-*nr")
        return "".join(p)
    raise ValueError(style)


def _size_field(rng, size):
    r = rng.random()
    if r < 0.65:
        return str(size)
    if r < 0.8:
        a = max(1, size - rng.randint(0, 30))
        return f"{a}-{2 * size - a}"
    return rng.choice(["-5", "0", "abc", "10-", "-", "1-2-3", "x-y", " 7", "150", "3"])


def gen_case(rng, idx):
    W = rng.choice([3, 4, 5, 6, 7, 8, 8, 9, 10, 11, 11, 11, 12, 13, 14, 16])
    M = rng.choice([0, 1, 3, 10, 50, 50])
    N = rng.choice([0, 0, 1, 1, 2, 3])
    X = rng.choice([0, 1, 1, 2, 4, 40])
    I = rng.choice([0, 0, 1])
    Z = rng.choice([240, 240, 100, 60])
    mode = rng.choice(["acgt", "acgt", "acgt", "nruns", "iupac", "mixedcase",
                       "lowcomplex", "rna", "junk"])
    n_sts = rng.randint(1, 10)
    sts_lines = []
    planted = []
    for s in range(n_sts):
        L1 = rng.randint(W, max(W, 26))
        L2 = rng.randint(W, max(W, 26))
        style = rng.choice(["acgt"] * 6 + ["lower", "iupac", "rna", "weird"])
        p1 = _primer(rng, L1, style)
        p2 = _primer(rng, L2, rng.choice(["acgt", "acgt", style]))
        size = rng.randint(max(1, L1 + L2 - 10), L1 + L2 + 250)
        field = _size_field(rng, size)
        alias = rng.choice(["", "alias%d" % s, "(D17S%d)  Chr.1, 2.0 cM" % s])
        cols = [f"STS{idx}_{s}", p1, p2, field]
        if alias or rng.random() < 0.3:
            cols.append(alias)
        if rng.random() < 0.05:
            cols.append("extra")
        sts_lines.append("\t".join(cols))
        if rng.random() < 0.08:
            sts_lines.append(sts_lines[-1])  # duplicate line -> duplicate hits
        planted.append((p1, p2, size))
    if rng.random() < 0.2:
        sts_lines.insert(rng.randrange(len(sts_lines) + 1), "# comment line")
    if rng.random() < 0.15:
        sts_lines.insert(rng.randrange(len(sts_lines) + 1), "")
    if rng.random() < 0.02:
        sts_lines.append("BAD\tONLY\tTHREE")

    if rng.random() < 0.08:
        # dense case: tiny word, low-complexity genome and primers -> many hits per seed
        W = rng.choice([3, 4, 5])
        alpha = rng.choice(["AT", "ACG", "GC"])
        sts_lines = []
        for s in range(rng.randint(1, 4)):
            p1 = "".join(rng.choice(alpha) for _ in range(rng.randint(W, 8)))
            p2 = "".join(rng.choice(alpha) for _ in range(rng.randint(W, 8)))
            sts_lines.append(f"D{idx}_{s}\t{p1}\t{p2}\t{rng.randint(10, 60)}\tdense")
        seq = "".join(rng.choice(alpha) for _ in range(rng.randint(100, 700)))
        params = dict(wordsize=W, margin=rng.choice([0, 3, 10]), mismatches=N,
                      three_prime_match=X, iupac_mode=I, default_pcr_size=Z)
        return params, "\n".join(sts_lines) + "\n", [(f">dense{idx}", seq)]

    n_rec = rng.choice([1, 1, 1, 2, 3])
    records = []
    for r in range(n_rec):
        n = rng.choice([0, W - 1, W, W + 1, rng.randint(50, 600), rng.randint(600, 4000)])
        if mode in ("lowcomplex",) or (I and mode in ("iupac", "nruns")):
            n = min(n, 800)
        seq = list(_rand_seq(rng, n, mode))
        # plant amplicons in the orientations merpcr finds
        for p1, p2, size in planted:
            if rng.random() < 0.8 and n > 0:
                prod = max(len(p1) + len(p2), size + rng.randint(-M - 2, M + 2))
                fill = max(0, prod - len(p1) - len(p2))
                form = rng.choice(["plus", "minus", "minus"])
                if form == "plus":
                    a, b = p1, p2
                else:
                    a, b = p2, _rc(p1)
                if N and rng.random() < 0.6:
                    a = _mutate(rng, a, rng.randint(1, N), protect_tail=min(X, len(a)))
                amp = a + _rand_seq(rng, fill, "acgt") + b
                if rng.random() < 0.3:
                    amp = amp.lower()
                start = rng.randint(0, max(0, n - 1))
                if rng.random() < 0.15:
                    start = max(0, n - len(amp) + rng.randint(-5, 5))
                seq[start:start + len(amp)] = list(amp)
        records.append((f">rec{idx}_{r} desc {r}", "".join(seq)))
    params = dict(wordsize=W, margin=M, mismatches=N, three_prime_match=X,
                  iupac_mode=I, default_pcr_size=Z)
    return params, "\n".join(sts_lines) + "\n", records


def gen_fasta_text(rng, records):
    out = []
    if rng.random() < 0.2:
        out.append("ACGTACGT orphan line before header")
    nl = rng.choice(["\n", "\r\n", "\n", "\r"])
    for head, seq in records:
        out.append(head + rng.choice(["", "  ", "\t"]))
        w = rng.choice([60, 70, 13, 1000])
        for i in range(0, len(seq), w):
            chunk = seq[i:i + w]
            if rng.random() < 0.1:
                chunk = chunk + rng.choice([" 123", "*", "  ", "-", "U", "ſ", "\t9"])
            if rng.random() < 0.05:
                out.append("")
            out.append(rng.choice(["", " "]) + chunk)
    return nl.join(out) + nl


# --------------------------------------------------------------------------
# running the reference
# --------------------------------------------------------------------------

def run_ref(params, sts_text, records=None, fasta_text=None, threads=1):
    MerPCR, FASTARecord = _ref()
    eng = MerPCR(threads=threads, **params)
    with tempfile.TemporaryDirectory() as td:
        sp = os.path.join(td, "x.sts")
        with open(sp, "w") as fh:
            fh.write(sts_text)
        ok = eng.load_sts_file(sp)
        if not ok:
            return {"load_ok": False}
        if fasta_text is not None:
            fp = os.path.join(td, "x.fa")
            with open(fp, "w", newline="") as fh:
                fh.write(fasta_text)
            recs = eng.load_fasta_file(fp)
            loaded = [[r.defline, r.sequence, r.label] for r in recs]
        else:
            recs = [FASTARecord(defline=d, sequence=s) for d, s in records]
            loaded = None
        op = os.path.join(td, "out.txt")
        n = eng.search(recs, op)
        with open(op) as fh:
            out = fh.read()
    res = {"load_ok": True, "n_hits": n, "output": out,
           "max_pcr_size": eng.max_pcr_size,
           "n_records": len(eng.sts_records)}
    if loaded is not None:
        res["fasta"] = loaded
    return res


class _Capture(logging.Handler):
    def __init__(self):
        super().__init__(logging.DEBUG)
        self.msgs = []

    def emit(self, record):
        self.msgs.append([record.levelname, record.getMessage()])


def run_ref_err(params, sts_text, records, threads=1):
    """run_ref for the error paths: the exception type the reference raises from
    load_sts_file or search (if any), the output it wrote before it, and its log lines
    (minus timings)."""
    MerPCR, FASTARecord = _ref()
    cap = _Capture()
    lg = logging.getLogger("merpcr")
    lg.addHandler(cap)
    lg.setLevel(logging.DEBUG)
    res = {}
    try:
        eng = MerPCR(threads=threads, **params)
        with tempfile.TemporaryDirectory() as td:
            sp = os.path.join(td, "x.sts")
            with open(sp, "w") as fh:
                fh.write(sts_text)
            try:
                res["load_ok"] = eng.load_sts_file(sp)
                res["load_error"] = None
            except Exception as e:  # noqa: BLE001 - record the reference's exception type
                res["load_ok"] = None
                res["load_error"] = type(e).__name__
            res["n_records"] = len(eng.sts_records)
            res["keys"] = sorted(eng.sts_table)
            if res["load_ok"]:
                recs = [FASTARecord(defline=d, sequence=s) for d, s in records]
                op = os.path.join(td, "out.txt")
                try:
                    res["n_hits"] = eng.search(recs, op)
                    res["search_error"] = None
                except Exception as e:  # noqa: BLE001
                    res["search_error"] = type(e).__name__
                import gc
                gc.collect()  # the reference leaves its output file to be closed by the collector
                with open(op) as fh:
                    res["output"] = fh.read()
    finally:
        lg.removeHandler(cap)
    res["log"] = [m for m in cap.msgs if " seconds" not in m[1] and not m[1].startswith("Reading STS file")]
    return res


def error_cases(rng):
    """Characters beyond U+00FF (after upper()) in primers and sequences: the reference's
    scode[ord(c)] lookups raise IndexError when the hash or the scan reaches them
    (engine.py:345, 472, 497); characters that upper-case into Latin-1 do not."""
    MerPCR, _ = _ref()
    odd = ["\u03a9", "\u00ff", "\u0131", "\u00df", "\u00e9", "\u017f", "\u4e2d", "\u00b5", "N", "n", "U"]
    kats = []
    for _ in range(400):
        W = rng.randint(3, 12)
        L = rng.randint(0, 24)
        p = "".join(rng.choice(odd) if rng.random() < 0.12 else rng.choice("ACGTacgt") for _ in range(L))
        try:
            r = list(MerPCR(wordsize=W)._hash_value(p))
        except IndexError:
            r = "IndexError"
        kats.append([p, W, r])
    cases = []
    base = "".join(rng.choice("ACGT") for _ in range(3000))
    for i in range(60):
        W = rng.choice([4, 6, 8, 11])
        prm = dict(wordsize=W, margin=rng.choice([0, 5, 50]), mismatches=rng.randint(0, 2), three_prime_match=1,
                   iupac_mode=rng.randint(0, 1), default_pcr_size=240)
        lines = []
        for s in range(rng.randint(1, 4)):
            a = rng.randrange(0, 2500)
            p1 = base[a:a + rng.randint(W, 22)]
            q = a + rng.randint(100, 300)
            p2 = _rc(base[q - rng.randint(W, 22):q])
            if i % 3 == 0 and rng.random() < 0.6:  # an odd character in a primer
                which = rng.choice([0, 1])
                pr = list(p1 if which == 0 else p2)
                pr[rng.randrange(len(pr))] = rng.choice(odd[:8])
                if which == 0:
                    p1 = "".join(pr)
                else:
                    p2 = "".join(pr)
            lines.append(f"S{s}\t{p1}\t{p2}\t{q - a}\tal{s}")
        recs = []
        for r in range(rng.randint(1, 3)):
            s = list(base[rng.randrange(0, 500):][:rng.randint(0, 2500)])
            if i % 3 == 1 and s and rng.random() < 0.5:  # an odd character in a sequence
                s[rng.randrange(len(s))] = rng.choice(odd[:8])
            if i % 3 == 2 and rng.random() < 0.3:  # a short sequence (<= W) with one
                s = [rng.choice(odd[:8])] + list(base[:rng.randint(0, W - 1)])
            recs.append([f">r{r} d", "".join(s)])
        sts = "\n".join(lines) + "\n"
        cases.append({"params": prm, "sts_text": sts, "records": recs, **run_ref_err(prm, sts, recs)})
    return {"hash": kats, "cases": cases}


def unit_kats(rng):
    MerPCR, _ = _ref()
    kat = {"hash": [], "revcomp": [], "compare": [], "pcr_size": []}
    for _ in range(400):
        W = rng.randint(3, 16)
        L = rng.randint(0, 30)
        p = "".join(rng.choice("ACGTUacgtuNRYX-") if rng.random() < 0.15 else rng.choice("ACGT")
                    for _ in range(L))
        kat["hash"].append([p, W, list(MerPCR(wordsize=W)._hash_value(p))])
    eng = MerPCR()
    for _ in range(200):
        s = "".join(rng.choice("ACGTUBDHKMNRSVWXYacgtubdhkmnrsvwxyZ-*1") for _ in range(rng.randint(0, 20)))
        kat["revcomp"].append([s, eng._reverse_complement(s)])
    alpha = "ACGTUacgtuRYMKSWBDHVNXZ-"
    for _ in range(1500):
        L = rng.randint(1, 12)
        a = "".join(rng.choice(alpha) if rng.random() < 0.3 else rng.choice("ACGT") for _ in range(L))
        b = list(a) if rng.random() < 0.7 else [rng.choice("ACGT") for _ in range(L)]
        for _ in range(rng.randint(0, 3)):
            b[rng.randrange(L)] = rng.choice(alpha)
        b = "".join(b)
        if rng.random() < 0.03:
            b = b + "A"
        N = rng.randint(0, 3)
        X = rng.randint(0, 5)
        I = rng.randint(0, 1)
        strand = rng.choice("+-")
        e = MerPCR(mismatches=N, three_prime_match=X, iupac_mode=I)
        kat["compare"].append([a, b, strand, N, X, I, e._compare_seqs(a, b, strand)])
    for f in ["100", "150-250", "0", "-5", "abc", "10-", "-", "1-2-3", "x-y", " 7", "7 ", "3",
              "+9", "1_000", "٣", "100-200", "201-200", "5-5"]:
        kat["pcr_size"].append([f, MerPCR(default_pcr_size=240)._parse_pcr_size(f)])
    return kat


def _plan(n, threads, max_pcr, margin):
    """Chunk plan of the reference's -T N search (same rule as oracle.chunk_plan); used
    only to place amplicons on chunk seams."""
    t = threads if n >= 100000 else 1
    ov = max_pcr + margin - 1
    while t > 1 and (t + 1) * ov > n:
        t -= 1
    size = int((n - (t + 1) * ov) / t) + 2 * ov
    out, off = [], 0
    for i in range(t):
        ln = size if i < t - 1 else n - off
        out.append((off, ln))
        off += ln - ov
    return out


def chunked_cases():
    """-T N corpus: the reference's chunked search (duplicated overlap hits, chunk-local
    record ends) on genomes built so that hits fall on chunk seams."""
    g = random.Random(777)
    out = []

    def acgt(n):
        return "".join(g.choice("ACGT") for _ in range(n))

    def plant(seq, pos, amp):
        return seq[:pos] + amp + seq[pos + len(amp):]

    # 1. planted amplicons on the seams of every T's plan, two orientations
    p1, p2 = "GATTACAGGCTTACCGTA", "CCTAGGATCGATTGCAAT"
    prm = dict(wordsize=11, margin=50, mismatches=1, three_prime_match=1, iupac_mode=0,
               default_pcr_size=240)
    st = f"SEAM\t{p1}\t{p2}\t180\tseam marker\nSEAM2\t{p2}\t{p1}\t200-240\n"
    big = acgt(400000)
    ampf = p1 + acgt(180 - len(p1) - len(p2)) + p2
    ampr = p2 + acgt(190 - len(p1) - len(p2)) + _rc(p1)
    for T in (2, 3, 4, 8):
        for off, ln in _plan(len(big), T, 220, 50)[1:]:    # max_pcr_size = (200+240)//2
            big = plant(big, off + 10, ampf)            # inside the overlap: found twice
            big = plant(big, off + 269 - 60, ampr)      # straddles the previous chunk's end
    small = plant(acgt(60000), 30000, ampf)
    cases = [("seam", prm, st, [(">big seam test", big), (">small", small)], (1, 2, 3, 4, 8))]

    # 2. dense chance hits (W=4, 4-mer primers): many amplicons truncated by chunk ends
    prm2 = dict(wordsize=4, margin=20, mismatches=1, three_prime_match=1, iupac_mode=0,
                default_pcr_size=60)
    st2 = "".join(f"D{i}\t{acgt(g.randint(4, 6))}\t{acgt(g.randint(4, 6))}\t{g.randint(20, 90)}\n"
                  for i in range(4))
    cases.append(("dense", prm2, st2, [(">dense1", acgt(210000)), (">dense2", acgt(100000))], (1, 3, 5)))

    # 3. T reduced by a long product (ov ~ 20k), records at the 100 kbp threshold
    prm3 = dict(wordsize=8, margin=49, mismatches=0, three_prime_match=2, iupac_mode=1,
                default_pcr_size=240)
    q1, q2 = "ACGTTGCAAGGCTA", "TTGACGGCATCAGA"
    st3 = f"LONG\t{q1}\t{q2}\t20000\nSHORT\t{q2}\t{q1}\t150\nIUP\tACGTRYNNACGTAC\tGGCATTYCAGGA\t120\n"
    recs3 = []
    for n in (99999, 100000, 100001, 130000, 250000):
        sq = acgt(n)
        for pos in range(500, n - 300, 21011):
            sq = plant(sq, pos, q2 + acgt(150 - 2 * len(q1)) + q1)         # SHORT '+'
        for pos in range(1700, n - 20100, 17003):
            sq = plant(sq, pos, q1)                                         # LONG '+'
            sq = plant(sq, pos + 20000 - len(q2) + g.randint(-49, 49), q2)
        recs3.append((f">r{n} len={n}", sq))
    cases.append(("reduce", prm3, st3, recs3, (1, 4, 8)))

    for name, prm_, st_, recs, ts in cases:
        outs = {}
        for T in ts:
            r = run_ref(prm_, st_, records=recs, threads=T)
            outs[str(T)] = {"n_hits": r["n_hits"], "output": r["output"]}
            print("chunked", name, T, r["n_hits"], file=sys.stderr)
        out.append({"name": name, "params": prm_, "sts_text": st_, "records": [list(x) for x in recs],
                    "max_pcr_size": r["max_pcr_size"], "by_threads": outs})
    return out


# --------------------------------------------------------------------------
# --wide: hashed tables (W >= 14), long primers, wide margins
# --------------------------------------------------------------------------

WIDE_MARGINS = (51, 64, 100, 300, 1500, 3000, 10000)
_IUPAC_SETS = {"R": "AG", "Y": "CT", "M": "AC", "K": "GT", "S": "CG", "W": "AT", "N": "ACGT"}


def wide_lengths(W):
    return [W, W + 1, 31, 32, 33, 40, 63, 64, 65, 97, 130]


def wide_case(rng, tag, W, M, N, X, I, lengths, n_sts, n_rec, max_rec, tandem=False, gap=(20, 200),
              roomy=1, tandem_width=None, min_rec=0):
    """One planted case: (params, sts_text, records, plants).

    Every STS gets amplicons in both orientations ('+': p1 .. p2, '-': p2 .. revcomp(p1)) with
    a known product length size + d.  plants lists [kind, record, k, k + size + d - 1, id,
    direct, d, expect]: expect 1 means the output must hold exactly that line, 0 that it must
    not (near misses with N + 1 mismatches, a mismatch in a protected 3' base, products at
    d = +-(M + 1)), -1 that the reference decides (genome ambiguity characters, tandem runs).
    The first `roomy` STS have sizes of l1 + l2 + M or more, so that d = -M and -(M + 1) can be
    planted; their plants come first, and plants that no longer fit n_rec records of max_rec
    bases are left out.  tandem: one more STS whose primer 2 is CA x 10, with (CA) runs where
    its tries fall (every try at M <= 400, else tandem_width tries at either end)."""
    def acgt(n):
        return "".join(rng.choices("ACGT", k=n)) if n > 0 else ""

    def other(c, primer_c):
        return rng.choice([b for b in "ACGT" if b != c and b != primer_c])

    sts = []
    for s in range(n_sts):
        l1, l2 = rng.choice(lengths), rng.choice(lengths)
        p1, p2 = list(acgt(l1)), list(acgt(l2))
        for p in (p1, p2):                       # IUPAC letters past base 32
            if len(p) > 34 and rng.random() < (0.5 if I else 0.15):
                for _ in range(rng.randint(1, 2)):
                    p[rng.randrange(32, len(p))] = rng.choice("RYMKSWN")
        if rng.random() < 0.15 and l1 > W + 3:   # seed taken past a leading 'N' (hash_offset > 0)
            p1[:rng.randint(1, 3)] = "N" * 3
            p1 = p1[:l1]
        p1, p2 = "".join(p1), "".join(p2)
        r = rng.random()
        if s < roomy:
            room = M + rng.randint(0, 40)        # roomy: d = -M and -(M + 1) are plantable
        elif r < 0.3:
            room = rng.choice([0, 1, 5])         # lo clipped, primers overlap for d < -room
        else:
            room = rng.randint(20, 120)
        size = l1 + l2 + room
        field = str(size) if rng.random() < 0.85 or room else str(size - 3)
        sts.append(dict(id=f"{tag}s{s}", p1=p1, p2=p2, size=size, field=field, alias=f"w {s}"))
    if tandem:
        l1 = rng.choice(lengths)
        sts.append(dict(id=f"{tag}tan", p1=acgt(l1), p2="CA" * 10, size=l1 + 20 + M + rng.randint(10, 60),
                        field=None, alias="tandem"))
        sts[-1]["field"] = str(sts[-1]["size"])

    def concrete(p):
        out = []
        for c in p:
            if c in "ACGT" or not I or rng.random() < 0.3:
                out.append(c)                    # I = 0: the letter itself is what matches
            else:
                out.append(rng.choice(_IUPAC_SETS[c]))
        return out

    def seed_off(p):
        for off in range(len(p) - W + 1):
            if all(c in "ACGT" for c in p[off:off + W]):
                return off
        return -1

    def mutate(text, primer, positions):
        for i in positions:
            text[i] = other(text[i], primer[i])

    def pick(allowed, n, split):
        """n positions from allowed, preferring bases >= 32; split: both sides of base 32."""
        late = [i for i in allowed if i >= 32]
        early = [i for i in allowed if i < 32]
        if split and n >= 2 and late and early:
            got = [rng.choice(late), rng.choice(early)]
            rest = [i for i in allowed if i not in got]
            return got + rng.sample(rest, min(n - 2, len(rest)))
        pool = late if late and rng.random() < 0.8 else allowed
        if len(pool) < n:
            pool = allowed
        return rng.sample(pool, n) if len(pool) >= n else None

    plants = []  # (kind, id, direct, d, expect, text, at_end)
    for st in sts:
        if st["id"].endswith("tan"):
            continue
        kinds = ["match", "plusM", "minusLo", "near1", "near2", "over+", "deco", "match"]
        if N:
            kinds += ["mm", "mm", "mm"]
        if X:
            kinds += ["prot1", "prot2"]
        if st in sts[:roomy]:
            kinds += ["over-"]
            chosen = ["plusM", "minusLo", "over-", "over+"] + rng.sample(kinds, 2)
        else:
            chosen = rng.sample(kinds, min(len(kinds), rng.randint(3, 5)))
        if M >= 1500 and st not in sts[:roomy]:
            chosen = [k for k in chosen if k not in ("plusM", "over+")] or ["match"]
        for kind in chosen:
            direct = rng.choice("+-")
            a, b = (st["p1"], st["p2"]) if direct == "+" else (st["p2"], _rc(st["p1"]))
            la, lb = len(a), len(b)
            off = seed_off(a)
            if off < 0:
                continue
            e = st["size"]
            lo = max(0, min(M, e - la - lb))
            ta, tb = concrete(a), concrete(b)
            ok_a = [i for i in range(la) if a[i] in "ACGT" and not off <= i < off + W and i < la - X]
            ok_b = [i for i in range(lb) if b[i] in "ACGT" and i >= X]
            expect = 1
            d = rng.choice([0, rng.randint(-lo, M), rng.randint(-lo, min(M, 60))])
            if kind == "plusM":
                d = M
            elif kind == "minusLo":
                d = -lo
            elif kind == "over+":
                d, expect = M + 1, 0
            elif kind == "over-":
                if e - la - lb < M + 1:
                    continue
                d, expect = -(M + 1), 0
            elif kind == "mm":
                for t, p, ok in ((ta, a, ok_a), (tb, b, ok_b)):
                    if ok and rng.random() < 0.75:
                        pos = pick(ok, min(len(ok), rng.randint(1, N)), False)
                        mutate(t, p, pos)
            elif kind in ("near1", "near2"):
                t, p, ok = (ta, a, ok_a) if kind == "near1" else (tb, b, ok_b)
                pos = pick(ok, N + 1, True)
                if pos is None:
                    continue
                mutate(t, p, pos)
                expect = 0
            elif kind in ("prot1", "prot2"):
                if kind == "prot1":
                    ok = [i for i in range(max(0, la - X), la) if a[i] in "ACGT" and not off <= i < off + W]
                else:
                    ok = [i for i in range(min(X, lb)) if b[i] in "ACGT"]
                if not ok:
                    continue
                late = [i for i in ok if i >= 32]
                i = rng.choice(late or ok)
                mutate(ta if kind == "prot1" else tb, a if kind == "prot1" else b, [i])
                expect = 0
            elif kind == "deco":                 # genome ambiguity characters under the primers
                for t, ok in ((ta, ok_a), (tb, ok_b)):
                    if ok:
                        t[rng.choice(ok)] = rng.choice("NRU")
                expect = -1
            fill = list(acgt(e + d - la - lb))
            if fill and rng.random() < 0.3:      # ... and inside the tries' stretch
                fill[rng.randrange(len(fill))] = rng.choice("NRU")
            at_end = expect == 1 and kind == "match" and rng.random() < 0.5
            if at_end:                           # ends the record: hi = 0, or e truncated for d < 0
                d = rng.choice([0, -min(lo, 3), -min(lo, 7)])
                fill = list(acgt(e + d - la - lb))
            plants.append((kind, st["id"], direct, d, expect, "".join(ta) + "".join(fill) + "".join(tb), at_end, e))
    rng.shuffle(plants)
    first = {st["id"] for st in sts[:roomy]}
    plants.sort(key=lambda pl: pl[1] not in first)
    if tandem:
        st = sts[-1]
        a, e = st["p1"], st["size"]
        tw = tandem_width or (160 if M > 3000 else 300 if M > 1500 else 500)
        spans = [(-M, M)] if M <= 400 else [(-M, -M + tw), (M - tw, M)]
        text = a
        for d0, d1 in spans:
            start = e - 20 + d0                   # primer 2's window at try d0
            text += acgt(start - len(text)) + "CA" * ((d1 - d0 + 20) // 2)
        plants.insert(0, ("tandem", st["id"], "+", 0, -1, text, True, 0))

    records, meta = [], []
    cur, has_end, need = [], False, 0
    plain = [st for st in sts if not st["id"].endswith("tan")]

    def close():
        """End the record; unless a plant ends it, every plant keeps its whole size ahead of it
        (a record that ends sooner truncates the size and shifts the tries)."""
        nonlocal cur, has_end, need
        if cur:
            if not has_end:
                cur.append(acgt(max(rng.randint(*gap), need - sum(map(len, cur)))))
                st = rng.choice(plain)           # an exact product on the record's last bases: hi = 0
                direct = rng.choice("+-")
                a, b = (st["p1"], st["p2"]) if direct == "+" else (st["p2"], _rc(st["p1"]))
                if seed_off(a) >= 0:
                    text = "".join(concrete(a)) + acgt(st["size"] - len(a) - len(b)) + "".join(concrete(b))
                    k = sum(map(len, cur))
                    cur.append(text)
                    meta.append(["end", len(records), k, k + len(text) - 1, st["id"], direct, 0, 1])
            records.append("".join(cur))
        cur, has_end, need = [], False, 0

    for kind, sid, direct, d, expect, text, at_end, e in plants:
        n = sum(map(len, cur))
        if has_end or (cur and n + len(text) + gap[1] > max_rec):
            close()
        if len(records) >= n_rec:
            break
        cur.append(acgt(rng.randint(*gap) if cur or rng.random() < 0.8 else 0))
        k = sum(map(len, cur))
        cur.append(text.lower() if rng.random() < 0.1 else text)
        # a plant ends the record unless the record is still short of min_rec bases or an
        # earlier plant needs it longer
        has_end = at_end and need <= k + len(text) and k + len(text) >= min_rec
        if not has_end:
            need = max(need, k + e)
        meta.append([kind, len(records), k, k + len(text) - 1, sid, direct, d, expect])
    if len(records) < n_rec:
        close()
    params = dict(wordsize=W, margin=M, mismatches=N, three_prime_match=X, iupac_mode=I,
                  default_pcr_size=240)
    sts_text = "".join(f"{s['id']}\t{s['p1']}\t{s['p2']}\t{s['field']}\t{s['alias']}\n" for s in sts)
    recs = [(f">{tag}r{i} wide", s) for i, s in enumerate(records)]
    return params, sts_text, recs, meta


def wide_plan():
    """(W, M, N, X, I, tandem) of every --wide case: each W of the hashed table against the
    small margins, W 8/11 against every margin, one tandem case per margin."""
    g = random.Random(41)
    plan = []
    for W in (14, 15, 16):
        for j in range(12):
            M = (51, 64, 100, 300, 51, 64, 100, 300, 1500, 3000, 64, 100)[j]
            plan.append((W, M, j % 4, g.choice([0, 1, 2, 4, 40]), j % 2, False))
    for M in WIDE_MARGINS:
        for W in (8, 11):
            for j in range(2 if M <= 300 else 1):
                plan.append((W, M, g.randint(0, 3), g.choice([0, 1, 2, 4, 40]), g.randint(0, 1), False))
        plan.append((g.choice([8, 11, 14, 16]), M, g.randint(0, 1), g.choice([0, 1, 2]), 0, True))
    return plan


def wide_cases(seed=20261019):
    rng = random.Random(seed)
    cases = []
    for i, (W, M, N, X, I, tandem) in enumerate(wide_plan()):
        big = M >= 1500
        n_sts = rng.randint(2, 3) if big else rng.randint(2, 15)
        if tandem:
            n_sts = 2
        params, sts_text, recs, plants = wide_case(
            rng, f"w{i}", W, M, N, X, I, wide_lengths(W), n_sts, 3 if big else rng.randint(1, 3),
            40000 if big else rng.randint(2000, 9000), tandem=tandem)
        case = {"params": params, "sts_text": sts_text, "records": [list(r) for r in recs], "plants": plants}
        case.update(run_ref(params, sts_text, records=recs))
        cases.append(case)
    return cases


def wide_tally(cases):
    """What the wide corpus holds, counted with this repository's oracle from the recorded
    inputs and outputs (tests/test_oracle_golden.py asserts the floors)."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from oracle import c_oracle as C
    from oracle import epcr_oracle as O
    t = dict(cases=len(cases), hits=0, l1_33=0, l2_33=0, l1_65=0, l2_65=0, mm_ge32=0, mm_ge64=0, d_plus_m=0,
             d_minus_m=0, near_absent=0, over_absent=0, prot_absent=0, planted_found=0, last_base=0,
             truncated=0, hash_offset=0, tandem_max=0, by_w={}, by_m={})
    for case in cases:
        prm = case["params"]
        p = O.params(**prm)
        table = O.load_sts_lines(case["sts_text"].splitlines(True), prm["wordsize"], prm["default_pcr_size"])
        out = set(case["output"].splitlines())
        t["by_w"][prm["wordsize"]] = t["by_w"].get(prm["wordsize"], 0) + 1
        t["by_m"][prm["margin"]] = t["by_m"].get(prm["margin"], 0) + 1
        labels = [O.fasta_label(d) for d, _ in case["records"]]
        for kind, r, k, end, sid, direct, d, expect in case["plants"]:
            alias = next(x.alias for x in table.records if x.sts_id == sid)
            line = f"{labels[r]}\t{k + 1}..{end + 1}\t{sid}\t{alias}\t({direct})"
            if expect == 1:
                assert line in out, (prm, kind, line)
                t["planted_found"] += 1
                t["d_plus_m"] += d == prm["margin"]
                t["d_minus_m"] += d == -prm["margin"]
            elif expect == 0:
                assert line not in out, (prm, kind, line)
                t["near_absent"] += kind.startswith("near")
                t["over_absent"] += kind.startswith("over")
                t["prot_absent"] += kind.startswith("prot")
        found = C.search(table, [s.encode() for _, s in case["records"]], p, 1)
        assert len(found) == case["n_hits"], prm
        for q, (_, seq) in enumerate(case["records"]):
            S = seq.upper()
            per = {}
            mine = found[found["seq"] == q]
            for k, pos2, ri in zip(mine["pos1"].tolist(), mine["pos2"].tolist(), mine["rec"].tolist()):
                rec = table.records[ri]
                l1, l2 = len(rec.primer1), len(rec.primer2)
                t["hits"] += 1
                t["l1_33"] += l1 > 32
                t["l2_33"] += l2 > 32
                t["l1_65"] += l1 > 64
                t["l2_65"] += l2 > 64
                t["last_base"] += pos2 == len(S) - 1
                t["truncated"] += rec.pcr_size > len(S) - k
                t["hash_offset"] += rec.hash_offset > 0
                per[(k, ri)] = per.get((k, ri), 0) + 1
                late = 0
                for w, pr, strand in ((S[k:k + l1], rec.primer1, "+"), (S[pos2 + 1 - l2:pos2 + 1], rec.primer2, "-")):
                    bad = [i for i in range(32, len(pr))
                           if not O.primer_match(w[i], pr[i], strand, 0, 0, prm["iupac_mode"])]
                    late = max([late] + bad)
                t["mm_ge32"] += late >= 32
                t["mm_ge64"] += late >= 64
            t["tandem_max"] = max([t["tandem_max"]] + list(per.values()))
    return t


def main():
    if "--wide" in sys.argv:
        logging.disable(logging.CRITICAL)
        cases = wide_cases()
        print("wide:", json.dumps(wide_tally(cases)), file=sys.stderr)
        with gzip.open(os.path.join(HERE, "wide.json.gz"), "wt") as fh:
            json.dump({"cases": cases}, fh, separators=(",", ":"))
        return
    if "--errors" in sys.argv:
        erng = random.Random(2026)
        obj = error_cases(erng)
        print("errors: hash raises", sum(k[2] == "IndexError" for k in obj["hash"]),
              "load raises", sum(c["load_error"] is not None for c in obj["cases"]),
              "search raises", sum(bool(c.get("search_error")) for c in obj["cases"]), file=sys.stderr)
        with gzip.open(os.path.join(HERE, "errors.json.gz"), "wt") as fh:
            json.dump(obj, fh, separators=(",", ":"))
        return
    if "--chunked" in sys.argv:
        logging.disable(logging.CRITICAL)
        with gzip.open(os.path.join(HERE, "chunked.json.gz"), "wt") as fh:
            json.dump({"cases": chunked_cases()}, fh, separators=(",", ":"))
        return
    logging.disable(logging.CRITICAL)
    rng = random.Random(20261015)
    sts_path = os.path.join(DATA, "test.sts")
    fa_path = os.path.join(DATA, "test.fa")
    with open(sts_path) as fh:
        sts_text = fh.read()
    with open(fa_path) as fh:
        fa_text = fh.read()

    bundled = []
    variants = [{}, {"mismatches": 1}, {"mismatches": 2}, {"mismatches": 3, "three_prime_match": 0},
                {"iupac_mode": 1, "mismatches": 2}, {"wordsize": 8}, {"wordsize": 16},
                {"wordsize": 8, "mismatches": 3, "margin": 200}, {"margin": 0},
                {"wordsize": 3, "margin": 10}]
    for v in variants:
        params = dict(wordsize=11, margin=50, mismatches=0, three_prime_match=1,
                      iupac_mode=0, default_pcr_size=240)
        params.update(v)
        res = run_ref(params, sts_text, fasta_text=fa_text)
        res.pop("fasta", None)
        bundled.append({"params": params, **res})
        print("bundled", v, res["n_hits"], file=sys.stderr)

    repeat = {"params": dict(wordsize=4, margin=50, mismatches=0, three_prime_match=1,
                             iupac_mode=0, default_pcr_size=240),
              "sts_text": "REPEAT\tATCG\tCGAT\t20\n",
              "records": [[">repeat", "ATCGCGAT" * 1000]]}
    r = run_ref(repeat["params"], repeat["sts_text"], records=repeat["records"])
    repeat.update(r)
    repeat["sha256"] = hashlib.sha256(r["output"].encode()).hexdigest()
    print("repeat", r["n_hits"], repeat["sha256"][:16], file=sys.stderr)

    cases = []
    for i in range(700):
        params, sts, recs = gen_case(rng, i)
        use_fasta = rng.random() < 0.25
        if use_fasta:
            ft = gen_fasta_text(rng, recs)
            res = run_ref(params, sts, fasta_text=ft)
            case = {"params": params, "sts_text": sts, "fasta_text": ft, **res}
        else:
            res = run_ref(params, sts, records=recs)
            case = {"params": params, "sts_text": sts, "records": [list(x) for x in recs], **res}
        cases.append(case)
    tot = sum(c.get("n_hits", 0) for c in cases)
    print("random cases", len(cases), "hits", tot, file=sys.stderr)

    # IUPAC N-run explosion and record-end truncation, hand-built
    special = []
    p1, p2 = "ACGTTGCAAGCTTAGC", "GGATCCTTAGGCATCA"
    seq = "ACGT" * 10 + p1 + "N" * 300 + "ACGT" * 10
    for I in (0, 1):
        prm = dict(wordsize=11, margin=50, mismatches=0, three_prime_match=1, iupac_mode=I,
                   default_pcr_size=240)
        st = f"NRUN\t{p1}\t{p2}\t200\n"
        special.append({"params": prm, "sts_text": st, "records": [[">nrun", seq]],
                        **run_ref(prm, st, records=[(">nrun", seq)])})
    g = random.Random(7)
    body = "".join(g.choice("ACGT") for _ in range(300))
    tail = p2 + "".join(g.choice("ACGT") for _ in range(60)) + _rc(p1)
    for cut in range(0, 40, 3):
        s = body + tail[:len(tail) - cut] if cut else body + tail
        prm = dict(wordsize=8, margin=50, mismatches=1, three_prime_match=1, iupac_mode=0,
                   default_pcr_size=240)
        st = f"END\t{p1}\t{p2}\t150\n"
        special.append({"params": prm, "sts_text": st, "records": [[">end", s]],
                        **run_ref(prm, st, records=[(">end", s)])})

    # T>1 chunking artefacts (documentation of reference behaviour, not a parity target)
    threaded = []
    g = random.Random(11)
    big = "".join(g.choice("ACGT") for _ in range(400000))
    pp1, pp2 = "TTGACCGATAGCTAGGCA", "CATGCTAGGATCCAGTTA"
    amp = pp2 + "".join(g.choice("ACGT") for _ in range(164)) + _rc(pp1)
    big = list(big)
    for pos in (1000, 99950, 199880, 299830, 399700):
        big[pos:pos + len(amp)] = list(amp)
    big = "".join(big)
    prm = dict(wordsize=11, margin=50, mismatches=0, three_prime_match=1, iupac_mode=0,
               default_pcr_size=240)
    st = f"CHUNK\t{pp1}\t{pp2}\t200\n"
    for T in (1, 4):
        threaded.append({"params": prm, "threads": T, "sts_text": st,
                         "records": [[">big", big]],
                         **run_ref(prm, st, records=[(">big", big)], threads=T)})
        print("threaded", T, threaded[-1]["n_hits"], file=sys.stderr)

    kats = unit_kats(rng)

    def dump(name, obj):
        with gzip.open(os.path.join(HERE, name), "wt") as fh:
            json.dump(obj, fh, separators=(",", ":"))

    dump("bundled.json.gz", {"sts_sha256": hashlib.sha256(sts_text.encode()).hexdigest(),
                             "fa_sha256": hashlib.sha256(fa_text.encode()).hexdigest(),
                             "cases": bundled})
    dump("repeat.json.gz", repeat)
    dump("random_cases.json.gz", {"cases": cases})
    dump("special_cases.json.gz", {"cases": special})
    dump("threaded.json.gz", {"cases": threaded})
    dump("unit_kats.json.gz", kats)


if __name__ == "__main__":
    main()
