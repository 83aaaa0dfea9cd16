"""pair_kernel outside its staged shape, and primer_ok's chunk loop: primers of more than 32 and
more than 64 bases, margins from 64 to 10,000, against the C oracle byte for byte.

The C oracle is pinned to the reference's recorded output in these regimes by
tests/golden/wide.json.gz (tests/test_c_oracle.py).  The inputs come from the planted-case
generator that built that fixture (tests/golden/make_golden.py: wide_case), at 300 STS x
400 kbp, with genome ambiguity characters and lower case added here.  Every case asserts, on
the oracle's hits, that the classes it is there for occurred.
"""

import functools
import random
import tempfile

import numpy as np
import pytest

from merpcr_amd import FASTARecord, MerPCR
from oracle import c_oracle as C
from oracle import epcr_oracle as O
from tests.golden.make_golden import wide_case
from tests.test_gpu_details import _check
from tests.test_gpu_parity import _load_sts

pytestmark = pytest.mark.gpu

#        W   M      N  I  X   primer lengths
CASES = [(11, 64, 1, 0, 1, tuple(range(18, 26))),    # staging depends on alignment: both shapes
         (11, 100, 2, 1, 2, tuple(range(18, 33))),
         (11, 300, 2, 1, 2, (20, 31, 32, 33, 40, 64, 65, 97)),
         (12, 1500, 1, 0, 1, (18, 25, 33, 70)),        # the register window re-stages
         (8, 10000, 1, 0, 0, (20, 33, 65)),            # dense or split scan, maximal try rank
         (16, 2500, 2, 0, 40, (40, 65, 97))]           # hashed table, protection longer than a chunk
IDS = [f"W{c[0]}-M{c[1]}" for c in CASES]
SEEDS = {64: 1, 100: 2, 300: 3, 1500: 4, 10000: 5, 2500: 6}


@functools.lru_cache(maxsize=None)
def _case(i):
    """Inputs, the oracle's hits and the counts of the planted classes among them."""
    W, M, N, I, X, lengths = CASES[i]
    rng = random.Random(SEEDS[M])
    prm, sts_text, recs, plants = wide_case(rng, "p", W, M, N, X, I, list(lengths), 300, 3, 133_000, tandem=True,
                                            roomy=2 if M >= 1500 else 6, tandem_width=500, min_rec=100_000)
    nrng = np.random.default_rng(SEEDS[M])
    seqs = []
    for q, (_, s) in enumerate(recs):
        g = np.frombuffer(s.encode(), dtype=np.uint8).copy()
        free = np.ones(len(g), dtype=bool)        # not in a plant that must stay a non-hit or ends a record
        for kind, r, k, end, sid, direct, d, expect in plants:
            if r == q and (expect == 0 or kind == "end"):
                free[k:end + 1] = False
        for _ in range(3):                        # a few 'N' runs
            a = int(nrng.integers(0, len(g) - 100))
            run = np.arange(a, a + int(nrng.integers(5, 90)))
            g[run[free[run]]] = ord("N")
        for c in b"UR":                           # 0.2% each
            at = nrng.integers(0, len(g), len(g) // 500)
            g[at[free[at]]] = c
        for _ in range(len(g) // 4000):           # 5% lower case, in stretches of 200
            a = int(nrng.integers(0, len(g) - 200))
            g[a:a + 200] = np.frombuffer(g[a:a + 200].tobytes().lower(), dtype=np.uint8)
        seqs.append(g.tobytes().decode("ascii"))
    prm = {k: v for k, v in prm.items() if k != "default_pcr_size"}
    table = O.load_sts_lines(sts_text.splitlines(True), W, 240)
    ref = C.search(table, [s.upper().encode() for s in seqs], O.params(**prm), 8)
    lens = [len(s) for s in seqs]
    base = np.concatenate([[0], np.cumsum([(n + 63) // 64 * 64 for n in lens])])  # records padded to 64
    c = dict(hits=len(ref), l1_33=0, l2_33=0, l_65=0, d_plus_m=0, d_minus_m=0, last_base=0, staged=0,
             unstaged=0, tandem_max=0, near_absent=0, over_absent=0, prot_absent=0)
    per = {}
    for k, pos2, q, ri in zip(ref["pos1"].tolist(), ref["pos2"].tolist(), ref["seq"].tolist(), ref["rec"].tolist()):
        rec = table.records[ri]
        l1, l2, n = len(rec.primer1), len(rec.primer2), lens[q]
        c["l1_33"] += l1 > 32
        c["l2_33"] += l2 > 32
        c["l_65"] += max(l1, l2) > 64
        c["last_base"] += pos2 == n - 1
        if rec.pcr_size <= n - k:
            e, hi = rec.pcr_size, min(M, n - k - rec.pcr_size)
            c["d_plus_m"] += pos2 + 1 - k - e == M
            c["d_minus_m"] += pos2 + 1 - k - e == -M
        else:
            e, hi = n - k, 0
        lo = max(0, min(M, e - l1 - l2))
        # the stretch every try of this survivor reads, in the padded layout: staged when primer 2
        # fits one chunk and the stretch spans fewer than 6 32-base and fewer than 4 64-base words
        p0 = int(base[q]) + k + e - l2 - lo
        last = p0 + lo + hi + l2 - 1
        fits = l2 <= 32 and (last >> 5) - (p0 >> 5) + 1 < 6 and (last >> 6) - (p0 >> 6) + 1 < 4
        c["staged" if fits else "unstaged"] += 1
        if rec.sts_id == "ptan":
            per[(q, k, ri)] = per.get((q, k, ri), 0) + 1
    c["tandem_max"] = max(per.values(), default=0)
    found = set(zip(ref["seq"].tolist(), ref["pos1"].tolist(), ref["pos2"].tolist(),
                    [(table.records[ri].sts_id, table.records[ri].direct) for ri in ref["rec"].tolist()]))
    for kind, r, k, end, sid, direct, d, expect in plants:
        if expect == 0:
            assert (r, k, end, (sid, direct)) not in found, (kind, r, k, end, sid)
            c[kind[:4] + "_absent"] += 1
    return prm, sts_text, seqs, table, ref, c


def _engine(prm, sts_text, opts=None):
    eng = MerPCR(**prm)
    if opts:
        eng.search_options = opts
    with tempfile.TemporaryDirectory() as td:
        assert _load_sts(eng, sts_text, td)
    return eng


def _records(seqs):
    return [FASTARecord(defline=f">pr{i} wide", sequence=s) for i, s in enumerate(seqs)]


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_pair_wide_vs_c_oracle(i):
    """Matches, near misses, d = +-M and +-(M + 1) products, record-end products and a tandem
    STS (primer 2 = CA x 10 against (CA) runs: hundreds of tries of one survivor hit, and the
    try order 0, -1, +1, ... decides the output order)."""
    W, M, N, I, X, lengths = CASES[i]
    prm, sts_text, seqs, table, ref, c = _case(i)
    print(IDS[i], c)
    assert 200 < c["hits"] < 100_000, c
    assert c["d_plus_m"] > 0 and c["d_minus_m"] > 0 and c["last_base"] > 0, c
    assert c["near_absent"] >= 20 and c["over_absent"] >= 4, c
    if max(lengths) > 32:
        assert c["l1_33"] >= 20 and c["l2_33"] >= 20, c
    if X:
        assert c["prot_absent"] > 0, c
    # one survivor has 2M + 1 tries and CA x 10 can hit at every second one: more than 200 hits
    # of one (k, record) need M >= 200; below that, every second try of the whole margin
    assert c["tandem_max"] > (200 if M >= 200 else M // 2), c
    if M == 64:
        assert c["staged"] > 0 and c["unstaged"] > 0, c
    else:
        assert c["unstaged"] > 0, c
    hits = _engine(prm, sts_text).find_hits(_records(seqs))
    assert len(hits) == len(ref) and hits.tobytes() == ref.tobytes()
    if M == 10000:  # try ranks up to 20,000 through the other two hit orderings
        for opts in (dict(sort="radix128"), dict(sort_bucket_bits=1)):
            again = _engine(prm, sts_text, opts).find_hits(_records(seqs))
            assert again.tobytes() == ref.tobytes(), opts


def test_details_on_long_primers():
    """mm1, mm2, sizes and amplicon text of the 300-margin case (primers to 97 bases: the
    annotate kernel's chunk loop past its second chunk) against primer_match and the upper-cased
    text."""
    i = IDS.index("W11-M300")
    prm, sts_text, seqs, table, ref, c = _case(i)
    I = prm["iupac_mode"]
    long_primer, late_mm = 0, 0
    for k, pos2, q, ri in zip(ref["pos1"].tolist(), ref["pos2"].tolist(), ref["seq"].tolist(), ref["rec"].tolist()):
        rec = table.records[ri]
        l1, l2 = len(rec.primer1), len(rec.primer2)
        if max(l1, l2) <= 32:
            continue
        S = seqs[q].upper()
        long_primer += max(l1, l2) > 64
        late_mm += any(not O.primer_match(w[j], pr[j], "+", 0, 0, I)
                       for w, pr in ((S[k:k + l1], rec.primer1), (S[pos2 + 1 - l2:pos2 + 1], rec.primer2))
                       for j in range(32, len(pr)))
    print(dict(hits=len(ref), long_primer=long_primer, late_mm=late_mm))
    assert long_primer >= 20 and late_mm >= 20
    eng = _engine(prm, sts_text)
    recs = _records(seqs)
    d = eng.find_hits_detailed(recs, amplicons=True)
    assert d.hits.tobytes() == ref.tobytes()
    _check(eng, recs, seqs, d)
