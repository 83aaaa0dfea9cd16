"""The hashed seed table (W >= 14: hashed presence filter, open-addressed slots with linear
probing, scan_kernel<2, ...>) at size, against the C oracle byte for byte.

The C oracle is pinned to the reference's recorded output at these word sizes by
tests/golden/wide.json.gz (tests/test_c_oracle.py).  Every case asserts that the table it
built is the hashed one; nothing here depends on which tail mode a table takes by default.
"""

import functools
import tempfile

import numpy as np
import pytest

from merpcr_amd import FASTARecord, MerPCR, synth
from oracle import c_oracle as C
from oracle import epcr_oracle as O
from tests.test_gpu_parity import _load_sts

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _engine(sts_text, prm, opts=None):
    eng = MerPCR(**prm)
    if opts:
        eng.search_options = opts
    with tempfile.TemporaryDirectory() as td:
        assert _load_sts(eng, sts_text, td)
    assert "hashed" in eng.device_table().layout()
    return eng


def _hits(eng, g, name=">chrH"):
    return eng.find_hits([FASTARecord(defline=name, sequence=g.tobytes().decode("ascii"))])


# ------------------------------------------------------------------ a. tables at size
N_STS, GLEN = 20_000, 2_000_000
GROUPS3 = range(0, 2001, 3)              # ~10% of the records: keys shared by three
BIG = ((4000, 12), (4100, 12), (4200, 40), (4300, 40))


@functools.lru_cache(maxsize=None)
def _sized(W, N, I):
    """20,000 STS against 2 Mbp: (sts text, genome, oracle table, oracle hits, counts)."""
    sts = synth.make_sts(N_STS, seed=7 + W, W=W, iupac=0.1 if I else 0.0)
    rng = np.random.default_rng(W * 10 + N)
    for i in GROUPS3:
        for j in (1, 2):
            sts.p1[i + j] = sts.p1[i][:W] + sts.p1[i + j][W:]
    for first, n in BIG:
        for j in range(1, n):
            sts.p1[first + j] = sts.p1[first][:W] + sts.p1[first + j][W:]
    lead_n = rng.choice(np.arange(5000, N_STS), N_STS // 50, replace=False)
    for i in lead_n:                           # the seed starts after the 'N's (hash_offset 1..3)
        j = int(rng.integers(1, 4))
        sts.p1[i] = b"N" * j + sts.p1[i][j:]
    g = ACGT[rng.integers(0, 4, GLEN)].copy()
    for _ in range(20):
        a = int(rng.integers(0, GLEN - 3000))
        g[a:a + int(rng.integers(50, 3000))] = ord("N")
    amps, starts = synth.amplicons(sts, GLEN, 5, N, 50, W)
    step = max(2, -(-460 // (GLEN // len(amps))))  # every step-th slot: planted amplicons do not overlap
    for amp, st in list(zip(amps, starts))[::step]:
        if st + len(amp) <= GLEN:
            g[st:st + len(amp)] = np.frombuffer(amp, dtype=np.uint8)
    # exact '+' amplicons of the large groups and of some groups of three, 600 bases apart
    at = 1000
    for i in [f + j for f, n in BIG for j in range(n)] + list(range(0, 300)) + lead_n[:40].tolist():
        p1 = sts.p1[i]
        lead = len(p1) - len(p1.lstrip(b"N"))  # a genome 'N' under a primer 'N' matches at I = 0 too
        fill = ACGT[rng.integers(0, 4, int(sts.size[i]) - len(p1) - len(sts.p2[i]))].tobytes()
        amp = b"N" * lead + synth._concrete(rng, p1[lead:]) + fill + synth._concrete(rng, sts.p2[i])
        g[at:at + len(amp)] = np.frombuffer(amp, dtype=np.uint8)
        at += 600
    text = sts.text()
    table = O.load_sts_lines(text.splitlines(True), W, 240)
    prm = dict(wordsize=W, mismatches=N, iupac_mode=I, margin=50)
    ref = C.search(table, [g], O.params(**prm), 8)
    size = np.array([len(table.buckets[table.records[int(r)].key]) for r in ref["rec"]])
    offs = np.array([table.records[int(r)].hash_offset for r in ref["rec"]])
    counts = dict(hits=len(ref), keys=len(table.buckets), shared3=int((size >= 3).sum()),
                  shared12=int((size >= 12).sum()), shared40=int((size >= 40).sum()),
                  hash_offset=int((offs > 0).sum()))
    return text, g, table, ref, prm, counts


SIZED = [(14, 1, 0), (15, 2, 0), (16, 1, 1), (16, 0, 0)]


@pytest.mark.parametrize("tails", ["auto", "inline", "kernel"])
@pytest.mark.parametrize("W,N,I", SIZED)
def test_hashed_tables_vs_c_oracle(W, N, I, tails):
    """40k keys in 2^17 slots (probe chains, filter false positives that end on an empty slot),
    keys shared by 3, 12 and 40 records behind one slot through both tail paths, primers that
    start with 'N' (hash_offset > 0), IUPAC primers at I = 1, N runs."""
    text, g, table, ref, prm, counts = _sized(W, N, I)
    print(W, N, I, counts)
    assert counts["hits"] >= 100 and counts["shared3"] >= 50 and counts["shared12"] >= 10, counts
    assert counts["shared40"] >= 10 and counts["hash_offset"] >= 5, counts
    eng = _engine(text, prm, None if tails == "auto" else dict(tails=tails, dense=False))
    hits = _hits(eng, g)
    assert len(hits) == len(ref) and hits.tobytes() == ref.tobytes()


def test_hashed_forced_regrowth_is_identical():
    """W = 15 with the survivor, bucket-tail and hit lists created one entry long: every list
    overflows and is regrown; identical to the default capacities (and to the oracle)."""
    text, g, table, ref, prm, counts = _sized(15, 2, 0)
    base = _hits(_engine(text, prm), g)
    eng = _engine(text, prm, dict(hit_cap=1, surv_cap=1, tail_cap=1))
    hits = _hits(eng, g)
    assert hits.tobytes() == base.tobytes() == ref.tobytes()
    assert eng.last_search_stats["regrowths"] >= 1


# ------------------------------------------------------------------ b. the ends of the key space
def _ends_case(I):
    W, N = 16, 1
    rng = np.random.default_rng(160 + I)

    def rnd(n):
        return ACGT[rng.integers(0, 4, n)].tobytes().decode()

    lines, planted = [], []
    for i in range(40):
        kind = i % 4
        p1, p2 = rnd(int(rng.integers(20, 31))), rnd(int(rng.integers(20, 31)))
        if kind == 0:
            p1 = "A" * 16 + p1[16:]
        elif kind == 1:
            p1 = "T" * 16 + p1[16:]
        elif kind == 2:
            p2 = "A" * 16 + p2[16:]          # the '-' record's key
        else:
            p2 = "T" * 16 + p2[16:]
        size = len(p1) + len(p2) + int(rng.integers(0, 200))
        lines.append(f"E{i}\t{p1}\t{p2}\t{size}\tend {i}\n")
        planted.append((p1, p2, size))
    sts_text = "".join(lines)
    glen = 300_000
    g = list(rnd(glen))
    at = 500
    near_n = 0
    for i, (p1, p2, size) in enumerate(planted):
        for form in range(4):
            a, b = (p1, p2) if form % 2 == 0 else (p2, O.revcomp(p1))
            amp = list(a + rnd(max(0, size - len(a) - len(b) + int(rng.integers(-50, 51)))) + b)
            if form >= 2:                      # the same amplicon with an 'N' inside the seed window
                if a[:16] not in ("A" * 16, "T" * 16):
                    continue
                amp[int(rng.integers(0, 16))] = "N"
                near_n += 1
            g[at:at + len(amp)] = amp
            at += len(amp) + int(rng.integers(5, 300))
    for _ in range(60):                        # runs: every window of a run seeds key 0 or 2^32 - 1
        a = int(rng.integers(at, glen - 200))
        n = int(rng.integers(16, 120))
        g[a:a + n] = "AT"[int(rng.integers(0, 2))] * n
        if rng.random() < 0.5:
            g[a + int(rng.integers(0, n))] = "N"
        if rng.random() < 0.3:
            g[a - 1] = "N"
    assert at < glen
    gb = np.frombuffer("".join(g)[:glen].encode(), dtype=np.uint8)
    prm = dict(wordsize=W, mismatches=N, iupac_mode=I, margin=50)
    table = O.load_sts_lines(sts_text.splitlines(True), W, 240)
    ref = C.search(table, [gb], O.params(**prm), 4)
    keys = np.array([table.records[int(r)].key for r in ref["rec"]], dtype=np.uint64)
    n0, n1 = int((keys == 0).sum()), int((keys == 2**32 - 1).sum())
    counts = dict(hits=len(ref), key0=n0, key_max=n1, n_in_seed=near_n,
                  bucket0=len(table.buckets[0]), bucket_max=len(table.buckets[2**32 - 1]))
    return sts_text, gb, prm, ref, counts


@pytest.mark.parametrize("I", [0, 1])
def test_keys_at_the_ends_of_the_key_space(I):
    """W = 16: primers that start with A x 16 (key 0) and T x 16 (key 2^32 - 1), 20 records per
    key, against a genome with their amplicons and long A and T runs.  An A run cut by an 'N'
    must not seed: the 2-bit plane reads 'N' as 'A', and the primer compare would accept it (one
    mismatch at I = 0, none at I = 1)."""
    sts_text, gb, prm, ref, counts = _ends_case(I)
    print(counts)
    assert counts["key0"] >= 20 and counts["key_max"] >= 20 and counts["n_in_seed"] >= 20, counts
    assert counts["bucket0"] >= 10 and counts["bucket_max"] >= 10, counts
    hits = _hits(_engine(sts_text, prm), gb)
    assert len(hits) == len(ref) and hits.tobytes() == ref.tobytes()


# ------------------------------------------------------------------ c. probes that wrap
def _slot(key, lg):
    return ((key * 0x9E3779B97F4A7C15) & (2**64 - 1)) >> (64 - lg)


def _wrapping_keys(table):
    """Keys that linear insertion in first-appearance order places by stepping from the last
    slot to slot 0.  This restates the table build only to choose and count inputs; what the
    search returns is compared with the oracle."""
    lg = 6
    while (1 << lg) < 2 * len(table.buckets):
        lg += 1
    used, wrapped = set(), set()
    for key in table.buckets:                  # dict order: first appearance
        s = s0 = _slot(key, lg)
        while s in used:
            s = (s + 1) & ((1 << lg) - 1)
        used.add(s)
        if s < s0:
            wrapped.add(key)
    return wrapped, lg


def test_probe_wraps_past_the_last_slot():
    """60 half-full slot tables (32, 64 and 128 distinct keys in 64, 128 and 256 slots), W 14-16,
    each against a 60 kbp genome that holds an exact amplicon of every record: a cluster that
    straddles the last slot must be walked round to slot 0 by the lookup as by the build."""
    tables_wrapping, hits_of_wrapped, total = 0, 0, 0
    for seed in range(60):
        n_sts = (16, 32, 64)[seed % 3]
        W = 14 + (seed // 3) % 3
        rng = np.random.default_rng(1000 + seed)

        def rnd(n):
            return ACGT[rng.integers(0, 4, n)].tobytes().decode()

        sts = [(rnd(int(rng.integers(W, 28))), rnd(int(rng.integers(W, 28))), int(rng.integers(60, 200)))
               for _ in range(n_sts)]
        sts_text = "".join(f"P{seed}_{i}\t{a}\t{b}\t{n}\n" for i, (a, b, n) in enumerate(sts))
        table = O.load_sts_lines(sts_text.splitlines(True), W, 240)
        assert len(table.buckets) == 2 * n_sts        # exactly half of 2^lg slots
        wrapped, lg = _wrapping_keys(table)
        assert 1 << lg == 4 * n_sts
        g = list(rnd(60_000))
        at = 100
        for a, b, n in sts:
            for x, y in ((a, b), (b, O.revcomp(a))):
                amp = x + rnd(max(0, n - len(x) - len(y))) + y
                g[at:at + len(amp)] = amp
                at += len(amp) + 20
        assert at < 58_000
        gb = np.frombuffer("".join(g).encode(), dtype=np.uint8)
        prm = dict(wordsize=W, mismatches=0, margin=50)
        ref = C.search(table, [gb], O.params(**prm), 2)
        assert len(ref) >= 2 * n_sts
        hits = _hits(_engine(sts_text, prm), gb)
        assert len(hits) == len(ref) and hits.tobytes() == ref.tobytes(), seed
        tables_wrapping += bool(wrapped)
        hits_of_wrapped += sum(table.records[int(r)].key in wrapped for r in ref["rec"])
        total += len(ref)
    print(dict(tables_wrapping=tables_wrapping, hits_of_wrapped_keys=hits_of_wrapped, hits=total))
    assert tables_wrapping >= 5 and hits_of_wrapped >= 1
