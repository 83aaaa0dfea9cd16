"""Per-hit details, the host side: the two formatters (mp_format_hits_ex, mp_format_amplicons)
against Python f-strings, the ABI struct, the CLI options and the engine's argument checks.
None of this needs a GPU; tests/test_gpu_details.py covers the device calls.
"""

import ctypes
import os
import subprocess

import numpy as np
import pytest

from merpcr_amd import FASTARecord, MerPCR, _native, cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LABELS = ["chr1", "L78833", "séq_ſ", "x" * 300, "中文"]
RECS = [("AFM248yg9", "(D17S932)  Chr.17, 63.7 cM", "-"), ("s1", "", "+"), ("é", "a\x0bb\x1cc", "+"),
        ("id", "alias with spaces", "-")]
SIZES = np.array([201, 1, 10000, 2**40], dtype=np.uint64)


def _fmt():
    return _native.Formatter(LABELS, [f"{i}\t{a}\t({d})" for i, a, d in RECS])


def _hits(n, seed):
    rng = np.random.default_rng(seed)
    h = np.zeros(n, dtype=_native.HIT_DTYPE)
    p1 = rng.integers(0, 1 << 40, n, dtype=np.uint64)
    p1[: min(n, 4)] = [0, 8, 9, 99][: min(n, 4)]
    h["pos1"] = p1
    h["pos2"] = p1 + rng.integers(0, 300, n, dtype=np.uint64)
    h["seq"] = rng.integers(0, len(LABELS), n)
    h["rec"] = rng.integers(0, len(RECS), n)
    info = rng.integers(0, 256, (n, 2)).astype(np.uint8)
    if n:
        info[0] = (0, 255)
    return h, info


def _bases(h, seed):
    """Random amplicon bytes of each hit's length (any byte but newline), and their offsets."""
    rng = np.random.default_rng(seed)
    ln = (h["pos2"] - h["pos1"] + 1).astype(np.int64)
    off = np.zeros(len(h) + 1, dtype=np.uint64)
    np.cumsum(ln, out=off[1:])
    data = rng.choice(np.frombuffer(b"ACGTNRYU\xc1\x80", dtype=np.uint8), int(off[-1]))
    return data, off


def _expected_ex(h, info):
    out = []
    for k in range(len(h)):
        p1, p2, sq, ri = int(h["pos1"][k]), int(h["pos2"][k]), int(h["seq"][k]), int(h["rec"][k])
        i, a, d = RECS[ri]
        out.append(f"{LABELS[sq]}\t{p1 + 1}..{p2 + 1}\t{i}\t{a}\t({d})\t{info[k, 0]}\t{info[k, 1]}\t"
                   f"{p2 - p1 + 1}/{int(SIZES[ri])}\n")
    return "".join(out).encode("utf-8")


def _expected_fasta(h, data, off):
    out = []
    for k in range(len(h)):
        p1, p2, sq, ri = int(h["pos1"][k]), int(h["pos2"][k]), int(h["seq"][k]), int(h["rec"][k])
        i, a, d = RECS[ri]
        out.append(f">{LABELS[sq]}:{p1 + 1}..{p2 + 1}\t{i}\t{a}\t({d})\n".encode("utf-8") +
                   data[int(off[k]):int(off[k + 1])].tobytes() + b"\n")
    return b"".join(out)


@pytest.mark.parametrize("n", [0, 1, 7, 1000, 40_000])
def test_format_hits_ex_matches_fstring(n):
    """n = 40,000 takes the threaded fill (more than 8,192 hits per thread's share)."""
    h, info = _hits(n, n)
    assert _fmt().detailed(h, info, SIZES) == _expected_ex(h, info)


@pytest.mark.parametrize("n", [0, 1, 7, 1000, 40_000])
def test_format_amplicons_matches_fstring(n):
    h, _ = _hits(n, n + 1)
    data, off = _bases(h, n)
    assert _fmt().amplicons(h, data, off) == _expected_fasta(h, data, off)


def test_format_amplicons_takes_a_window_of_the_offsets():
    """off need not start at 0: a window's offsets into the whole byte buffer."""
    h, _ = _hits(20, 3)
    data, off = _bases(h, 3)
    assert _fmt().amplicons(h[5:9], data, off[5:10]) == _expected_fasta(h[5:9], data, off[5:10])


def test_format_edge_coordinates():
    h = np.zeros(2, dtype=_native.HIT_DTYPE)
    h["pos1"] = [0, 999_999_999]
    h["pos2"] = [0, 1_000_000_008]
    info = np.array([[0, 0], [10, 9]], dtype=np.uint8)
    assert _fmt().detailed(h, info, SIZES) == _expected_ex(h, info)


def _raw_call(fn, h, extra, out, cap):
    f = _fmt()
    n = ctypes.c_uint64(12345)
    rc = fn(_native.ptr(h), h.size, _native.ptr(f.labels), _native.ptr(f.label_off), f.n_seq, _native.ptr(f.rec),
            _native.ptr(f.rec_off), f.n_rec, *extra, out, cap, ctypes.byref(n))
    return rc, n.value


def test_size_query_and_cap():
    """out == NULL reports the size; a short buffer fails with MP_E_CAP, reports the need and
    is left untouched."""
    lib = _native.lib()
    h, info = _hits(9, 5)
    data, off = _bases(h, 5)
    for fn, extra, want in ((lib.mp_format_hits_ex, (_native.ptr(info), _native.ptr(SIZES)), _expected_ex(h, info)),
                            (lib.mp_format_amplicons, (_native.ptr(data), _native.ptr(off)),
                             _expected_fasta(h, data, off))):
        rc, need = _raw_call(fn, h, extra, None, 0)
        assert (rc, need) == (_native.MP_OK, len(want))
        buf = np.full(len(want), 0xAB, dtype=np.uint8)
        rc, need = _raw_call(fn, h, extra, _native.ptr(buf), len(want) - 1)
        assert (rc, need) == (_native.MP_E_CAP, len(want))
        assert (buf == 0xAB).all()
        rc, need = _raw_call(fn, h, extra, _native.ptr(buf), len(want))
        assert rc == _native.MP_OK and buf.tobytes() == want
        # an empty list needs no bytes and no arrays
        e = h[:0]
        rc, need = _raw_call(fn, e, (None, None), None, 0)
        assert (rc, need) == (_native.MP_OK, 0)


def test_formatters_reject_bad_input():
    h, info = _hits(3, 1)
    data, off = _bases(h, 1)
    bad = h.copy()
    bad["rec"][2] = len(RECS)
    with pytest.raises(ValueError):
        _fmt().detailed(bad, info, SIZES)
    with pytest.raises(ValueError):
        _fmt().amplicons(bad, data, off)
    with pytest.raises(ValueError):
        _fmt().detailed(h, info[:2], SIZES)
    with pytest.raises(ValueError):
        _fmt().detailed(h, info, SIZES[:2])
    with pytest.raises(ValueError):
        _fmt().amplicons(h, data, off[:-1])
    dec = off.copy()
    dec[1], dec[2] = dec[2], dec[1]
    if dec[1] != dec[2]:
        with pytest.raises(ValueError):
            _fmt().amplicons(h, data, dec)


def test_hit_info_is_two_bytes(tmp_path):
    """sizeof(mp_hit_info) == 2 with mm1 first, checked by the host C compiler against the
    header; the ctypes mirror agrees."""
    src = tmp_path / "info.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "merpcr_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %d\\n", sizeof(mp_hit_info), offsetof(mp_hit_info, mm1),\n'
                   '                        offsetof(mp_hit_info, mm2), MP_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "info"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert out == ["2", "0", "1", "3"]
    assert ctypes.sizeof(_native.MPHitInfo) == 2
    assert (_native.MPHitInfo.mm1.offset, _native.MPHitInfo.mm2.offset) == (0, 1)


def test_cli_options():
    p = cli.create_parser()
    a = p.parse_args(["a.sts", "b.fa"])
    assert a.details is False and a.amplicons is None
    a = p.parse_args(["a.sts", "b.fa", "--details", "--amplicons", "amp.fa", "-N", "1"])
    assert a.details is True and a.amplicons == "amp.fa" and a.mismatches == 1
    a = p.parse_args(cli.convert_mepcr_arguments(["a.sts", "b.fa", "N=2", "--amplicons=out.fa"]))
    assert a.details is False and a.amplicons == "out.fa" and a.mismatches == 2


RECORD = [FASTARecord(defline=">x", sequence="ACGT" * 10)]


@pytest.mark.parametrize("kw", [dict(devices=[0, 1]), dict(devices=[0, 0]), dict(emulate_chunks=True, threads=2)])
def test_details_out_of_scope_is_value_error(kw, tmp_path, monkeypatch):
    """Multi-device engines and chunk emulation have no per-hit details: a ValueError before
    any device call (the native layer is made unreachable to show it)."""
    eng = MerPCR(**kw)

    def unreachable(*a, **k):
        raise AssertionError("a device call was made")

    for name in ("Table", "Genome", "Search", "Multi"):
        monkeypatch.setattr(_native, name, unreachable)
    out = tmp_path / "o.txt"
    with pytest.raises(ValueError):
        eng.find_hits_detailed(RECORD)
    with pytest.raises(ValueError):
        eng.find_hits_detailed(RECORD, amplicons=True)
    with pytest.raises(ValueError):
        eng.search(RECORD, str(out), details=True)
    with pytest.raises(ValueError):
        eng.search(RECORD, str(out), amplicon_file=str(tmp_path / "a.fa"))
    assert not out.exists()  # refused before the output file is opened


def test_emulate_chunks_single_thread_is_in_scope(monkeypatch):
    """emulate_chunks alone (threads = 1) searches one chunk: details are allowed, and the call
    goes on to the device."""
    eng = MerPCR(emulate_chunks=True, threads=1)
    eng._check_details()


def test_find_hits_detailed_without_gpu_fails_loudly():
    """No CPU fallback: without a device the call raises; with one it answers."""
    eng = MerPCR()
    if _native.device_count() == 0:
        with pytest.raises(Exception):
            eng.find_hits_detailed(RECORD)
        with pytest.raises(Exception):
            eng.find_hits_detailed(RECORD, amplicons=True)
    else:
        d = eng.find_hits_detailed(RECORD, amplicons=True)
        assert len(d) == 0 and d.mm1.shape == d.mm2.shape == d.size.shape == d.expected.shape == (0,)
