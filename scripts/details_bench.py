#!/usr/bin/env python
"""Timing of the per-hit detail kernels on the bench's c3 workload (100k STS x 3 Gbp, W=11 N=1,
seeded, built by merpcr_amd.synth exactly as bench.py builds it).

After one search, `--reps` repetitions (after `--warmup`) of
  * mp_search_annotate over every hit: the annotate kernel alone (the library's HIP events
    around it) and the host-visible call (kernel + result copy + synchronise);
  * mp_search_amplicons over every hit (the filling call): length kernel + offsets scan +
    amplicon kernel (events, without the offsets' readback between them) and the host-visible
    call, which also copies the text to the host;
  * the search itself, for the handle's own pair_ms (the pair kernel makes the same two
    compares for every fingerprint survivor, in unsorted order): the yardstick of annotate;
  * a device-to-device copy of as many bytes as the amplicon text (torch, events): the
    yardstick of the amplicon kernel's output rate.
Prints one JSON line (medians with min/max); --out saves it too.  Needs a GPU.
"""

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stat(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=["c2", "c3", "c4", "c5"])
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the config's genome and STS set")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import numpy as np
    import torch
    from merpcr_amd import MerPCR, _native, synth
    from merpcr_amd._build import source_digest

    if not torch.cuda.is_available():
        raise SystemExit("details_bench.py measures on the GPU: no HIP device is visible")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    cfg = dict(synth.CONFIGS[args.config])
    total = int(cfg["total"] * args.scale) // 64 * 64
    n_sts = max(1, int(cfg["n_sts"] * args.scale))
    sts = synth.make_sts(n_sts, W=cfg["W"], iupac=cfg["iupac"])
    eng = MerPCR(wordsize=cfg["W"], margin=cfg["M"], mismatches=cfg["N"], iupac_mode=cfg["I"], device=0)
    with tempfile.NamedTemporaryFile("w", suffix=".sts", delete=False) as fh:
        fh.write(sts.text())
    try:
        assert eng.load_sts_file(fh.name)
    finally:
        os.unlink(fh.name)
    table = eng.device_table()
    names, lens, buf, offs, planted = synth.build_genome_torch(
        total, cfg["records"], sts, seed=1, N=cfg["N"], M=cfg["M"], W=cfg["W"], nrun=cfg["nrun"], device=dev)
    torch.cuda.synchronize()
    genome = _native.Genome(0, lens)
    stream = torch.cuda.current_stream().cuda_stream
    for r, n in enumerate(lens):
        genome.put_device(r, buf.data_ptr() + int(offs[r]), n, stream=stream)
    genome.seal(stream)
    del buf
    search = _native.Search(table, genome)

    pair_ms, n_hits, survivors = [], 0, 0
    for i in range(args.warmup + args.reps):
        n_hits = search.run(None, stream)
        st = search.last_stats()
        survivors = st["survivors"]
        if i >= args.warmup:
            pair_ms.append(st["pair_ms"])
    hits = search.fetch(n_hits)

    ann_k, ann_call = [], []
    for i in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        mm = search.annotate(0, n_hits, stream=stream)
        dt = (time.perf_counter() - t0) * 1e3
        if i >= args.warmup:
            ann_k.append(search.detail_timing()["annotate_ms"])
            ann_call.append(dt)

    # the filling call alone is timed: offsets buffer and text buffer sized by one query
    off = np.zeros(n_hits + 1, dtype=np.uint64)
    need = _native.c_uint64(0)
    lib = _native.lib()
    _native.check(lib.mp_search_amplicons(search._h, 0, n_hits, None, 0, _native.ptr(off), _native.ctypes.byref(need),
                                          _native.c_void_p(stream)))
    text = np.empty(need.value, dtype=np.uint8)
    amp_k, amp_call = [], []
    for i in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        _native.check(lib.mp_search_amplicons(search._h, 0, n_hits, _native.ptr(text), text.size, _native.ptr(off),
                                              _native.ctypes.byref(need), _native.c_void_p(stream)))
        dt = (time.perf_counter() - t0) * 1e3
        if i >= args.warmup:
            amp_k.append(search.detail_timing()["amplicon_ms"])
            amp_call.append(dt)
    assert int(off[-1]) == need.value == int((hits["pos2"] - hits["pos1"] + 1).sum())

    # plain device-to-device copy of the same number of bytes
    src = torch.empty(max(1, need.value), dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    copy_ms = []
    for i in range(args.warmup + args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src, non_blocking=True)
        e1.record()
        e1.synchronize()
        if i >= args.warmup:
            copy_ms.append(e0.elapsed_time(e1))

    gbs = lambda ms: round(need.value / (ms * 1e-3) / 1e9, 1)  # noqa: E731
    res = {
        "tool": "details_bench", "config": args.config, "scale": args.scale, "reps": args.reps, "warmup": args.warmup,
        "build": source_digest(), "device": torch.cuda.get_device_name(0),
        "hits": int(n_hits), "survivors": int(survivors), "amplicon_bytes": int(need.value),
        "mm1_nonzero": int((mm[:, 0] > 0).sum()), "mm2_nonzero": int((mm[:, 1] > 0).sum()),
        "pair_ms": stat(pair_ms),
        "annotate_kernel_ms": stat(ann_k), "annotate_call_ms": stat(ann_call),
        "annotate_over_pair": round(statistics.median(ann_k) / statistics.median(pair_ms), 3),
        "annotate_bar": "median annotate kernel <= 1.5 x median pair_ms",
        "annotate_bar_met": bool(statistics.median(ann_k) <= 1.5 * statistics.median(pair_ms)),
        "amplicon_kernels_ms": stat(amp_k), "amplicon_call_ms": stat(amp_call),
        "amplicon_out_GBps": gbs(statistics.median(amp_k)),
        "d2d_copy_ms": stat(copy_ms), "d2d_copy_GBps": gbs(statistics.median(copy_ms)),
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
