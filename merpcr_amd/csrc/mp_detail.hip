// Per-hit details of a completed search run: the mismatch count of each primer and the
// amplicon text, computed on the device from what the run left resident -- the sorted hit
// list (Search::out), the genome planes with their exception-run index, and the primers'
// accept planes and raw bytes.  Nothing here runs inside a search: the search kernels and
// their lists are untouched, and a handle that never asks for details allocates nothing.
//
// annotate_kernel: one lane per hit.  The hits are sorted by (sequence, pos1), so the 64
//   hits of a wave read neighbouring genome lines; each lane makes the two compares of
//   _compare_seqs (engine.py:599-642) in 32-base chunks through the accept planes, with no
//   mismatch cap and no 3' exit: every position is counted.
// amplicon kernels: length_kernel writes pos2 - pos1 + 1 per hit, a rocPRIM exclusive scan
//   makes the offsets, and amplicon_kernel gives each amplicon to a group of lanes -- a whole
//   wave, or a quarter of one when the window's mean amplicon is at most 512 bytes (a 250-base
//   product is 16 lines: a wave of its own would leave 48 lanes idle) -- grid-stride over the
//   hits: the text is cut at the 16-byte lines of the OUTPUT, one line per lane per pass, so
//   every store but the ragged first and last line is one aligned 16-B store and a group
//   writes contiguously; the 16 bases of a line come from the 2-bit plane at whatever base
//   alignment that implies (ext2), exception bases from the run index.
#include <algorithm>
#include <rocprim/device/device_scan.hpp>

#include "mp_internal.h"

namespace mp {

struct Detail {
    mp_hit_info* info = nullptr;  // annotate output
    uint64_t info_cap = 0;
    uint64_t* len = nullptr;      // amplicon lengths, count + 1 (the last one 0)
    uint64_t* off = nullptr;      // their exclusive prefix sum, count + 1
    uint64_t off_cap = 0;
    void* scan_tmp = nullptr;
    size_t scan_tmp_bytes = 0;
    uint8_t* bytes = nullptr;     // concatenated amplicon text
    uint64_t bytes_cap = 0;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    // the last call's kernels alone (device events): annotate_kernel; length_kernel + the scan
    // (ev 0-1) plus amplicon_kernel (ev 2-3), without the offsets' readback between them
    float annotate_ms = -1.f, amplicon_ms = -1.f;
};

void free_detail(Search* s) {
    Detail* d = s->detail;
    if (!d) return;
    hipFree(d->info); hipFree(d->len); hipFree(d->off); hipFree(d->scan_tmp); hipFree(d->bytes);
    for (hipEvent_t e : d->ev)
        if (e) hipEventDestroy(e);
    delete d;
    s->detail = nullptr;
    s->detail_bytes = 0;
}

namespace {

struct DetailArgs {
    const mp_hit* hits;          // the window's first hit
    uint64_t count;
    const uint64_t* g2;          // Genome planes
    const uint64_t* gexc;
    const uint64_t* gpair;
    const uint64_t* xr_start;    // exception-run index
    const uint8_t* xr_char;
    const uint32_t* xr_dir;
    uint64_t n_xr;
    const uint64_t* seq_base;
    const DevRec* recs;          // Table
    const uint64_t* planes;
    const uint8_t* pchars;
    int I;
};

// 32-bit per-base mask (bit 31-i) -> spaced form (bit 62-2i), and back (as mp_search.hip's).
__device__ __forceinline__ uint64_t spread32(uint32_t v) {
    uint64_t x = v;
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & kEven;
    return x;
}
__device__ __forceinline__ uint32_t compress_even(uint64_t x) {
    x &= kEven;
    x = (x | (x >> 1)) & 0x3333333333333333ull;
    x = (x | (x >> 2)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x >> 4)) & 0x00FF00FF00FF00FFull;
    x = (x | (x >> 8)) & 0x0000FFFF0000FFFFull;
    x = (x | (x >> 16)) & 0x00000000FFFFFFFFull;
    return (uint32_t)x;
}

// Run of exception base j: the run index entry with the largest start <= j, searched between
// the directory bounds of j's 4096-base block (exc_run of mp_search.hip).  j must be an
// exception base of a packed sequence (never padding), so such a run exists.
__device__ __forceinline__ uint64_t run_of(const DetailArgs& a, uint64_t j) {
    const uint64_t b = j >> kDirShift;
    uint64_t lo = a.xr_dir[b];
    const uint64_t d1 = (uint64_t)a.xr_dir[b + 1] + 1;
    uint64_t hi = d1 < a.n_xr ? d1 : a.n_xr;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (a.xr_start[mid] <= j) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Forward walk over the run index: the character of exception base pos, for calls with
// rising pos.
struct RunWalk {
    uint64_t j, nxt;
    uint8_t ch;
    __device__ __forceinline__ RunWalk(const DetailArgs& a, uint64_t first) {
        j = run_of(a, first);
        ch = a.xr_char[j];
        nxt = j + 1 < a.n_xr ? a.xr_start[j + 1] : ~0ull;
    }
    __device__ __forceinline__ uint8_t at(const DetailArgs& a, uint64_t pos) {
        while (pos >= nxt) {  // a later run starts at or before pos
            ++j;
            ch = a.xr_char[j];
            nxt = j + 1 < a.n_xr ? a.xr_start[j + 1] : ~0ull;
        }
        return ch;
    }
};

// Mismatching positions of one chunk (bases c .. c+len-1 of a primer, len <= 32): chunk_ok's
// per-position rule (mp_search.hip; engine.py:613-631) without its N cap and 3' exit.
// G: the genome window (2-bit, base c on top), ex / wild: its exception and 'N' bits (bit
// 31-i), P: the primer chunk's accept planes, gpos_c / ch_c: the chunk's first genome base
// and primer byte.
__device__ __forceinline__ int chunk_mm(const DetailArgs& a, uint64_t G, uint32_t ex, uint32_t wild, uint64_t P0,
                                        uint64_t P1, uint64_t P2, uint64_t P3, uint64_t gpos_c, uint32_t ch_c, int len) {
    const uint64_t lo = G & kEven, hi = (G >> 1) & kEven;
    const uint64_t nlo = lo ^ kEven, nhi = hi ^ kEven;
    const uint64_t match = (nhi & nlo & P0) | (nhi & lo & P1) | (hi & nlo & P2) | (hi & lo & P3);
    const uint64_t inside = sp_lt(len);
    const uint64_t acgt = (P0 | P1 | P2 | P3) & kEven;  // primer positions with an IUPAC meaning
    uint64_t mmv = ~match & inside;
    if (len < 32) ex &= ~(0xFFFFFFFFu >> len);
    if (a.I) {
        // a genome 'N' matches exactly the primer bases with an IUPAC meaning (char_match);
        // its 2-bit code (A) left the other positions mismatched, as 'N' against them is
        wild &= ex;
        mmv &= ~(spread32(wild) & acgt);
        ex &= ~wild;
    } else {
        // literal compare: a genome exception character is never exactly A/C/G/T, so it
        // mismatches every primer base that is one of them (a plane bit set under I = 0)
        mmv |= spread32(ex) & acgt & inside;
        ex &= ~compress_even(acgt);
    }
    if (ex) {  // the other exception bases: their characters from the run index
        RunWalk w(a, gpos_c + (uint32_t)__clz(ex));
        while (ex) {
            const int i = __clz(ex);
            ex &= ~(0x80000000u >> i);
            const bool ok = char_match(w.at(a, gpos_c + (uint32_t)i), a.pchars[ch_c + (uint32_t)i], a.I);
            const uint64_t bit = 1ull << (62 - 2 * i);
            mmv = ok ? (mmv & ~bit) : (mmv | bit);
        }
    }
    return __popcll(mmv);
}

// Mismatching positions of the L genome bases at global gpos against one primer (planes from
// chunk pl, bytes from ch).  Reads the interleaved planes as primer_ok does: a chunk at base j
// reads blocks j >> 6 and (j >> 6) + 1 of gpair, which seal fills for every block up to
// total / 64 + 1.
__device__ __forceinline__ uint32_t primer_mm(const DetailArgs& a, uint64_t gpos, uint32_t L, uint32_t pl, uint32_t ch) {
    int mm = 0;
    for (uint32_t c = 0; c < L; c += 32) {
        const int len = (int)min(32u, L - c);
        const uint64_t G = ext2p(a.gpair, gpos + c);
        const uint32_t ex = (uint32_t)(ext1p<2>(a.gpair, gpos + c) >> 32);
        const uint32_t wl = a.I && ex ? (uint32_t)(ext1p<3>(a.gpair, gpos + c) >> 32) : 0u;
        const uint64_t* P = a.planes + (uint64_t)(pl + (c >> 5)) * 4;
        mm += chunk_mm(a, G, ex, wl, P[0], P[1], P[2], P[3], gpos + c, ch + c, len);
    }
    return (uint32_t)mm;
}

constexpr int kDetailBlock = 256;

__global__ __launch_bounds__(kDetailBlock) void annotate_kernel(DetailArgs a, mp_hit_info* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * kDetailBlock + threadIdx.x;
    if (i >= a.count) return;
    const mp_hit h = a.hits[i];
    const DevRec r = a.recs[h.rec];
    const uint64_t base = a.seq_base[h.seq];
    // primer 1 over [pos1, pos1 + l1), primer 2 over [pos2 + 1 - l2, pos2 + 1)
    const uint32_t m1 = primer_mm(a, base + h.pos1, r.l1, r.p1_pl, r.p1_ch);
    const uint32_t m2 = primer_mm(a, base + h.pos2 + 1 - r.l2, r.l2, r.p2_pl, r.p2_ch);
    mp_hit_info o;
    o.mm1 = (uint8_t)min(m1, 255u);
    o.mm2 = (uint8_t)min(m2, 255u);
    out[i] = o;
}

// len[i] = pos2 - pos1 + 1 for the window's hits, len[count] = 0 (its scan slot is the total).
__global__ __launch_bounds__(kDetailBlock) void length_kernel(const mp_hit* __restrict__ hits, uint64_t count,
                                                              uint64_t* __restrict__ len) {
    const uint64_t i = (uint64_t)blockIdx.x * kDetailBlock + threadIdx.x;
    if (i > count) return;
    len[i] = i < count ? hits[i].pos2 - hits[i].pos1 + 1 : 0ull;
}

// Upper-cased text of every amplicon of the window into out at off[i] (out is 16-B aligned,
// off[0] = 0).  One group of kGroup lanes (16 or 64) per amplicon; lane l of pass p takes output
// line a0 + 16 (kGroup p + l), a0 = off[i] rounded down to 16: its bytes inside
// [off[i], off[i + 1]) are n <= 16 bases from global base j on.  No lane exchanges data with
// another, so the groups of a wave run their own trip counts.  A whole line is one 16-B store; the ragged first and last lines go out
// byte by byte, so nothing outside [off[0], off[count]) is written.
// Plane reads: ext2 / ext1 at a base j of the amplicon read words j >> 5, (j >> 5) + 1 of g2
// and j >> 6, (j >> 6) + 1 of gexc, whatever n is.  j < total (an amplicon lies inside its
// sequence), so these are the words ext2 reads for the search's own last window, inside the
// planes' allocation of total / 32 + 4 and total / 64 + 4 words (mp_genome.hip place()).
// Exception bits past the line's n bases are masked before any run lookup: padding bases
// have gexc set but no run.
template <uint32_t kGroup>
__global__ __launch_bounds__(kDetailBlock) void amplicon_kernel(DetailArgs a, const uint64_t* __restrict__ off,
                                                                uint8_t* __restrict__ out) {
    static_assert(kGroup == 16 || kGroup == 64, "lanes per amplicon");
    const uint32_t lane = threadIdx.x & (kGroup - 1u);
    const uint64_t group0 = ((uint64_t)blockIdx.x * kDetailBlock + threadIdx.x) / kGroup;
    const uint64_t n_groups = ((uint64_t)gridDim.x * kDetailBlock) / kGroup;
    for (uint64_t i = group0; i < a.count; i += n_groups) {  // uniform over the group
        const mp_hit h = a.hits[i];
        const uint64_t o0 = off[i], o1 = off[i + 1];
        const uint64_t g0 = a.seq_base[h.seq] + h.pos1;
        const uint64_t a0 = o0 & ~15ull;
        const uint64_t n_lines = (o1 - a0 + 15) >> 4;
        for (uint64_t ln = lane; ln < n_lines; ln += kGroup) {
            const uint64_t ob = a0 + (ln << 4);
            const uint64_t lo = ob > o0 ? ob : o0;
            const uint64_t hi = ob + 16 < o1 ? ob + 16 : o1;
            const uint32_t n = (uint32_t)(hi - lo);  // 1..16
            const uint64_t j = g0 + (lo - o0);
            const uint32_t code = (uint32_t)(ext2(a.g2, j) >> 32);  // 16 bases, base j on top
            uint32_t ex = (uint32_t)(ext1(a.gexc, j) >> 48) & ~(0xFFFFu >> n);
            uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const uint32_t c = (code >> (30 - 2 * k)) & 3u;
                w[k >> 2] |= ((0x54474341u >> (8u * c)) & 0xFFu) << (8 * (k & 3));  // "ACGT"[c]
            }
            if (ex) {  // exception bases: the character of the last run starting at or before each
                RunWalk rw(a, j + ((uint32_t)__clz(ex) - 16u));
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if (ex & (0x8000u >> k)) {
                        const uint32_t ch = rw.at(a, j + (uint32_t)k);
                        w[k >> 2] = (w[k >> 2] & ~(0xFFu << (8 * (k & 3)))) | (ch << (8 * (k & 3)));
                    }
            }
            if (n == 16) {
                *reinterpret_cast<uint4*>(out + ob) = make_uint4(w[0], w[1], w[2], w[3]);
            } else {
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if ((uint32_t)k < n) out[lo + (uint32_t)k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
            }
        }
    }
}

int detail_of(Search* s, Detail** out) {
    if (!s->detail) {
        Detail* d = new Detail();
        s->detail = d;  // freed with the handle
        for (hipEvent_t& e : d->ev)
            if (hipEventCreate(&e) != hipSuccess) return fail(MP_E_HIP, "mp_search details: event creation failed");
    }
    *out = s->detail;
    return MP_OK;
}

void account(Search* s) {
    const Detail* d = s->detail;
    s->detail_bytes = d->info_cap * sizeof(mp_hit_info) + d->off_cap * 16 + d->scan_tmp_bytes + d->bytes_cap;
}

// The checks every detail call starts with; on MP_OK with count > 0 the device is current.
int detail_window(Search* s, const char* who, uint64_t first, uint64_t count) {
    if (!s) return fail(MP_E_ARG, std::string(who) + ": null search");
    if (s->pending) return fail(MP_E_STATE, std::string(who) + ": a run is enqueued (mp_search_complete first)");
    if (!s->has_run) return fail(MP_E_STATE, std::string(who) + ": no completed run on this handle");
    if (s->run_gen != s->genome->gen || !s->genome->sealed)
        return fail(MP_E_STATE, std::string(who) + ": the genome was reset or refilled since the run");
    if (first > s->n_hits || count > s->n_hits - first)
        return fail(MP_E_ARG, std::string(who) + ": window past the run's " + std::to_string(s->n_hits) + " hits");
    return MP_OK;
}

DetailArgs detail_args(const Search* s, uint64_t first, uint64_t count) {
    const Genome* g = s->genome;
    const Table* t = s->table;
    DetailArgs a{};
    a.hits = s->out + first;
    a.count = count;
    a.g2 = g->g2; a.gexc = g->gexc; a.gpair = g->gpair;
    a.xr_start = g->xr_start; a.xr_char = g->xr_char; a.xr_dir = g->xr_dir; a.n_xr = g->n_xr;
    a.seq_base = g->d_base;
    a.recs = t->recs; a.planes = t->planes; a.pchars = t->pchars;
    a.I = t->prm.iupac_mode;
    return a;
}

}  // namespace
}  // namespace mp

using namespace mp;

MP_EXPORT int mp_search_annotate(void* search, uint64_t first, uint64_t count, mp_hit_info* host_out, void* stream) {
    Search* s = (Search*)search;
    int rc = detail_window(s, "mp_search_annotate", first, count);
    if (rc) return rc;
    if (!count) return MP_OK;
    if (!host_out) return fail(MP_E_ARG, "mp_search_annotate: null output");
    MP_HIP_CHECK(hipSetDevice(s->genome->device));
    Detail* d = nullptr;
    rc = detail_of(s, &d);
    if (rc) return rc;
    if (count > d->info_cap) {
        hipFree(d->info);
        d->info = nullptr;
        d->info_cap = 0;
        account(s);
        const uint64_t cap = count + count / 4;
        if (hipMalloc(&d->info, cap * sizeof(mp_hit_info)) != hipSuccess)
            return fail(MP_E_NOMEM, "mp_search_annotate: device allocation failed");
        d->info_cap = cap;
        account(s);
    }
    hipStream_t st = (hipStream_t)stream;
    const DetailArgs a = detail_args(s, first, count);
    MP_HIP_CHECK(hipEventRecord(d->ev[0], st));
    hipLaunchKernelGGL(annotate_kernel, dim3((uint32_t)((count + kDetailBlock - 1) / kDetailBlock)), dim3(kDetailBlock), 0,
                       st, a, d->info);
    MP_HIP_CHECK(hipGetLastError());
    MP_HIP_CHECK(hipEventRecord(d->ev[1], st));
    MP_HIP_CHECK(hipMemcpyAsync(host_out, d->info, count * sizeof(mp_hit_info), hipMemcpyDeviceToHost, st));
    MP_HIP_CHECK(hipStreamSynchronize(st));
    MP_HIP_CHECK(hipEventElapsedTime(&d->annotate_ms, d->ev[0], d->ev[1]));
    return MP_OK;
}

MP_EXPORT int mp_search_amplicons(void* search, uint64_t first, uint64_t count, uint8_t* host_out, uint64_t cap,
                                  uint64_t* off, uint64_t* n_bytes, void* stream) {
    Search* s = (Search*)search;
    if (n_bytes) *n_bytes = 0;
    int rc = detail_window(s, "mp_search_amplicons", first, count);
    if (rc) return rc;
    if (!off || !n_bytes) return fail(MP_E_ARG, "mp_search_amplicons: null pointer");
    if (!count) {
        off[0] = 0;
        return MP_OK;
    }
    MP_HIP_CHECK(hipSetDevice(s->genome->device));
    Detail* d = nullptr;
    rc = detail_of(s, &d);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const uint64_t n1 = count + 1;
    if (n1 > d->off_cap) {
        hipFree(d->len); hipFree(d->off); hipFree(d->scan_tmp);
        d->len = d->off = nullptr;
        d->scan_tmp = nullptr;
        d->off_cap = 0;
        d->scan_tmp_bytes = 0;
        account(s);
        const uint64_t c = n1 + n1 / 4;
        size_t tb = 0;
        MP_HIP_CHECK(rocprim::exclusive_scan(nullptr, tb, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, (size_t)c,
                                             rocprim::plus<uint64_t>(), st));
        tb = std::max<size_t>(tb, 16);
        if (hipMalloc(&d->len, c * 8) != hipSuccess || hipMalloc(&d->off, c * 8) != hipSuccess ||
            hipMalloc(&d->scan_tmp, tb) != hipSuccess) {
            hipFree(d->len); hipFree(d->off); hipFree(d->scan_tmp);
            d->len = d->off = nullptr;
            d->scan_tmp = nullptr;
            return fail(MP_E_NOMEM, "mp_search_amplicons: device allocation failed");
        }
        d->off_cap = c;
        d->scan_tmp_bytes = tb;
        account(s);
    }
    const DetailArgs a = detail_args(s, first, count);
    MP_HIP_CHECK(hipEventRecord(d->ev[0], st));
    hipLaunchKernelGGL(length_kernel, dim3((uint32_t)((n1 + kDetailBlock - 1) / kDetailBlock)), dim3(kDetailBlock), 0, st,
                       a.hits, count, d->len);
    MP_HIP_CHECK(hipGetLastError());
    size_t tb = d->scan_tmp_bytes;
    MP_HIP_CHECK(rocprim::exclusive_scan(d->scan_tmp, tb, d->len, d->off, (uint64_t)0, (size_t)n1, rocprim::plus<uint64_t>(), st));
    MP_HIP_CHECK(hipEventRecord(d->ev[1], st));
    MP_HIP_CHECK(hipMemcpyAsync(off, d->off, n1 * 8, hipMemcpyDeviceToHost, st));
    MP_HIP_CHECK(hipStreamSynchronize(st));
    const uint64_t need = off[count];
    *n_bytes = need;
    if (!host_out) return MP_OK;  // size query
    if (cap < need) return fail(MP_E_CAP, "mp_search_amplicons: output buffer too small");
    if (need > d->bytes_cap) {
        hipFree(d->bytes);
        d->bytes = nullptr;
        d->bytes_cap = 0;
        account(s);
        const uint64_t c = round_up(need + need / 4, 256);
        if (hipMalloc(&d->bytes, c) != hipSuccess) return fail(MP_E_NOMEM, "mp_search_amplicons: device allocation failed");
        d->bytes_cap = c;
        account(s);
    }
    // a quarter wave per amplicon while the mean amplicon is at most 32 lines, else a wave; a
    // grid past ~8 blocks per CU only adds launches
    const bool narrow = need / count <= 512;
    const uint64_t per_block = kDetailBlock / (narrow ? 16 : 64);
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((count + per_block - 1) / per_block, 2048);
    MP_HIP_CHECK(hipEventRecord(d->ev[2], st));
    if (narrow) hipLaunchKernelGGL(amplicon_kernel<16>, dim3(blocks), dim3(kDetailBlock), 0, st, a, d->off, d->bytes);
    else hipLaunchKernelGGL(amplicon_kernel<64>, dim3(blocks), dim3(kDetailBlock), 0, st, a, d->off, d->bytes);
    MP_HIP_CHECK(hipGetLastError());
    MP_HIP_CHECK(hipEventRecord(d->ev[3], st));
    MP_HIP_CHECK(hipMemcpyAsync(host_out, d->bytes, need, hipMemcpyDeviceToHost, st));
    MP_HIP_CHECK(hipStreamSynchronize(st));
    float t_scan = 0.f, t_text = 0.f;
    MP_HIP_CHECK(hipEventElapsedTime(&t_scan, d->ev[0], d->ev[1]));
    MP_HIP_CHECK(hipEventElapsedTime(&t_text, d->ev[2], d->ev[3]));
    d->amplicon_ms = t_scan + t_text;
    return MP_OK;
}

MP_EXPORT int mp_search_detail_timing(void* search, float* annotate_ms, float* amplicon_ms) {
    Search* s = (Search*)search;
    if (!s) return fail(MP_E_ARG, "mp_search_detail_timing: null search");
    if (annotate_ms) *annotate_ms = s->detail ? s->detail->annotate_ms : -1.f;
    if (amplicon_ms) *amplicon_ms = s->detail ? s->detail->amplicon_ms : -1.f;
    return MP_OK;
}
