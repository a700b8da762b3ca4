// Statistics over an id stream that is already in device memory (the dataset encoder runs them on
// each region's ids while they are still in HBM or L2 from the emit; bpe_amd.id_counts and
// id_positions run them on a caller's tensor):
//   ids_histogram : counts[id] += occurrences, 64-bit, into the caller's table
//   ids_find      : the positions of one id, ascending (an ordered compaction)
// and the host-side carry rule of the dataset encoder's read grid (bpe_window_holdback).
//
// Both kernels take ids of 2, 4 or 8 bytes that start at any element offset: a region begins where
// the previous one ended, so only the element's own alignment can be assumed.  The stream is read
// as 16-byte vectors on the 16-byte grid of the address space; the first and the last vector of the
// grid may lie partly outside [0, n) and are loaded element by element, every other one with one
// 16-byte load (load_ids, idload.h).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "idload.h"
#include "internal.h"
#include "prims.h"

namespace bpe {
namespace {

// ------------------------------------------------------------------ id histogram
// BPE ids are Zipfian and the frequent ones are the low ones (bytes, early merges), while one
// global address takes only about 88 returning atomics per microsecond on this chip (DESIGN.md
// section 4, k_find_specials).  Each workgroup therefore counts the ids below kHistCells in a
// private LDS table of 32-bit cells and sends only the rest to 64-bit global adds; at the end (and
// at the flush bound below) it adds its non-zero cells to the caller's table with 64-bit
// no-return adds.  kHistCells = 8192 is 32 KiB of LDS: the grid runs four workgroups of 256
// threads per CU (five would fit its 160 KiB; the kernel takes 36 VGPRs and no scratch), the
// residency a streaming kernel wants, and GPT-2's ids below 8192 cover most of a natural text's
// tokens.
//
// Invariant (no private cell can wrap): a cell counts at most the ids its workgroup has consumed
// since the last flush, a workgroup consumes 256 x V ids per step of its loop, and it flushes
// before a step that would take the ids consumed since the last flush past flush_ids <= 2^31.
constexpr unsigned kHistCells = 8192;
constexpr unsigned long long kHistFlushIds = 1ull << 31;

template <class E>
__global__ void __launch_bounds__(256)
k_ids_hist(const E* __restrict__ ids, size_t n, unsigned sh, size_t nvec, unsigned long long* __restrict__ counts,
           unsigned long long n_counts, unsigned long long flush_ids, unsigned long long* __restrict__ bad) {
    constexpr unsigned V = 16 / sizeof(E);
    __shared__ unsigned cell[kHistCells];
    for (unsigned c = threadIdx.x; c < kHistCells; c += 256) cell[c] = 0;
    __syncthreads();
    auto flush = [&] {
        __syncthreads();
        for (unsigned c = threadIdx.x; c < kHistCells; c += 256) {
            const unsigned k = cell[c];
            if (k) {   // c < n_counts: only ids below n_counts are counted
                atomicAdd(&counts[c], (unsigned long long)k);
                cell[c] = 0;
            }
        }
        __syncthreads();
    };
    auto add = [&](unsigned long long id, unsigned k) {
        if (id >= n_counts) atomicMin(bad, id);
        else if (id < kHistCells) atomicAdd(&cell[(unsigned)id], k);
        else atomicAdd(&counts[id], (unsigned long long)k);
    };
    unsigned long long consumed = 0;
    for (size_t b0 = (size_t)blockIdx.x * 256; b0 < nvec; b0 += (size_t)gridDim.x * 256) {
        if (consumed + 256ull * V > flush_ids) {   // uniform over the workgroup
            flush();
            consumed = 0;
        }
        consumed += 256ull * V;
        const size_t j = b0 + threadIdx.x;
        if (j >= nvec) continue;
        E v[V];
        const unsigned m = load_ids(ids, n, sh, j, v);
        // equal neighbours (a run of one id) go out as one add
        unsigned long long cur = 0;
        unsigned run = 0;
#pragma unroll
        for (unsigned k = 0; k < V; ++k) {
            if (!(m >> k & 1u)) continue;
            const unsigned long long id = (unsigned long long)v[k];
            if (run && id == cur) { ++run; continue; }
            if (run) add(cur, run);
            cur = id;
            run = 1;
        }
        if (run) add(cur, run);
    }
    flush();
}

// ------------------------------------------------------------------ positions of one id
// Ordered compaction in the two-pass shape of k_enc_emit: every workgroup owns `iters` x 256
// consecutive vectors; pass 1 counts its matches, an exclusive scan gives its first output index,
// pass 2 scans the same vectors again and writes base + element index.  Nothing is staged in LDS:
// in pass 2 a block-wide exclusive scan of the threads' match counts per step places every match
// directly, so a workgroup whose every id matches writes as many positions as it reads ids.
// Positions past `cap` are counted and not written.
__device__ __forceinline__ unsigned block_excl_scan(unsigned c, unsigned* wtot, unsigned& total) {
    const unsigned lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(inc, o);
        if ((int)lane >= o) inc += t;
    }
    if (lane == 63) wtot[w] = inc;
    __syncthreads();
    unsigned before = 0;
    total = 0;
#pragma unroll
    for (unsigned i = 0; i < 4; ++i) {
        const unsigned t = wtot[i];
        before += i < w ? t : 0u;
        total += t;
    }
    __syncthreads();   // wtot is rewritten by the next step
    return before + inc - c;
}

template <class E, bool kWrite>
__global__ void __launch_bounds__(256)
k_ids_find(const E* __restrict__ ids, size_t n, unsigned sh, size_t nvec, unsigned iters, E value,
           unsigned long long base, const unsigned long long* __restrict__ blk_off,
           unsigned long long* __restrict__ blk_cnt, unsigned long long* __restrict__ out, unsigned long long cap,
           unsigned* __restrict__ wide) {
    constexpr unsigned V = 16 / sizeof(E);
    __shared__ unsigned wtot[4];
    const size_t v0 = (size_t)blockIdx.x * iters * 256;
    unsigned long long running = kWrite ? blk_off[blockIdx.x] : 0ull;
    unsigned mine = 0;
    for (unsigned it = 0; it < iters; ++it) {
        const size_t j = v0 + (size_t)it * 256 + threadIdx.x;
        unsigned hit = 0;
        if (j < nvec) {
            E v[V];
            const unsigned m = load_ids(ids, n, sh, j, v);
#pragma unroll
            for (unsigned k = 0; k < V; ++k) {
                if ((m >> k & 1u) && v[k] == value) hit |= 1u << k;
                if (sizeof(E) == 8 && (m >> k & 1u) && ((unsigned long long)v[k] >> 32) != 0) atomicOr(wide, 1u);
            }
        }
        const unsigned c = (unsigned)__popc(hit);
        if (!kWrite) {
            mine += c;
            continue;
        }
        unsigned total;
        const unsigned before = block_excl_scan(c, wtot, total);
        unsigned long long at = running + before;
        const long long e0 = (long long)(j * V) - (long long)sh;
#pragma unroll
        for (unsigned k = 0; k < V; ++k)
            if (hit >> k & 1u) {
                if (at < cap) out[at] = base + (unsigned long long)(e0 + (long long)k);
                ++at;
            }
        running += total;
    }
    if (!kWrite) {
        unsigned total;
        (void)block_excl_scan(mine, wtot, total);
        if (threadIdx.x == 0) blk_cnt[blockIdx.x] = total;
    }
}

template <class F>
int guarded_ids(F&& f) {
    try {
        f();
        set_error(0, "");
        return BPE_OK;
    } catch (const Error& e) {
        set_error(e.code, e.msg, e.sys_errno);
        return e.code;
    } catch (const std::bad_alloc&) {
        set_error(BPE_E_NOMEM, "host allocation failed");
        return BPE_E_NOMEM;
    }
}

template <class E>
unsigned vec_shift(const void* p) {
    return (unsigned)((reinterpret_cast<uintptr_t>(p) & 15u) / sizeof(E));
}

template <class E>
void hist_launch(const void* d_ids, size_t n, unsigned long long* d_counts, size_t n_counts, unsigned long long flush_ids,
                 unsigned long long* d_bad, hipStream_t s) {
    constexpr size_t V = 16 / sizeof(E);
    const unsigned sh = vec_shift<E>(d_ids);
    const size_t nvec = (n + sh + V - 1) / V;
    int dev = 0, n_cu = 0;
    BPE_HIP(hipGetDevice(&dev));
    BPE_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
    const unsigned grid = (unsigned)std::min<size_t>((nvec + 255) / 256, (size_t)std::max(1, n_cu) * 4);
    hipLaunchKernelGGL(k_ids_hist<E>, dim3(grid), dim3(256), 0, s, static_cast<const E*>(d_ids), n, sh, nvec, d_counts,
                       (unsigned long long)n_counts, flush_ids, d_bad);
    BPE_HIP(hipGetLastError());
}

template <class E, bool kWrite>
void find_launch(const void* d_ids, size_t n, size_t nvec, unsigned iters, unsigned blocks, uint64_t value, uint64_t base,
                 IdScratch& sc, unsigned long long* d_pos, size_t cap, hipStream_t s) {
    hipLaunchKernelGGL((k_ids_find<E, kWrite>), dim3(blocks), dim3(256), 0, s, static_cast<const E*>(d_ids), n,
                       vec_shift<E>(d_ids), nvec, iters, (E)value, (unsigned long long)base, sc.blk_off.p, sc.blk_cnt.p,
                       d_pos, (unsigned long long)cap, reinterpret_cast<unsigned*>(sc.flags.p));
    BPE_HIP(hipGetLastError());
}

void check_ids_arg(const void* d_ids, size_t n, int elem_bytes) {
    BPE_REQUIRE(elem_bytes == 2 || elem_bytes == 4 || elem_bytes == 8, BPE_E_ARG, "ids must be 2, 4 or 8 bytes each");
    BPE_REQUIRE(n == 0 || d_ids, BPE_E_ARG, "NULL ids");
    BPE_REQUIRE((reinterpret_cast<uintptr_t>(d_ids) & (uintptr_t)(elem_bytes - 1)) == 0, BPE_E_ARG,
                "ids are not aligned to their own size");
    BPE_REQUIRE(n < (1ull << 60), BPE_E_LIMIT, "too many ids");
}

}  // namespace

void ids_histogram(const void* d_ids, size_t n, int elem_bytes, unsigned long long* d_counts, size_t n_counts,
                   hipStream_t s, IdScratch& sc) {
    check_ids_arg(d_ids, n, elem_bytes);
    BPE_REQUIRE(n_counts <= (1ull << 32), BPE_E_ARG, "an id table holds at most 2^32 entries");
    if (n == 0) return;
    BPE_REQUIRE(d_counts && n_counts, BPE_E_ARG, "an empty id table");
    // test knob: a small flush bound, so that the flush between steps runs on a small stream
    unsigned long long flush_ids = kHistFlushIds;
    if (const char* e = std::getenv("BPE355_HIST_FLUSH_IDS")) {
        const unsigned long long v = std::strtoull(e, nullptr, 10);
        if (v) flush_ids = std::min(kHistFlushIds, std::max<unsigned long long>(v, 256 * 8));
    }
    sc.flags.reserve(2);
    const unsigned long long none = ~0ull;
    to_device(sc.flags.p, &none, 8, s);
    if (elem_bytes == 2) hist_launch<uint16_t>(d_ids, n, d_counts, n_counts, flush_ids, sc.flags.p, s);
    else if (elem_bytes == 4) hist_launch<uint32_t>(d_ids, n, d_counts, n_counts, flush_ids, sc.flags.p, s);
    else hist_launch<unsigned long long>(d_ids, n, d_counts, n_counts, flush_ids, sc.flags.p, s);
    unsigned long long bad = 0;
    to_host(&bad, sc.flags.p, 8, s);
    if (bad != none) {
        if (elem_bytes == 8 && (bad >> 32) != 0)
            throw Error{BPE_E_ARG, "an int64 id is outside [0, 2^32): " + std::to_string((long long)bad)};
        throw Error{BPE_E_ARG, "id " + std::to_string(bad) + " is outside the table of " + std::to_string(n_counts) +
                                   " counts (the smallest such id)"};
    }
}

size_t ids_find(const void* d_ids, size_t n, int elem_bytes, uint64_t value, uint64_t base, unsigned long long* d_pos,
                size_t cap, hipStream_t s, IdScratch& sc) {
    check_ids_arg(d_ids, n, elem_bytes);
    BPE_REQUIRE(cap == 0 || d_pos, BPE_E_ARG, "NULL positions");
    if (n == 0) return 0;
    const bool fits = elem_bytes == 2 ? value <= 0xFFFFu : value <= 0xFFFFFFFFull;
    if (!fits && elem_bytes != 8) return 0;   // (8-byte ids are still checked for their range)
    const size_t V = 16 / (size_t)elem_bytes;
    const unsigned sh = (unsigned)((reinterpret_cast<uintptr_t>(d_ids) & 15u) / (size_t)elem_bytes);
    const size_t nvec = (n + sh + V - 1) / V;
    // a workgroup takes iters x 256 vectors: 32 KiB of ids, more only where the grid would pass
    // kMaxGridBlocks
    const unsigned iters = (unsigned)std::max<size_t>(8, (nvec + 256 * kMaxGridBlocks - 1) / (256 * kMaxGridBlocks));
    const unsigned blocks = (unsigned)((nvec + (size_t)iters * 256 - 1) / ((size_t)iters * 256));
    sc.blk_cnt.reserve(blocks);
    sc.blk_off.reserve(blocks);
    sc.flags.reserve(2);
    BPE_HIP(hipMemsetAsync(sc.flags.p, 0, 8, s));
    auto run = [&](auto tag_write) {
        constexpr bool kW = decltype(tag_write)::value;
        if (elem_bytes == 2) find_launch<uint16_t, kW>(d_ids, n, nvec, iters, blocks, value, base, sc, d_pos, cap, s);
        else if (elem_bytes == 4) find_launch<uint32_t, kW>(d_ids, n, nvec, iters, blocks, value, base, sc, d_pos, cap, s);
        else find_launch<unsigned long long, kW>(d_ids, n, nvec, iters, blocks, value, base, sc, d_pos, cap, s);
    };
    run(std::false_type{});
    exclusive_sum(sc.blk_cnt.p, sc.blk_off.p, (size_t)blocks, s, &sc.tmp);
    unsigned long long last[2];
    unsigned wide = 0;
    to_host(&last[0], sc.blk_off.p + blocks - 1, 8, s);
    to_host(&last[1], sc.blk_cnt.p + blocks - 1, 8, s);
    to_host(&wide, sc.flags.p, 4, s);
    BPE_REQUIRE(!wide, BPE_E_ARG, "an int64 id is outside [0, 2^32)");
    const size_t total = (size_t)(last[0] + last[1]);
    if (total && cap) {
        run(std::true_type{});
        BPE_HIP(hipStreamSynchronize(s));
    }
    return total;
}

}  // namespace bpe

extern "C" {

int bpe_ids_histogram_device(const void* d_ids, size_t n, int elem_bytes, uint64_t* d_counts, size_t n_counts,
                             void* hip_stream) {
    return bpe::guarded_ids([&] {
        bpe::IdScratch sc;
        bpe::ids_histogram(d_ids, n, elem_bytes, reinterpret_cast<unsigned long long*>(d_counts), n_counts,
                           (hipStream_t)hip_stream, sc);
    });
}

int bpe_ids_find_device(const void* d_ids, size_t n, int elem_bytes, uint64_t value, uint64_t base, uint64_t* d_pos_out,
                        size_t cap, size_t* n_out, void* hip_stream) {
    return bpe::guarded_ids([&] {
        BPE_REQUIRE(n_out, BPE_E_ARG, "NULL argument");
        *n_out = 0;
        bpe::IdScratch sc;
        *n_out = bpe::ids_find(d_ids, n, elem_bytes, value, base, reinterpret_cast<unsigned long long*>(d_pos_out), cap,
                               (hipStream_t)hip_stream, sc);
    });
}

// How many of the last n raw bytes of a read range cannot be decoded yet: the longest suffix that
// is a proper prefix of a well-formed UTF-8 sequence (the table of text.hip's validate_unit), else
// a final \r, which may be the first half of \r\n.  Nothing waits at the end of a file.
size_t bpe_window_holdback(const uint8_t* tail, size_t n, int at_eof) {
    if (!tail || n == 0 || at_eof) return 0;
    if (n > 4) {
        tail += n - 4;
        n = 4;
    }
    for (size_t k = std::min<size_t>(n, 3); k >= 1; --k) {
        const uint8_t* p = tail + n - k;
        const unsigned b0 = p[0];
        unsigned need, lo = 0x80, hi = 0xBF;
        if (b0 >= 0xC2 && b0 <= 0xDF) need = 2;
        else if (b0 == 0xE0) { need = 3; lo = 0xA0; }
        else if (b0 >= 0xE1 && b0 <= 0xEF) { need = 3; if (b0 == 0xED) hi = 0x9F; }
        else if (b0 == 0xF0) { need = 4; lo = 0x90; }
        else if (b0 >= 0xF1 && b0 <= 0xF3) need = 4;
        else if (b0 == 0xF4) { need = 4; hi = 0x8F; }
        else continue;
        if (k >= need) continue;
        if (k >= 2 && (p[1] < lo || p[1] > hi)) continue;
        if (k >= 3 && (p[2] & 0xC0) != 0x80) continue;
        return k;
    }
    return tail[n - 1] == 0x0D ? 1 : 0;
}

}  // extern "C"
