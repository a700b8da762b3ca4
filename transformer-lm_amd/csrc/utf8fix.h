// The UTF-8 repair (utf8fix.hip): bytes(in).decode("utf-8", errors).encode("utf-8") on the device
// for errors = "replace" (mode 1) and "ignore" (mode 2), as CPython defines them.
#pragma once

#include "internal.h"

namespace bpe {

constexpr int kFixUnit = 16;                       // bytes a thread classifies (one 16-byte load)
constexpr int kFixThreads = 256;
constexpr int kFixTile = kFixUnit * kFixThreads;   // bytes a workgroup repairs per step

// ------------------------------------------------------------------ the rule, per 16-byte unit
// (host and device: the kernels classify with it, and so can a host-side check)
// bit k of bad: byte lo + k belongs to an ill-formed unit; of start: it is that unit's first byte
__host__ __device__ inline void classify_unit(const uint32_t w[4], uint32_t prev, uint32_t next, size_t lo, size_t n,
                                              uint32_t& bad, uint32_t& start) {
    bad = start = 0;
    if (!((w[0] | w[1] | w[2] | w[3]) & 0x80808080u)) return;   // all ASCII
    // window b[0..24): 4 bytes before the unit, its 16, 4 after; b[x] is text byte lo + x - 4
    uint8_t b[24];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        b[k] = (uint8_t)(prev >> (8 * k));
        b[20 + k] = (uint8_t)(next >> (8 * k));
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) b[4 + k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
    auto exists = [&](int x) -> bool { return lo + (size_t)x >= 4 && lo + (size_t)x < n + 4; };
    // the units that start at window positions 1..19: length (0: no unit starts there), complete
    uint32_t ulen[20];
    uint32_t complete = 0;
#pragma unroll
    for (int x = 1; x < 20; ++x) {
        const uint32_t b0 = b[x];
        ulen[x] = 0;
        if (!exists(x) || (b0 & 0xC0u) == 0x80u) continue;
        uint32_t need = 0, lo8 = 0x80, hi8 = 0xBF;
        if (b0 < 0x80u) need = 1;
        else if (b0 >= 0xC2u && b0 <= 0xDFu) need = 2;
        else if (b0 == 0xE0u) { need = 3; lo8 = 0xA0; }
        else if (b0 >= 0xE1u && b0 <= 0xECu) need = 3;
        else if (b0 == 0xEDu) { need = 3; hi8 = 0x9F; }
        else if (b0 >= 0xEEu && b0 <= 0xEFu) need = 3;
        else if (b0 == 0xF0u) { need = 4; lo8 = 0x90; }
        else if (b0 >= 0xF1u && b0 <= 0xF3u) need = 4;
        else if (b0 == 0xF4u) { need = 4; hi8 = 0x8F; }
        uint32_t len = 1;
        if (need >= 2 && exists(x + 1) && b[x + 1] >= lo8 && b[x + 1] <= hi8) {
            len = 2;
            if (need >= 3 && exists(x + 2) && (b[x + 2] & 0xC0u) == 0x80u) {
                len = 3;
                if (need == 4 && exists(x + 3) && (b[x + 3] & 0xC0u) == 0x80u) len = 4;
            }
        }
        ulen[x] = len;
        if (len == need) complete |= 1u << x;
    }
#pragma unroll
    for (int k = 0; k < kFixUnit; ++k) {
        const int x = 4 + k;
        const uint32_t c = b[x];
        if (lo + (size_t)k >= n || c < 0x80u) continue;
        const uint32_t bit = 1u << k;
        if ((c & 0xC0u) != 0x80u) {
            if (!((complete >> x) & 1u)) { bad |= bit; start |= bit; }
            continue;
        }
        bool found = false;
#pragma unroll
        for (int d = 1; d <= 3; ++d) {
            if (found || ulen[x - d] == 0) continue;
            found = true;
            if ((uint32_t)d < ulen[x - d]) {                    // inside that unit
                if (!((complete >> (x - d)) & 1u)) bad |= bit;
            } else {                                            // past it: a stray
                bad |= bit;
                start |= bit;
            }
        }
        if (!found) { bad |= bit; start |= bit; }
    }
}

__host__ __device__ inline uint32_t valid_mask(size_t lo, size_t n) {
    if (lo >= n) return 0;
    return n - lo >= (size_t)kFixUnit ? 0xFFFFu : (1u << (unsigned)(n - lo)) - 1u;
}

// The first two launches of a repair: the classification with the per-tile output sizes, and
// their scan.  After plan() the output size and the stats are known on the host and nothing has
// been written; write() is the third launch, into a buffer of at least n_out bytes.
struct RepairPlan {
    const uint8_t* in = nullptr;
    size_t n = 0, n_out = 0, n_tiles = 0;
    int mode = 0;
    bpe_utf8_stats stats{0, 0, ~0ULL};
    DevBuf<unsigned long long> sum;   // per tile: output bytes (n_tiles + 1 entries, the last 0)
    DevBuf<unsigned long long> off;   // their exclusive sums (n_tiles + 1), then the 3 stats words
    DevBuf<unsigned> dirty;           // per tile: it holds a byte of an ill-formed unit
    void plan(const uint8_t* d_in, size_t n_in, int errors_mode, hipStream_t stream);   // returns with n_out, stats set
    void write(uint8_t* d_out, hipStream_t stream) const;                               // enqueues only
};

// d_in repaired into `out` (grown to fit); returns out.p, *n_out its length.  Returns once the
// text is written.
const uint8_t* repair_text(const uint8_t* d_in, size_t n, int mode, DevBuf<uint8_t>& out, size_t* n_out,
                           bpe_utf8_stats* stats, hipStream_t stream);

// a += b for the reports of several windows; b's first position is relative to `offset`
inline void utf8_stats_add(bpe_utf8_stats& a, const bpe_utf8_stats& b, uint64_t offset) {
    if (a.first == ~0ULL && b.first != ~0ULL) a.first = b.first + offset;
    a.n_units += b.n_units;
    a.n_bytes += b.n_bytes;
}

}  // namespace bpe
