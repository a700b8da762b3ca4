// Host evaluation of the byte-parallel token-start predicate (tokstart.h), block by block exactly
// as the device counter evaluates it, for the CPU tests that check it against the serial scanner
// and the oracle (tests/test_tokstart.py); and the word hash of stage.h on the host, for the CPU
// test that ties the counter's constructed inputs to it (tests/test_count_cases.py).  Test support:
// no product path calls either.
#include <cstring>

#include "internal.h"
#include "stage.h"
#include "tokstart.h"

namespace bpe {
namespace hosttab {
#define BPE_UCTAB static const
#include "uniclass_tables.inc"
#undef BPE_UCTAB
struct Tab {
    static unsigned page(unsigned i) { return BPE_UC_PAGE[i]; }
    static unsigned bits(unsigned pg, unsigned i) { return BPE_UC_BITS[pg][i]; }
    static int cls(uint32_t cp) { return uc_class<Tab>(cp); }
};
}  // namespace hosttab
}  // namespace bpe

namespace {
struct HostWin {
    const uint8_t* b;
    uint32_t byte(int j) const { return b[j]; }
    uint32_t dword(int k) const {
        return (uint32_t)b[4 * k] | ((uint32_t)b[4 * k + 1] << 8) | ((uint32_t)b[4 * k + 2] << 16) |
               ((uint32_t)b[4 * k + 3] << 24);
    }
};
}  // namespace

// flags[i] = 1 when a pre-token of text[0..n) begins at byte i (n >= 1: flags[0] = 1)
extern "C" int bpe_pretok_starts_host(const uint8_t* text, size_t n, uint8_t* flags) {
    if ((!text && n) || !flags) return BPE_E_ARG;
    for (size_t o = 0; o < n; o += 64) {
        uint8_t w[bpe::kStartWin];
        for (int j = 0; j < bpe::kStartWin; ++j) {
            const long long p = (long long)o - bpe::kStartPre + j;
            w[j] = p < 0 ? '\n' : (p < (long long)n ? text[p] : 0);
        }
        const long long vhi = (long long)n - ((long long)o - bpe::kStartPre);
        uint64_t m = bpe::token_starts64<bpe::hosttab::Tab>(HostWin{w}, (int)(vhi > bpe::kStartWin ? bpe::kStartWin : vhi));
        if (o == 0) m |= 1;   // the text start
        for (int k = 0; k < 64 && o + k < n; ++k) flags[o + k] = (uint8_t)((m >> k) & 1);
    }
    return BPE_OK;
}

// out[i] = short_hash of word i of `n` words of `len` bytes each (2..16), laid end to end: the
// packing is pack_word's (byte i of the word is bits 8 i of lo for i < 8, of hi beyond)
extern "C" int bpe_short_hash_host(const uint8_t* words, size_t n, size_t len, uint64_t* out) {
    if ((!words && n) || (!out && n) || len < 2 || len > (size_t)bpe::kInline) return BPE_E_ARG;
    for (size_t w = 0; w < n; ++w) {
        uint64_t lo = 0, hi = 0;
        for (size_t i = 0; i < len; ++i) {
            const uint64_t b = words[w * len + i];
            if (i < 8) lo |= b << (8 * i);
            else hi |= b << (8 * (i - 8));
        }
        out[w] = bpe::short_hash(lo, hi, len);
    }
    return BPE_OK;
}
