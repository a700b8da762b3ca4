// The UTF-8 repair: bytes(in).decode("utf-8", errors).encode("utf-8") for errors = "replace" and
// "ignore", byte-parallel, with an output whose length differs from the input's.
//
// The rule (CPython's decoder: one U+FFFD per maximal subpart of an ill-formed subsequence) is
// local.  A byte that is not 10xxxxxx starts a unit: itself plus the following bytes for as long
// as each lies in the range its lead allows at that place (utf8_len_valid's table), up to the
// needed length or the end of the text.  A complete unit is well formed and is copied; an
// incomplete one, and a lead 80..C1 or F5..FF (length 1), is ill formed: its first byte becomes
// EF BF BD (replace) or nothing (ignore), its other bytes nothing.  A continuation byte belongs to
// the unit of the nearest non-continuation byte within 3 positions before it when that unit
// reaches it; otherwise it is a stray, an ill-formed unit of its own.  So what position i emits is
// decided by s[i - 3 .. i + 3] and the end of the text alone.
//
// Three launches.  k_fix_count: a thread classifies the 16 bytes of one aligned load, with the 4
// bytes on either side taken from the neighbouring lanes, and a workgroup sums the output bytes of
// its 4 KiB tile.  A rocPRIM exclusive scan of the 64-bit tile totals gives every tile's place in
// the output and the output's size, before anything is written.  k_fix_write classifies again,
// places each lane's bytes with a wave prefix, stages the tile's output in LDS and stores it as
// aligned 16-byte vectors; a tile without a byte of an ill-formed unit is copied as it is.

#include "prims.h"
#include "utf8fix.h"

namespace bpe {

namespace {

// the unit of a thread: its 16 bytes as four words (bytes past the text read 0), the 4 bytes
// before (prev) and after (next) them.  Every lane of the wave calls it (the neighbours come from
// lanes lane - 1 and lane + 1; a wave's edge lanes read theirs from memory, byte by byte).
__device__ __forceinline__ void load_unit_halo(const uint8_t* __restrict__ s, size_t n, size_t lo, bool aligned,
                                               uint32_t w[4], uint32_t& prev, uint32_t& next) {
    w[0] = w[1] = w[2] = w[3] = 0;
    if (aligned && lo + kFixUnit <= n) {
        const uint4 v = *reinterpret_cast<const uint4*>(s + lo);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else if (lo < n) {   // an unaligned text, or the text's last unit
#pragma unroll
        for (int k = 0; k < kFixUnit; ++k)
            if (lo + k < n) w[k >> 2] |= (uint32_t)s[lo + k] << (8 * (k & 3));
    }
    const int lane = threadIdx.x & 63;
    prev = __shfl_up(w[3], 1);
    next = __shfl_down(w[0], 1);
    const uint32_t hi_bits = (w[0] | w[1] | w[2] | w[3]) & 0x80808080u;
    if (hi_bits && lane == 0) {
        prev = 0;
        for (int k = 0; k < 4; ++k)
            if (lo + k >= 4) prev |= (uint32_t)s[lo + k - 4] << (8 * k);
    }
    if (hi_bits && lane == 63) {
        next = 0;
        for (int k = 0; k < 4; ++k)
            if (lo + kFixUnit + k < n) next |= (uint32_t)s[lo + kFixUnit + k] << (8 * k);
    }
}

// stat[0] += ill-formed units, stat[1] += their bytes, stat[2] = min(their first positions)
__global__ void __launch_bounds__(kFixThreads) k_fix_count(const uint8_t* __restrict__ s, size_t n, size_t n_tiles, int mode,
                                                           unsigned long long* __restrict__ tile_sum,
                                                           unsigned* __restrict__ tile_dirty,
                                                           unsigned long long* __restrict__ stat) {
    __shared__ unsigned s_out[4], s_units[4], s_bytes[4];
    __shared__ unsigned long long s_first[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool aligned = ((uintptr_t)s & 15u) == 0;
    for (size_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const size_t lo = tile * kFixTile + (size_t)tid * kFixUnit;
        uint32_t w[4], prev, next, bad, start;
        load_unit_halo(s, n, lo, aligned, w, prev, next);
        classify_unit(w, prev, next, lo, n, bad, start);
        const uint32_t valid = valid_mask(lo, n);
        unsigned out = (unsigned)__popc(valid & ~bad) + (mode == 1 ? 3u * (unsigned)__popc(start) : 0u);
        unsigned units = (unsigned)__popc(start), bytes = (unsigned)__popc(bad);
        unsigned long long first = start ? (unsigned long long)lo + (unsigned)(__ffs((int)start) - 1) : ~0ULL;
        out = wave_sum(out);
        units = wave_sum(units);
        bytes = wave_sum(bytes);
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long f = __shfl_xor(first, o);
            first = f < first ? f : first;
        }
        if (lane == 0) { s_out[wave] = out; s_units[wave] = units; s_bytes[wave] = bytes; s_first[wave] = first; }
        __syncthreads();
        if (tid == 0) {
            const unsigned u = s_units[0] + s_units[1] + s_units[2] + s_units[3];
            const unsigned by = s_bytes[0] + s_bytes[1] + s_bytes[2] + s_bytes[3];
            tile_sum[tile] = (unsigned long long)s_out[0] + s_out[1] + s_out[2] + s_out[3];
            tile_dirty[tile] = by != 0;   // (a tile may hold the tail of a unit that starts before it)
            if (u) {
                unsigned long long f = s_first[0];
                for (int k = 1; k < 4; ++k) f = s_first[k] < f ? s_first[k] : f;
                atomicAdd(stat, (unsigned long long)u);
                atomicMin(stat + 2, f);
            }
            if (by) atomicAdd(stat + 1, (unsigned long long)by);
        }
        __syncthreads();
    }
}

constexpr int kStageWords = 3 * kFixTile / 4 + 8;   // a tile of all ill-formed bytes grows 3x

// stage[0, total) -> dst: the 16-byte vectors of dst that the bytes fill whole are stored whole,
// each put together from the staged words at its byte shift; the ragged ends go byte by byte
__device__ __forceinline__ void flush_stage(const uint32_t* stage, unsigned total, uint8_t* __restrict__ dst) {
    const unsigned shift = (unsigned)((uintptr_t)dst & 15u);
    const unsigned n_vec = (shift + total + 15u) / 16u;
    const uint8_t* stage8 = reinterpret_cast<const uint8_t*>(stage);
    for (unsigned c = threadIdx.x; c < n_vec; c += kFixThreads) {
        const int k0 = (int)(16u * c) - (int)shift;   // the staged byte that lands on the vector's first byte
        if (k0 >= 0 && (unsigned)k0 + 16u <= total) {
            const unsigned i = (unsigned)k0 >> 2, r = 8u * ((unsigned)k0 & 3u);
            uint32_t v[5];
#pragma unroll
            for (int j = 0; j < 5; ++j) v[j] = stage[i + j];
            uint4 o;
            o.x = (uint32_t)((((uint64_t)v[1] << 32) | v[0]) >> r);
            o.y = (uint32_t)((((uint64_t)v[2] << 32) | v[1]) >> r);
            o.z = (uint32_t)((((uint64_t)v[3] << 32) | v[2]) >> r);
            o.w = (uint32_t)((((uint64_t)v[4] << 32) | v[3]) >> r);
            *reinterpret_cast<uint4*>(dst + k0) = o;
        } else {
            for (int j = 0; j < 16; ++j) {
                const int k = k0 + j;
                if (k >= 0 && (unsigned)k < total) dst[k] = stage8[k];
            }
        }
    }
}

__global__ void __launch_bounds__(kFixThreads) k_fix_write(const uint8_t* __restrict__ s, size_t n, size_t n_tiles, int mode,
                                                           const unsigned long long* __restrict__ tile_off,
                                                           const unsigned* __restrict__ tile_dirty,
                                                           uint8_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint32_t stage[kStageWords];
    __shared__ unsigned s_wave[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool aligned = ((uintptr_t)s & 15u) == 0;
    uint8_t* const stage8 = reinterpret_cast<uint8_t*>(stage);
    for (size_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const size_t base = tile * kFixTile, lo = base + (size_t)tid * kFixUnit;
        uint32_t w[4], prev, next;
        load_unit_halo(s, n, lo, aligned, w, prev, next);
        unsigned total;
        if (!tile_dirty[tile]) {   // (the same for the whole workgroup) a plain copy
            uint4 v;
            v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
            *reinterpret_cast<uint4*>(stage + 4 * tid) = v;
            total = n - base < (size_t)kFixTile ? (unsigned)(n - base) : (unsigned)kFixTile;
        } else {
            uint32_t bad, start;
            classify_unit(w, prev, next, lo, n, bad, start);
            const uint32_t valid = valid_mask(lo, n);
            const unsigned cnt = (unsigned)__popc(valid & ~bad) + (mode == 1 ? 3u * (unsigned)__popc(start) : 0u);
            unsigned incl = cnt;   // the wave's inclusive prefix
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned t = __shfl_up(incl, o);
                if (lane >= o) incl += t;
            }
            if (lane == 63) s_wave[wave] = incl;
            __syncthreads();
            unsigned at = incl - cnt;
            for (int k = 0; k < wave; ++k) at += s_wave[k];
            total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
#pragma unroll
            for (int k = 0; k < kFixUnit; ++k) {
                const uint32_t bit = 1u << k;
                if (!(valid & bit)) continue;
                if (!(bad & bit)) {
                    stage8[at++] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
                } else if ((start & bit) && mode == 1) {   // U+FFFD
                    stage8[at] = 0xEF;
                    stage8[at + 1] = 0xBF;
                    stage8[at + 2] = 0xBD;
                    at += 3;
                }
            }
        }
        __syncthreads();
        flush_stage(stage, total, out + tile_off[tile]);
        __syncthreads();   // the stage and s_wave are free for the next tile
    }
}

}  // namespace

void RepairPlan::plan(const uint8_t* d_in, size_t n_in, int errors_mode, hipStream_t stream) {
    BPE_REQUIRE(errors_mode == 1 || errors_mode == 2, BPE_E_ARG, "errors mode must be 1 (replace) or 2 (ignore)");
    in = d_in;
    n = n_in;
    mode = errors_mode;
    n_out = 0;
    stats = bpe_utf8_stats{0, 0, ~0ULL};
    n_tiles = (n + kFixTile - 1) / kFixTile;
    if (n == 0) return;
    sum.reserve(n_tiles + 1);
    off.reserve(n_tiles + 1 + 3);
    dirty.reserve(n_tiles);
    unsigned long long* const stat = off.p + n_tiles + 1;
    BPE_HIP(hipMemsetAsync(sum.p + n_tiles, 0, 8, stream));
    BPE_HIP(hipMemsetAsync(stat, 0, 16, stream));
    BPE_HIP(hipMemsetAsync(stat + 2, 0xFF, 8, stream));
    const unsigned grid = (unsigned)std::min<size_t>(n_tiles, 4096);
    hipLaunchKernelGGL(k_fix_count, dim3(grid), dim3(kFixThreads), 0, stream, d_in, n, n_tiles, mode, sum.p, dirty.p,
                       stat);
    BPE_HIP(hipGetLastError());
    exclusive_sum(sum.p, off.p, n_tiles + 1, stream);
    unsigned long long h[4];   // the output size, then the stats
    to_host(h, off.p + n_tiles, sizeof(h), stream);
    n_out = (size_t)h[0];
    stats = bpe_utf8_stats{h[1], h[2], h[3]};
}

void RepairPlan::write(uint8_t* d_out, hipStream_t stream) const {
    if (n == 0) return;
    const unsigned grid = (unsigned)std::min<size_t>(n_tiles, 4096);
    hipLaunchKernelGGL(k_fix_write, dim3(grid), dim3(kFixThreads), 0, stream, in, n, n_tiles, mode, off.p, dirty.p,
                       d_out);
    BPE_HIP(hipGetLastError());
}

const uint8_t* repair_text(const uint8_t* d_in, size_t n, int mode, DevBuf<uint8_t>& out, size_t* n_out,
                           bpe_utf8_stats* stats, hipStream_t stream) {
    RepairPlan P;
    P.plan(d_in, n, mode, stream);
    out.reserve(std::max<size_t>(P.n_out, 1));
    P.write(out.p, stream);
    BPE_HIP(hipStreamSynchronize(stream));   // the plan's arrays go with P
    *n_out = P.n_out;
    if (stats) *stats = P.stats;
    return out.p;
}

namespace {
template <class F>
int guarded_fix(F&& f) {
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
}  // namespace

}  // namespace bpe

extern "C" {

int bpe_utf8_repair_geometry(size_t* unit_bytes, size_t* tile_bytes) {
    if (unit_bytes) *unit_bytes = bpe::kFixUnit;
    if (tile_bytes) *tile_bytes = bpe::kFixTile;
    return BPE_OK;
}

int bpe_utf8_repair_device(const uint8_t* d_in, size_t n, int mode, uint8_t* d_out, size_t cap, size_t* n_out,
                           bpe_utf8_stats* stats, void* hip_stream) {
    return bpe::guarded_fix([&] {
        BPE_REQUIRE(n_out && (n == 0 || d_in), BPE_E_ARG, "NULL argument");
        BPE_REQUIRE(mode == 1 || mode == 2, BPE_E_ARG, "mode must be 1 (replace) or 2 (ignore)");
        *n_out = 0;
        if (stats) *stats = bpe_utf8_stats{0, 0, ~0ULL};
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
            throw bpe::Error{BPE_E_HIP, "no HIP device visible (libbpe355 needs an MI355X / gfx950 GPU)"};
        if (n == 0) return;
        const hipStream_t s = (hipStream_t)hip_stream;
        bpe::RepairPlan P;
        P.plan(d_in, n, mode, s);
        *n_out = P.n_out;
        if (stats) *stats = P.stats;
        if (!d_out) return;   // size query
        BPE_REQUIRE(cap >= P.n_out, BPE_E_ARG, "d_out holds " + std::to_string(cap) + " bytes, the repaired text has " +
                                                   std::to_string(P.n_out));
        P.write(d_out, s);
        BPE_HIP(hipStreamSynchronize(s));
    });
}

int bpe_text_prepare_device_ex(const uint8_t* d_in, size_t n, int mode, uint8_t* d_out, size_t cap, size_t* n_out,
                               bpe_utf8_stats* stats, void* hip_stream) {
    if (mode == 0) {   // strict: the call as it always was
        if (stats) *stats = bpe_utf8_stats{0, 0, ~0ULL};
        if (d_out && cap < n) {
            bpe::set_error(BPE_E_ARG, "d_out must hold the input's bytes");
            return BPE_E_ARG;
        }
        return bpe_text_prepare_device(d_in, n, d_out, n_out, hip_stream);
    }
    return bpe::guarded_fix([&] {
        BPE_REQUIRE(n_out && (n == 0 || d_in), BPE_E_ARG, "NULL argument");
        BPE_REQUIRE(mode == 1 || mode == 2, BPE_E_ARG, "mode must be 0 (strict), 1 (replace) or 2 (ignore)");
        *n_out = 0;
        if (stats) *stats = bpe_utf8_stats{0, 0, ~0ULL};
        if (n == 0) return;
        const hipStream_t s = (hipStream_t)hip_stream;
        bpe::RepairPlan P;
        P.plan(d_in, n, mode, s);
        if (stats) *stats = P.stats;
        if (!d_out) {   // size query: the repaired length (the newline translation only shrinks it)
            *n_out = P.n_out;
            return;
        }
        BPE_REQUIRE(cap >= P.n_out, BPE_E_ARG, "d_out holds " + std::to_string(cap) + " bytes, the repaired text has " +
                                                   std::to_string(P.n_out));
        const uint8_t* text = d_in;
        size_t tn = n;
        bpe::DevBuf<uint8_t> fixed;
        if (P.stats.n_units) {
            fixed.alloc(std::max<size_t>(P.n_out, 1));
            P.write(fixed.p, s);
            text = fixed.p;
            tn = P.n_out;
        }
        bpe::DevBuf<uint8_t> scratch;
        size_t m = 0;
        const uint8_t* p = tn ? bpe::prepare_text(text, tn, scratch, &m, s) : text;
        if (p != d_out && m) BPE_HIP(hipMemcpyAsync(d_out, p, m, hipMemcpyDeviceToDevice, s));
        BPE_HIP(hipStreamSynchronize(s));
        *n_out = m;
    });
}

}  // extern "C"
