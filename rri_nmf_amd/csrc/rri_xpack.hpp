// rri_xpack.hpp -- the lossless 28-bit copy of an fp32 X that the read-only pass streams.
//
// The top byte of an fp32 (sign and exponent bits 7..1) of non-negative data of ordinary dynamic range takes about a dozen
// values, so an element is kept as its low three bytes and a 4-bit code of the top byte: 3.5 bytes instead of 4, every bit of
// every value kept.  With fp32 bits b:   lo = b & 0xffffff,  hi = b >> 24;
//     code = 15         if hi == 0                   (zeros, denormals, values below 2^-125)
//     code = hi - base  if base <= hi <= base + 14
//     anything else is OUT OF WINDOW (negatives, Inf and NaN included): the tile is flagged and read as fp32.
// base = max(1, hmax - 14), hmax = the largest hi in [1, 0x7e] present in X.
//
// Layout: the copy is indexed by absolute (8-row chunk q = row / 8, 256-column wave panel p); each (q, p) is one record of
// seven wave-wide slots of 16 bytes per lane (7 KiB), so that every load of the pass is the 1 KiB coalesced 16-byte-per-lane
// load of the fp32 loop, seven per chunk instead of eight.  Slots 0..5 hold the lane's 8 rows x 4 columns of lo as a 96-byte
// stream (element (u, e) at byte 3 (4 u + e) of the stream; stream byte s in slot s / 16, byte s % 16), slot 6 their 32
// codes (code (u, e) in bits 4 e .. 4 e + 3 of halfword u).
//
// Plain inline functions, host and device: the stand-alone CPU test compiles this header with the host compiler.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RRI_XPACK_FN __host__ __device__ inline
#else
#define RRI_XPACK_FN inline
#endif

namespace rri {
namespace xpack {

enum : unsigned {
    LANES = 64,             // lanes of a wave = 4-column groups of a panel
    ROWS = 8,               // rows of a chunk
    COLS = 4,               // columns of a lane
    SLOTS = 7,              // 16-byte-per-lane slots of a record
    CODE_SLOT = 6,
    SLOT_BYTES = LANES * 16,
    RECORD_BYTES = SLOTS * SLOT_BYTES,
    LO_DWORDS = 24,         // dwords of a lane's lo stream (slots 0..5)
    CODE_ZERO = 15,
    WINDOW = 15,            // top bytes base .. base + 14
    HI_MAX = 0x7e           // the largest top byte a window may hold (0x7f: Inf, NaN and values from 2^127)
};

// the top byte as the max-reduction counts it: itself in [1, HI_MAX], otherwise 0
RRI_XPACK_FN uint32_t window_candidate(uint32_t bits) {
    const uint32_t hi = bits >> 24;
    return hi <= HI_MAX ? hi : 0u;
}
RRI_XPACK_FN uint32_t base_of(uint32_t hmax) { return hmax > WINDOW ? hmax - (WINDOW - 1) : 1u; }

RRI_XPACK_FN bool in_window(uint32_t bits, uint32_t base) {
    const uint32_t hi = bits >> 24;
    return hi == 0u || (hi >= base && hi <= base + (WINDOW - 1));
}
// the code of an element in the window (an element outside it gets the code of zero: its tile is flagged and never decoded)
RRI_XPACK_FN uint32_t encode_code(uint32_t bits, uint32_t base) {
    const uint32_t hi = bits >> 24;
    return (hi != 0u && in_window(bits, base)) ? hi - base : (uint32_t)CODE_ZERO;
}
RRI_XPACK_FN uint32_t decode(uint32_t lo, uint32_t code, uint32_t base) {
    const uint32_t hi = code == CODE_ZERO ? 0u : base + code;
    return hi << 24 | lo;
}

// ---- where things are ---------------------------------------------------------------------------------------------------------
// byte offset of record (q, p) in the copy; panels = wave panels of the copy (4 per workgroup of the pass, adjacent)
RRI_XPACK_FN uint64_t record_offset(uint64_t q, uint64_t p, uint64_t panels) { return (q * panels + p) * RECORD_BYTES; }
// byte offset, inside its record, of lane `lane`'s 16 bytes of slot `slot`
RRI_XPACK_FN uint32_t slot_offset(uint32_t slot, uint32_t lane) { return slot * SLOT_BYTES + lane * 16u; }
// byte offset, inside its record, of byte j (0..2) of the lo of element (u, e) of lane `lane`
RRI_XPACK_FN uint32_t lo_byte_offset(uint32_t lane, uint32_t u, uint32_t e, uint32_t j) {
    const uint32_t s = 3u * (COLS * u + e) + j;
    return slot_offset(s / 16u, lane) + s % 16u;
}
// byte offset inside its record of the byte that holds the code of element (u, e), and the code's shift inside that byte
RRI_XPACK_FN uint32_t code_byte_offset(uint32_t lane, uint32_t u, uint32_t e) { return slot_offset(CODE_SLOT, lane) + 2u * u + e / 2u; }
RRI_XPACK_FN uint32_t code_shift(uint32_t e) { return 4u * (e & 1u); }

// ---- a lane's 8 x 4 elements <-> its 28 dwords (slot-major: dword 4 s + i = dword i of the lane's 16 bytes of slot s) ---------
// One row of 4 elements takes three dwords of the lo stream and one halfword of codes.
RRI_XPACK_FN void encode_lane(const uint32_t (&bits)[ROWS][COLS], uint32_t base, uint32_t (&out)[4 * SLOTS], bool& flagged) {
    bool bad = false;
    for (int u = 0; u < (int)ROWS; ++u) {
        uint32_t lo[COLS], codes = 0u;
        for (int e = 0; e < (int)COLS; ++e) {
            bad = bad || !in_window(bits[u][e], base);
            lo[e] = bits[u][e] & 0xffffffu;
            codes |= encode_code(bits[u][e], base) << (4 * e);
        }
        out[3 * u] = lo[0] | lo[1] << 24;
        out[3 * u + 1] = lo[1] >> 8 | lo[2] << 16;
        out[3 * u + 2] = lo[2] >> 16 | lo[3] << 8;
        const int cw = 4 * (int)CODE_SLOT + u / 2;
        if (u % 2 == 0) out[cw] = codes;
        else out[cw] |= codes << 16;
    }
    flagged = bad;
}

// the four top bytes of a row from its halfword of codes, one per byte, SWAR: spread the nibbles over the bytes, add the base to
// all four at once (base + 15 <= 127: no carry leaves a byte), clear the bytes whose code is 15
RRI_XPACK_FN uint32_t decode_tops(uint32_t codes16, uint32_t base4) {
    uint32_t x = (codes16 | codes16 << 8) & 0x00ff00ffu;
    x = (x | x << 4) & 0x0f0f0f0fu;
    const uint32_t is15 = ((x + 0x01010101u) >> 4) & 0x01010101u;
    return (x + base4) & ~((is15 << 8) - is15);
}
// row u of a lane: its four fp32 bit patterns from the lane's 28 dwords; base4 = base * 0x01010101.  With u a compile-time
// constant every index and shift below is one too (funnel shifts and byte selects)
RRI_XPACK_FN void decode_row(const uint32_t (&in)[4 * SLOTS], int u, uint32_t base4, uint32_t (&bits)[COLS]) {
    const uint32_t a = in[3 * u], b = in[3 * u + 1], c = in[3 * u + 2];
    const uint32_t cw = in[4 * (int)CODE_SLOT + u / 2];
    const uint32_t tops = decode_tops(u % 2 ? cw >> 16 : cw & 0xffffu, base4);
    bits[0] = (a & 0x00ffffffu) | (tops << 24);
    bits[1] = ((a >> 24 | b << 8) & 0x00ffffffu) | (tops << 16 & 0xff000000u);
    bits[2] = ((b >> 16 | c << 16) & 0x00ffffffu) | (tops << 8 & 0xff000000u);
    bits[3] = c >> 8 | (tops & 0xff000000u);
}

}  // namespace xpack
}  // namespace rri
