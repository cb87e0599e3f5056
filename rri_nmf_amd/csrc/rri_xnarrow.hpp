// rri_xnarrow.hpp -- the lossless 26-bit copy of an fp32 X that the read-only pass streams.
//
// The 28-bit copy (rri_xpack.hpp) spends 4 bits on the top byte of an element.  The exponent byte (bits 30..23; the sign of
// every element of the copy is 0) carries about 2.2 bits on term-weight data, and its seven most frequent values hold 98 % of the
// elements.  So an element is kept as its 23 mantissa bits and a 3-bit code:
//     code 0..6: the exponent byte is book[code], the seven most frequent exponent bytes of X (the BOOK);
//     code 7   : the exponent byte comes from the record's EXCEPTION list.
// The window, its base and the tile flags are those of rri_xpack.hpp, unchanged: a tile with an element outside the window is
// flagged and read as fp32.  The window holds at most 32 exponent bytes (0 and 1 for top byte 0, and two for each of its fifteen
// top bytes); the book and the RARE book (up to 32 values) are chosen among exactly those, so every element inside the window is
// in one of the two and this format flags no tile that the 28-bit one does not.
//
// Layout: the record grid of rri_xpack.hpp -- (8-row chunk q, 256-column wave panel p), the lane's 8 rows x 4 columns in the
// order the row loop consumes them (element i = 4 u + e).  The FIXED PART of a record is 26 dwords per lane, 6.5 KiB: six
// wave-wide slots of 16 bytes per lane and one of 8.  Dwords 0..22 are the lane's 32 mantissas as one bit stream (element i at
// bits 23 i .. 23 i + 22), dwords 23..25 (C0, C1, C2) the 32 codes, laid out so that the four codes of a row come out as the
// four byte selectors of ONE byte-permute of the book:
//     rows 0..5: code (u, e) in bits 3 (u % 2) .. + 2 of byte e of C[u / 2];
//     row 6    : its low two bits in bits 6..7 of byte e of C0, its bit 2 in bit 6 of byte e of C2;
//     row 7    : its low two bits in bits 6..7 of byte e of C1, its bit 2 in bit 7 of byte e of C2.
// The EXCEPTIONS of a record are 16-bit entries, position (lane * 32 + i) in bits 0..10 and the index into the rare book in bits
// 11..15, ordered by position; a DIRECTORY of one 32-bit offset per record and one more (the prefix sum of the counts) says where
// a record's entries are.  Rows past n and lanes past the last column are padding: code 0, mantissa 0, never an exception; no sum
// the pass keeps takes them.
//
// Plain inline functions, host and device: the stand-alone CPU test compiles this header with the host compiler.
#pragma once
#include <stdint.h>

#include "rri_xpack.hpp"

namespace rri {
namespace xnarrow {

enum : unsigned {
    LANES = xpack::LANES,
    ROWS = xpack::ROWS,
    COLS = xpack::COLS,
    ELEMS = ROWS * COLS,            // elements of a lane
    MANT_BITS = 23,
    MANT_DWORDS = 23,               // 32 x 23 bits
    CODE_DWORD = 23,                // C0; C1, C2 follow
    LANE_DWORDS = 26,
    WIDE_SLOTS = 6,                 // 16 bytes per lane; then one slot of 8
    RECORD_BYTES = LANE_DWORDS * 4 * LANES,     // 6.5 KiB
    BOOK = 7,
    CODE_EXC = 7,
    RARE_MAX = 32,
    POS_BITS = 11,
    CLS_NONE = 0xff,                // class of an exponent byte in neither book
    CLS_RARE = 8                    // class of rare-book entry j: CLS_RARE + j; class of book entry c: c
};
constexpr uint64_t DIR_MAX = 0xffffff00ull;     // the most exception entries a copy may hold

// the book (exponent byte c in byte c of hi:lo, byte 7 zero) and the rare book (entry j in byte j % 4 of rare[j / 4])
struct Books {
    uint32_t lo, hi;
    uint32_t rare[RARE_MAX / 4];
};

// the byte-permute of gfx9 (v_perm_b32) for the selectors used here: 0..3 a byte of lo, 4..7 a byte of hi, 0x0c the constant 0
RRI_XPACK_FN uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    uint32_t r = 0;
    for (int i = 0; i < 4; ++i) {
        const uint32_t s = sel >> (8 * i) & 0xffu;
        const uint32_t b = s < 4u ? lo >> (8 * s) & 0xffu : s < 8u ? hi >> (8 * (s - 4u)) & 0xffu : 0u;
        r |= b << (8 * i);
    }
    return r;
#endif
}

RRI_XPACK_FN uint32_t book_entry(const Books& b, uint32_t code) { return (code < 4u ? b.lo >> (8u * code) : b.hi >> (8u * (code - 4u))) & 0xffu; }
// entry j of the rare book: four permutes and three selects, no table in memory (once per exception entry, not per element)
RRI_XPACK_FN uint32_t rare_entry(const Books& b, uint32_t j) {
    const uint32_t s = j & 7u, g = j >> 3;
    const uint32_t v0 = perm(b.rare[1], b.rare[0], s), v1 = perm(b.rare[3], b.rare[2], s);
    const uint32_t v2 = perm(b.rare[5], b.rare[4], s), v3 = perm(b.rare[7], b.rare[6], s);
    return (g == 0u ? v0 : g == 1u ? v1 : g == 2u ? v2 : v3) & 0xffu;
}

// ---- the books of an X --------------------------------------------------------------------------------------------------------
// From the 256 counts of the exponent byte (sign 0) and the window's base: the candidates are the exponent bytes of the window,
// ordered by count, larger first, ties to the smaller value; the first seven are the book, the others the rare book (at most 25).
// cls[256]: the class of every exponent byte.  Returns the number of counted elements of the window outside the book: the
// exception entries of the copy.
inline uint64_t choose_books(const uint64_t (&hist)[256], uint32_t base, Books& b, uint8_t (&cls)[256], int& nrare) {
    uint32_t cand[RARE_MAX];
    int nc = 0;
    for (uint32_t e = 0; e < 256u; ++e)
        if (xpack::in_window(e << 23, base)) cand[nc++] = e;      // ascending: at most 2 + 2 * 15
    for (int i = 1; i < nc; ++i)                                  // insertion sort, stable: ties stay ascending
        for (int j = i; j > 0 && hist[cand[j]] > hist[cand[j - 1]]; --j) { const uint32_t t = cand[j]; cand[j] = cand[j - 1]; cand[j - 1] = t; }
    b.lo = b.hi = 0u;
    for (uint32_t& r : b.rare) r = 0u;
    for (int e = 0; e < 256; ++e) cls[e] = (uint8_t)CLS_NONE;
    nrare = 0;
    uint64_t exceptions = 0;
    for (int i = 0; i < nc; ++i) {
        const uint32_t e = cand[i];
        if (i < (int)BOOK) {
            if (i < 4) b.lo |= e << (8 * i); else b.hi |= e << (8 * (i - 4));
            cls[e] = (uint8_t)i;
        } else {
            const int j = i - (int)BOOK;
            b.rare[j / 4] |= e << (8 * (j % 4));
            cls[e] = (uint8_t)(CLS_RARE + j);
            nrare = j + 1;
            exceptions += hist[e];
        }
    }
    return exceptions;
}

// the directory of a copy from the exception counts of its records: dir[r] = counts[0] + .. + counts[r - 1], nrec + 1 entries.
// False when the entries do not fit 32-bit offsets with room for a wave's stride past the end (the handle then keeps the 28-bit
// copy).
inline bool build_directory(const uint32_t* counts, uint64_t nrec, uint32_t* dir) {
    uint64_t at = 0;
    for (uint64_t r = 0; r < nrec; ++r) {
        dir[r] = (uint32_t)at;
        at += counts[r];
        if (at > DIR_MAX) return false;
    }
    dir[nrec] = (uint32_t)at;
    return true;
}

// ---- where things are ---------------------------------------------------------------------------------------------------------
RRI_XPACK_FN uint64_t record_index(uint64_t q, uint64_t p, uint64_t panels) { return q * panels + p; }
RRI_XPACK_FN uint64_t record_offset(uint64_t q, uint64_t p, uint64_t panels) { return record_index(q, p, panels) * RECORD_BYTES; }
// byte offset, inside its record, of dword k of lane `lane`: six slots of 16 bytes per lane, then one of 8
RRI_XPACK_FN uint32_t dword_offset(uint32_t k, uint32_t lane) {
    return k < 4u * WIDE_SLOTS ? (k / 4u) * (LANES * 16u) + lane * 16u + (k % 4u) * 4u
                               : WIDE_SLOTS * (LANES * 16u) + lane * 8u + (k - 4u * WIDE_SLOTS) * 4u;
}
// bit j of the mantissa / of the code of element (u, e) as 32 * (dword of the lane) + (bit of that dword)
RRI_XPACK_FN uint32_t mant_bit(uint32_t u, uint32_t e, uint32_t j) { return MANT_BITS * (COLS * u + e) + j; }
RRI_XPACK_FN uint32_t code_bit(uint32_t u, uint32_t e, uint32_t j) {
    if (u < 6u) return 32u * (CODE_DWORD + u / 2u) + 8u * e + 3u * (u % 2u) + j;
    if (j < 2u) return 32u * (CODE_DWORD + (u - 6u)) + 8u * e + 6u + j;
    return 32u * (CODE_DWORD + 2u) + 8u * e + u;
}
RRI_XPACK_FN uint32_t entry_of(uint32_t lane, uint32_t i, uint32_t rare_index) { return (lane * ELEMS + i) | (rare_index << POS_BITS); }
// where the pass parks the exponent byte of the element at position pos: a wave-private map of 8 rows, in which row u is 64
// dwords (lane l's four exponent bytes of row u in dword l) at a stride of map_row_bytes
RRI_XPACK_FN uint32_t map_offset(uint32_t pos, uint32_t map_row_bytes) {
    return (pos >> 2 & 7u) * map_row_bytes + (pos >> 5) * 4u + (pos & 3u);
}

// ---- a lane's 8 x 4 elements -> its 26 dwords and its exception entries -------------------------------------------------------
// rows_valid: rows 0 .. rows_valid - 1 of the lane are elements of X (0 for a lane past the last column); the others are padding.
// cls: the classes of choose_books.  Entries go to exc[0 .. nexc - 1] in the order of i; exc == nullptr only counts.
// neither: an element of X is negative or its exponent byte is in neither book (its tile must be flagged; it gets code 0).
RRI_XPACK_FN void encode_lane(const uint32_t (&bits)[ROWS][COLS], uint32_t rows_valid, const uint8_t* cls, uint32_t lane,
                              uint32_t (&out)[LANE_DWORDS], uint16_t* exc, uint32_t& nexc, bool& neither) {
#pragma unroll
    for (int k = 0; k < (int)LANE_DWORDS; ++k) out[k] = 0u;
    nexc = 0u;
    neither = false;
#pragma unroll
    for (uint32_t u = 0; u < ROWS; ++u)
#pragma unroll
        for (uint32_t e = 0; e < COLS; ++e) {
            if (u >= rows_valid) continue;
            const uint32_t b = bits[u][e];
            const uint32_t c = (b >> 31) ? (uint32_t)CLS_NONE : (uint32_t)cls[b >> 23];
            uint32_t code = 0u;
            if (c == CLS_NONE) { neither = true; continue; }
            if (c >= CLS_RARE) {
                code = CODE_EXC;
                if (exc) exc[nexc] = (uint16_t)entry_of(lane, COLS * u + e, c - CLS_RARE);
                ++nexc;
            } else code = c;
            const uint32_t m = b & 0x7fffffu, at = mant_bit(u, e, 0);
            out[at / 32u] |= m << (at % 32u);
            if (at % 32u + MANT_BITS > 32u) out[at / 32u + 1u] |= m >> (32u - at % 32u);
#pragma unroll
            for (uint32_t j = 0; j < 3u; ++j) {
                const uint32_t cb = code_bit(u, e, j);
                out[cb / 32u] |= (code >> j & 1u) << (cb % 32u);
            }
        }
}

// the four byte selectors of row u from the code dwords
RRI_XPACK_FN uint32_t row_selectors(uint32_t c0, uint32_t c1, uint32_t c2, int u) {
    if (u < 6) {
        const uint32_t c = u < 2 ? c0 : u < 4 ? c1 : c2;
        return (u % 2 ? c >> 3 : c) & 0x07070707u;
    }
    return ((u == 6 ? c0 : c1) >> 6 & 0x03030303u) | (c2 >> (u == 6 ? 4 : 5) & 0x04040404u);
}
// row u of a lane: its four fp32 bit patterns from the lane's 26 dwords, the book and `mapped`, the four exponent bytes the
// exception entries of the record gave this row of this lane (0 where the element has none).  With u a compile-time constant
// every index and shift below is one too: funnel shifts, bit-field inserts and byte permutes.
RRI_XPACK_FN void decode_row(const uint32_t (&in)[LANE_DWORDS], int u, uint32_t mapped, uint32_t book_lo, uint32_t book_hi,
                             uint32_t (&bits)[COLS]) {
    const uint32_t sel = row_selectors(in[CODE_DWORD], in[CODE_DWORD + 1], in[CODE_DWORD + 2], u);
    const uint32_t ex = perm(book_hi, book_lo, sel) | mapped;            // code 7 selects byte 7 of the book: 0
    const uint32_t pa = perm(0u, ex, 0x0c010c00u), pb = perm(0u, ex, 0x0c030c02u);     // (E0, 0, E1, 0), (E2, 0, E3, 0)
    const uint32_t t[COLS] = {pa << 23, pa << 7, pb << 23, pb << 7};     // the exponent at bits 23..30, bit 31 clear
    for (int e = 0; e < (int)COLS; ++e) {
        const int at = (int)MANT_BITS * ((int)COLS * u + e), k = at / 32, s = at % 32;
        const uint32_t m = s == 0 ? in[k] : s + (int)MANT_BITS <= 32 ? in[k] >> s : (in[k] >> s | in[k + 1] << (32 - s));
        bits[e] = (m & 0x007fffffu) | (t[e] & 0xff800000u);
    }
}

}  // namespace xnarrow
}  // namespace rri
